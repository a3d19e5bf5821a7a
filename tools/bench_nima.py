#!/usr/bin/env python3
"""Time the NIMA scorer (uegan_amd/nima.py) on the GPU: ms per image at batch 1, 8 and 32, eager and as one hipGraph, with HIP events after
warm-up, next to the HBM traffic the per-layer design needs (every layer reads its input and writes its output once; computed from the
layer table) and the fraction of the HBM peak that traffic over the measured time amounts to.  Prints one JSON line.

    python tools/bench_nima.py [--iters 50] [--batches 1,8,32] [--once B]      (--once B: one eager batch-B forward, for a kernel trace)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import nima as N  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification


def traffic_bytes():
    """(activation bytes per image, weight bytes per forward) of the per-layer design, fp32, padded channel counts.
    The expanded tensors (written by the expand 1x1, read and written by the depthwise, read by the projection) are listed apart."""
    act = expanded = weights = 0
    h = N.INPUT_SIZE
    act += 3 * h * h * 4                                        # the image
    h //= 2
    cin = N._cp(N.FIRST_CHANNELS)
    act += h * h * cin * 4
    weights += 27 * cin * 4
    for ci, co, s, t in N.block_specs():
        hid, cop, cip = N._cp(ci * t), N._cp(co), N._cp(ci)
        ho = (h - 1) // s + 1
        e = (h * h * hid * 2 + ho * ho * hid * 2) * 4          # expand writes, depthwise reads + writes, projection reads
        expanded += e
        act += h * h * cip * 4 + e + ho * ho * cop * 4 + (ho * ho * cop * 4 if s == 1 and ci == co else 0)
        weights += (hid * cip + 9 * hid + cop * hid + 2 * (2 * hid + cop)) * 4
        h = ho
    last = N._cp(N.LAST_CHANNELS)
    act += h * h * (N._cp(N.block_specs()[-1][1]) + 2 * last) * 4     # last 1x1 reads + writes, the head reads
    weights += (last * N._cp(N.block_specs()[-1][1]) + N.N_SCORES * N.LAST_CHANNELS) * 4
    return act, expanded, weights


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(3):                                          # three windows: the spread is part of the record
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        best.append(a.elapsed_time(b) / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--once", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nima.py needs a GPU")
    dev = torch.device("cuda:0")
    model = N.NIMA()
    model.load_state_dict(N.seeded_state_dict(1))
    model = model.to(dev)
    if args.once:
        x = torch.rand(args.once, 3, 224, 224, device=dev)
        for _ in range(2):
            model(x)
        torch.cuda.synchronize()
        return
    act, expanded, weights = traffic_bytes()
    out = {"what": "NIMA scorer forward, fp32, ms per image (min / median / max of 3 windows of --iters forwards)", "device": torch.cuda.get_device_name(0),
           "iters": args.iters, "hbm_bytes_per_image": act, "of_which_expanded_tensors": expanded, "weight_bytes_per_forward": weights,
           "hbm_peak_bytes_per_s": HBM_PEAK, "batch": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        x = torch.rand(B, 3, 224, 224, device=dev)
        eager = sorted(timed(lambda: model(x), args.iters))
        gr = N.GraphedNIMA(model, B)
        graphed = sorted(timed(lambda: gr(x), args.iters))
        byt = act * B + weights
        out["batch"][str(B)] = {"eager_ms_per_image": [round(t / B, 5) for t in eager], "graphed_ms_per_image": [round(t / B, 5) for t in graphed],
                                "hbm_peak_fraction_eager": round(byt / (eager[1] * 1e-3) / HBM_PEAK, 4),
                                "hbm_peak_fraction_graphed": round(byt / (graphed[1] * 1e-3) / HBM_PEAK, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
