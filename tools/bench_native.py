#!/usr/bin/env python3
"""Time the two kernels of native-size inference (`--test_img_size 0`) on the GPU against the composition of operations that served before
them, with HIP events after warm-up, the two arms alternating in one process:

    input side    data.native_input(pix)                          vs  F.pad(data.input_transform(pix, (h, w)), ..., mode="reflect")
    output side   tester.montage_u8(*xs, window=(h, w)), n = 1, 2  vs  tester.montage_u8(*[x[:, :, :h, :w].contiguous() for x in xs])

at 500x333, 1024x683 and 2000x3008 (h x w), the achieved bytes/s of each new kernel over the bytes its algorithm needs (input: 3 B read per
source pixel + 12 B written per padded pixel; output: 12 B read + 3 B written per window pixel and panel), and -- for information -- the eager
end-to-end tester.enhance_native at 500x333 in the three storage modes.  Writes one JSON document (default profiles/native_bench.json) and
prints it as one line.

    python tools/bench_native.py [--rounds 5] [--out profiles/native_bench.json] [--no-e2e]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import data, models, ops, tester  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification
SIZES = [(500, 333), (1024, 683), (2000, 3008)]


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def ab(old, new, iters, rounds):
    """`rounds` alternating windows of `iters` calls per arm -> sorted ms per call of each arm, and the verdict: the new arm's median is not
    above the old one's by more than the larger of the two arms' own spreads (max - min over the rounds)"""
    for _ in range(5):
        old()
        new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(rounds):
        t_old.append(window_ms(old, iters))
        t_new.append(window_ms(new, iters))
    t_old.sort()
    t_new.sort()
    spread = max(t_old[-1] - t_old[0], t_new[-1] - t_new[0])
    med_old, med_new = t_old[len(t_old) // 2], t_new[len(t_new) // 2]
    return {"iters_per_window": iters, "composition_ms": [round(t, 5) for t in t_old], "fused_ms": [round(t, 5) for t in t_new],
            "spread_ms": round(spread, 5), "speedup_of_medians": round(med_old / med_new, 3), "fused_not_slower": bool(med_new <= med_old + spread)}, med_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_bench.json"))
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_native.py needs a GPU")
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.float32)
    out = {"what": "native-size inference: fused kernels vs the composition they replace, ms per call (sorted, one value per alternating window)",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK, "sizes": {}}
    g = torch.Generator().manual_seed(1990)
    for h, w in SIZES:
        hp, wp = data.padded_size(h, w)
        iters = max(20, int(2e8 / (hp * wp)))
        pix = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        rec = {"padded": [hp, wp]}

        def composed_input():
            return F.pad(data.input_transform(pix, (h, w)), (0, wp - w, 0, hp - h), mode="reflect")
        assert torch.equal(data.native_input(pix), composed_input())
        r, med = ab(composed_input, lambda: data.native_input(pix), iters, args.rounds)
        byt = 3 * h * w + 12 * hp * wp
        r["fused_bytes"], r["fused_bytes_per_s"] = byt, round(byt / (med * 1e-3), 1)
        r["fused_hbm_peak_fraction"] = round(byt / (med * 1e-3) / HBM_PEAK, 4)
        rec["input"] = r
        xs = [(torch.rand(1, 3, hp, wp, generator=g) * 2.4 - 1.2).to(dev) for _ in range(2)]
        for n in (1, 2):
            src = xs[:n]

            def composed_output():
                return tester.montage_u8(*[x[:, :, :h, :w].contiguous() for x in src])
            assert torch.equal(tester.montage_u8(*src, window=(h, w)), composed_output())
            r, med = ab(composed_output, lambda: tester.montage_u8(*src, window=(h, w)), iters, args.rounds)
            byt = 15 * h * w * n
            r["fused_bytes"], r["fused_bytes_per_s"] = byt, round(byt / (med * 1e-3), 1)
            r["fused_hbm_peak_fraction"] = round(byt / (med * 1e-3) / HBM_PEAK, 4)
            rec["montage_n%d" % n] = r
        out["sizes"]["%dx%d" % (h, w)] = rec
        del xs, pix
    out["every_fused_kernel_not_slower"] = all(v["fused_not_slower"] for rec in out["sizes"].values() for k, v in rec.items() if k != "padded")
    if not args.no_e2e:
        h, w = SIZES[0]
        pix = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        e2e = {}
        for name, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16)):
            ops.set_compute_dtype(dt)
            torch.manual_seed(41)
            G = models.Generator(32, "none", "LeakyReLU", False).to(dev)
            for _ in range(3):
                tester.enhance_native(G, pix)
            torch.cuda.synchronize()
            e2e[name] = sorted(round(window_ms(lambda: tester.enhance_native(G, pix), 10), 4) for _ in range(3))
        ops.set_compute_dtype(torch.float32)
        out["enhance_native_eager_ms_%dx%d_conv_dim_32" % (h, w)] = e2e
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
