#!/usr/bin/env python3
"""Time tiled native-size inference (`tester.enhance_native(tile=)`) on the GPU in the three storage modes, with HIP events after
warm-up, the two arms alternating in one process:

    case 1   2048 x 4096 (the untiled cap)   tester.enhance_native(G, pix)  vs  tester.enhance_native(G, pix, tile=1024): ms and the ratio
    case 2   4096 x 6144 (above the cap)     tiled only: ms and the peak device memory

There is no speed target.  The expected overhead of tiling is the halo area, ((1024 + 2 * 80) / 1024)^2 = 1.34 for an interior tile (less at the
image's border, where a tile is clipped), plus the encoder-only first pass; the document records how close the ratio lands.  conv_dim 32, batch 1,
randomly initialised weights (time does not depend on them).  Writes one JSON document (default profiles/tiled_bench.json) and prints it as one line.

    python tools/bench_tiled.py [--rounds 3] [--iters 2] [--out profiles/tiled_bench.json] [--skip-large]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import data, models, ops, tester  # noqa: E402

MODES = (("float32", torch.float32), ("bfloat16", torch.bfloat16), ("float16", torch.float16))


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def halo_area_ratio(hp, wp, core, halo):
    """pixels the tiled passes run the network on, over the image's: (pass 2, pass 1)"""
    def area(h):
        return sum((t[5] - t[4]) * (t[7] - t[6]) for t in data.native_tiles(hp, wp, core, h))
    return area(halo) / (hp * wp), area(data.NATIVE_TILE_HALO_ENC) / (hp * wp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_bench.json"))
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled.py needs a GPU")
    dev = torch.device("cuda:0")
    T = data.NATIVE_TILE
    out = {"what": "tiled native-size inference, ms per image (sorted, one value per alternating window of `iters` calls)", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "iters_per_window": args.iters, "tile": T, "halo": data.NATIVE_TILE_HALO, "halo_enc": data.NATIVE_TILE_HALO_ENC, "conv_dim": 32}
    g = torch.Generator().manual_seed(1990)
    h, w = 2048, 4096
    pix = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
    a2, a1 = halo_area_ratio(h, w, T, data.NATIVE_TILE_HALO)
    case1 = {"size": [h, w], "tiles": len(data.native_tiles(h, w, T, 0)), "pass2_area_over_image": round(a2, 4), "pass1_area_over_image": round(a1, 4), "modes": {}}
    for name, dt in MODES:
        ops.set_compute_dtype(dt)
        torch.manual_seed(41)
        G = models.Generator(32, "none", "LeakyReLU", False).to(dev)
        for _ in range(2):
            tester.enhance_native(G, pix)
            tester.enhance_native(G, pix, tile=T)
        torch.cuda.synchronize()
        t_un, t_ti = [], []
        for _ in range(args.rounds):
            t_un.append(window_ms(lambda: tester.enhance_native(G, pix), args.iters))
            t_ti.append(window_ms(lambda: tester.enhance_native(G, pix, tile=T), args.iters))
        t_un.sort()
        t_ti.sort()
        ratio = t_ti[len(t_ti) // 2] / t_un[len(t_un) // 2]
        differ = int((tester.enhance_native(G, pix) != tester.enhance_native(G, pix, tile=T)).sum())
        case1["modes"][name] = {"untiled_ms": [round(t, 3) for t in t_un], "tiled_ms": [round(t, 3) for t in t_ti], "tiled_over_untiled": round(ratio, 3),
                                "ratio_over_pass2_area": round(ratio / a2, 3), "bytes_that_differ": differ, "of_bytes": h * w * 3}
        del G
    out["case_2048x4096"] = case1
    del pix
    if not args.skip_large:
        h, w = 4096, 6144
        assert h * w == data.NATIVE_TILED_MAX_PIXELS
        pix = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8).to(dev)
        case2 = {"size": [h, w], "tiles": len(data.native_tiles(h, w, T, 0)), "modes": {}}
        for name, dt in MODES:
            ops.set_compute_dtype(dt)
            torch.manual_seed(41)
            G = models.Generator(32, "none", "LeakyReLU", False).to(dev)
            q = tester.enhance_native(G, pix, tile=T)
            torch.cuda.synchronize()
            assert tuple(q.shape) == (1, h, w, 3)
            torch.cuda.reset_peak_memory_stats()
            ms = sorted(window_ms(lambda: tester.enhance_native(G, pix, tile=T), 1) for _ in range(args.rounds))
            case2["modes"][name] = {"tiled_ms": [round(t, 3) for t in ms], "peak_device_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
            del G, q
        out["case_4096x6144"] = case2
    ops.set_compute_dtype(torch.float32)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
