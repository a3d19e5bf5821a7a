#!/usr/bin/env python3
"""Time the two ways an 8-bit image stack on the device becomes PNG files in memory, the two arms alternating in one process (cf. bench_native.py):

    (a) host     images.cpu().numpy() + Pillow's Image.save(format="png") into a BytesIO per image: what tester.write_pngs does by default
    (b) device   codecs.png_encode(images), including its read of the sizes and its D2H copy of the used bytes ("device" encoder)

on photograph-shaped images (low-pass noise plus grain, as tests/test_native.py::_photo) at 512x512, 16 x 512x1536 (the sample montages of one training
batch), 2048x4096 and 4096x6144.  Wall-clock ms per image after a synchronize (both arms end on the host), `--rounds` windows per arm, sorted.  Per
size also: the file-size ratio device / Pillow, the device arm's time per launch from the library's HIP-event records (uegan_profile_begin / _end),
and its bytes/s over the bytes its algorithm needs: pixels read, filtered bytes written and read, the stream written, read, written into the file and
copied to the host.  Writes one JSON document (default profiles/png_bench.json) and prints it as one line.

    python tools/bench_png.py [--rounds 5] [--out profiles/png_bench.json] [--sizes 512x512x1,...]
"""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import _lib, codecs  # noqa: E402

SIZES = [(512, 512, 1), (512, 1536, 16), (2048, 4096, 1), (4096, 6144, 1)]      # h, w, batch


def photo(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(b, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    x = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False) + 0.03 * torch.randn(b, 3, h, w, generator=g)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pillow_arm(images):
    host = images.cpu().numpy()
    out = []
    for i in range(host.shape[0]):
        f = io.BytesIO()
        Image.fromarray(host[i], "RGB").save(f, format="png")
        out.append(f.getvalue())
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches(images, calls):
    """ms per launch of codecs.png_encode's kernels from the library's event records, mean over `calls` calls"""
    lib = _lib.load()
    _lib.check(lib.uegan_profile_begin(8 * calls))
    for _ in range(calls):
        codecs.png_encode(images)
    entries = (_lib.ProfileEntry * 16)()
    n = ctypes.c_int(0)
    _lib.check(lib.uegan_profile_end(entries, 16, ctypes.byref(n)))
    return {entries[i].name.decode(): round(entries[i].total_ms / entries[i].launches, 5) for i in range(n.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bench.json"))
    ap.add_argument("--sizes", default=",".join("%dx%dx%d" % s for s in SIZES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py needs a GPU")
    dev = torch.device("cuda:0")
    out = {"what": "8-bit images on the device -> PNG files in host memory: Pillow on the host vs codecs.png_encode, wall-clock ms per image (sorted, one value "
                   "per alternating window)", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "sizes": {}}
    for spec in args.sizes.split(","):
        h, w, b = (int(v) for v in spec.split("x"))
        images = photo(1990 + h, b, h, w).to(dev)
        files = codecs.png_encode(images)                      # (warm-up of the device arm; Pillow needs none)
        ref = pillow_arm(images)
        for i in (0, b - 1):
            with Image.open(io.BytesIO(files[i])) as im:
                assert torch.equal(torch.from_numpy(np.array(im)), images[i].cpu()), "the device's file does not decode to its image"
        codecs.png_encode(images)
        t_host, t_dev = [], []
        for _ in range(args.rounds):
            t_host.append(wall_ms(lambda: pillow_arm(images)) / b)
            t_dev.append(wall_ms(lambda: codecs.png_encode(images)) / b)
        t_host.sort()
        t_dev.sort()
        spread = max(t_host[-1] - t_host[0], t_dev[-1] - t_dev[0])
        med_host, med_dev = t_host[len(t_host) // 2], t_dev[len(t_dev) // 2]
        stream = sum(len(f) for f in files)
        filtered = b * h * (3 * w + 1)
        need = 3 * b * h * w + 2 * filtered + 4 * stream
        per_launch = launches(images, 3)
        rec = {"batch": b, "pillow_ms_per_image": [round(t, 3) for t in t_host], "device_ms_per_image": [round(t, 3) for t in t_dev],
               "spread_ms": round(spread, 3), "speedup_of_medians": round(med_host / med_dev, 1), "device_faster_beyond_spread": bool(med_dev + spread < med_host),
               "file_bytes_device": stream, "file_bytes_pillow": sum(len(f) for f in ref), "size_ratio_device_over_pillow": round(stream / sum(len(f) for f in ref), 4),
               "device_ms_per_launch": per_launch, "device_kernels_ms_per_call": round(sum(per_launch.values()), 4),
               "device_algorithm_bytes": need, "device_bytes_per_s": round(need / (med_dev * b * 1e-3), 1)}
        out["sizes"]["%dx%dx%d" % (h, w, b)] = rec
        print(json.dumps({"%dx%dx%d" % (h, w, b): rec}), flush=True)
        del images, files, ref
    # the three images tests/test_png.py::test_size_against_pillow bounds at 1.05 (same generator, same seeds)
    out["size_ratio_on_the_test_images"] = {}
    for h, w in ((96, 128), (512, 512), (1024, 1536)):
        images = photo(60 + h % 7, 1, h, w).to(dev)
        out["size_ratio_on_the_test_images"]["%dx%d" % (h, w)] = round(len(codecs.png_encode(images)[0]) / len(pillow_arm(images)[0]), 4)
    out["device_faster_at_every_size"] = all(r["device_faster_beyond_spread"] for r in out["sizes"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
