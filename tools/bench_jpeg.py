#!/usr/bin/env python3
"""Time the ways an 8-bit image stack on the device becomes image files in memory, the arms alternating in one process (cf. bench_png.py):

    (a) pillow   images.cpu().numpy() + Pillow's Image.save(format="JPEG", quality=q, subsampling=...) into a BytesIO per image
    (b) device   codecs.jpeg_encode(images, q, subsampling): sizing step, read of the sizes, writing step, D2H copy of the files
    (c) png      codecs.png_encode(images) of the same pixels: what the device wrote before there was a JPEG mode
    (d) device, optimize=True   every file with its own Huffman tables (two more launches: jpeg_stats_kernel, jpeg_build_kernel)
    (e) pillow, optimize=True   libjpeg's own two-pass optimisation of the same pixels

on photograph-shaped images (low-pass noise plus grain, as tests/test_native.py::_photo) at 512x512, 16 x 512x1536 (the sample montages of one training
batch), 2048x4096 and 4096x6144, for both subsamplings.  Wall-clock ms per image after a synchronize (every arm ends on the host), `--rounds` windows
per arm, sorted.  Per size also: the file sizes device / Pillow, and the device arm's time per launch from the library's HIP-event records
(uegan_profile_begin / _end).  "size_ratio_96x128" holds device / Pillow on the image tests/test_jpeg.py::test_size_against_pillow bounds (same
generator, same seed), with the two larger test images beside it; "optimize_ratio_*" holds optimised / standard for the device and for Pillow on the
images tests/test_jpeg_optimize.py::test_optimized_is_smaller asks to shrink.  Writes one JSON document (default profiles/jpeg_bench.json) and prints it as one line.

    python tools/bench_jpeg.py [--rounds 5] [--quality 95] [--out profiles/jpeg_bench.json] [--sizes 512x512x1,...]
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
PILLOW_SS = {"4:4:4": 0, "4:2:0": 2}


def photo(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(b, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    x = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False) + 0.03 * torch.randn(b, 3, h, w, generator=g)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pillow_arm(images, quality, ss, optimize=False):
    host = images.cpu().numpy()
    out = []
    for i in range(host.shape[0]):
        f = io.BytesIO()
        Image.fromarray(host[i], "RGB").save(f, format="JPEG", quality=quality, subsampling=PILLOW_SS[ss], optimize=optimize)
        out.append(f.getvalue())
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches(images, quality, ss, calls, optimize=False):
    """ms per launch of codecs.jpeg_encode's kernels from the library's event records, mean over `calls` calls"""
    lib = _lib.load()
    _lib.check(lib.uegan_profile_begin(8 * calls))
    for _ in range(calls):
        codecs.jpeg_encode(images, quality, ss, optimize=optimize)
    entries = (_lib.ProfileEntry * 16)()
    n = ctypes.c_int(0)
    _lib.check(lib.uegan_profile_end(entries, 16, ctypes.byref(n)))
    return {entries[i].name.decode(): round(entries[i].total_ms / entries[i].launches, 5) for i in range(n.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    ap.add_argument("--sizes", default=",".join("%dx%dx%d" % s for s in SIZES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py needs a GPU")
    dev = torch.device("cuda:0")
    q = args.quality
    out = {"what": "8-bit images on the device -> image files in host memory: Pillow's JPEG save on the host vs codecs.jpeg_encode vs codecs.png_encode, wall-clock "
                   "ms per image (sorted, one value per alternating window)", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "quality": q,
           "sizes": {}}
    for spec in args.sizes.split(","):
        h, w, b = (int(v) for v in spec.split("x"))
        images = photo(1990 + h, b, h, w).to(dev)
        png_files = codecs.png_encode(images)                      # (warm-up of the device arms; Pillow needs none)
        rec = {"batch": b, "png_file_bytes": sum(len(f) for f in png_files)}
        t_png = []
        for ss in PILLOW_SS:
            files = codecs.jpeg_encode(images, q, ss)
            ref = pillow_arm(images, q, ss)
            for i in (0, b - 1):
                src = images[i].cpu().numpy().astype(int)
                with Image.open(io.BytesIO(files[i])) as im, Image.open(io.BytesIO(ref[i])) as want:
                    err, err_ref = np.abs(np.array(im).astype(int) - src).mean(), np.abs(np.array(want).astype(int) - src).mean()
                    assert im.size == (w, h) and err <= err_ref + 0.1, "the device's file is further from its image than Pillow's: %.3f vs %.3f levels" % (err, err_ref)
            files_opt = codecs.jpeg_encode(images, q, ss, optimize=True)
            ref_opt = pillow_arm(images, q, ss, True)
            for i in (0, b - 1):                                    # own tables: other bytes, the same pixels
                with Image.open(io.BytesIO(files[i])) as im, Image.open(io.BytesIO(files_opt[i])) as im_opt:
                    assert np.array_equal(np.array(im), np.array(im_opt)), "the optimised file decodes to other pixels than the standard one"
            t_host, t_dev, t_host_opt, t_dev_opt = [], [], [], []
            for _ in range(args.rounds):
                t_host.append(wall_ms(lambda: pillow_arm(images, q, ss)) / b)
                t_dev.append(wall_ms(lambda: codecs.jpeg_encode(images, q, ss)) / b)
                t_host_opt.append(wall_ms(lambda: pillow_arm(images, q, ss, True)) / b)
                t_dev_opt.append(wall_ms(lambda: codecs.jpeg_encode(images, q, ss, optimize=True)) / b)
                if ss == "4:4:4":
                    t_png.append(wall_ms(lambda: codecs.png_encode(images)) / b)
            t_host.sort()
            t_dev.sort()
            spread = max(t_host[-1] - t_host[0], t_dev[-1] - t_dev[0])
            med_host, med_dev = t_host[len(t_host) // 2], t_dev[len(t_dev) // 2]
            per_launch = launches(images, q, ss, 3)
            t_host_opt.sort()
            t_dev_opt.sort()
            spread_opt = max(t_host_opt[-1] - t_host_opt[0], t_dev_opt[-1] - t_dev_opt[0], t_dev[-1] - t_dev[0])
            med_host_opt, med_dev_opt = t_host_opt[len(t_host_opt) // 2], t_dev_opt[len(t_dev_opt) // 2]
            per_launch_opt = launches(images, q, ss, 3, True)
            n_dev, n_opt, n_ref, n_ref_opt = (sum(len(f) for f in fs) for fs in (files, files_opt, ref, ref_opt))
            rec[ss] = {"pillow_ms_per_image": [round(t, 3) for t in t_host], "device_ms_per_image": [round(t, 3) for t in t_dev], "spread_ms": round(spread, 3),
                       "speedup_of_medians": round(med_host / med_dev, 1), "device_not_slower_beyond_spread": bool(med_dev <= med_host + spread),
                       "file_bytes_device": sum(len(f) for f in files), "file_bytes_pillow": sum(len(f) for f in ref),
                       "size_ratio_device_over_pillow": round(sum(len(f) for f in files) / sum(len(f) for f in ref), 4),
                       "device_ms_per_launch": per_launch, "device_kernels_ms_per_call": round(sum(per_launch.values()), 4),
                       "optimize": {"pillow_ms_per_image": [round(t, 3) for t in t_host_opt], "device_ms_per_image": [round(t, 3) for t in t_dev_opt],
                                    "spread_ms": round(spread_opt, 3), "speedup_of_medians_over_pillow_optimize": round(med_host_opt / med_dev_opt, 1),
                                    "device_not_slower_than_pillow_optimize_beyond_spread": bool(med_dev_opt <= med_host_opt + spread_opt),
                                    "device_ms_optimize_minus_standard": round(med_dev_opt - med_dev, 3),
                                    "file_bytes_device": n_opt, "file_bytes_pillow": n_ref_opt,
                                    "size_ratio_device_optimize_over_standard": round(n_opt / n_dev, 4),
                                    "size_ratio_pillow_optimize_over_standard": round(n_ref_opt / n_ref, 4),
                                    "device_ms_per_launch": per_launch_opt, "device_kernels_ms_per_call": round(sum(per_launch_opt.values()), 4)}}
            del files, ref, files_opt, ref_opt
        t_png.sort()
        rec["png_device_ms_per_image"] = [round(t, 3) for t in t_png]
        out["sizes"]["%dx%dx%d" % (h, w, b)] = rec
        print(json.dumps({"%dx%dx%d" % (h, w, b): rec}), flush=True)
        del images, png_files
    # the images tests/test_jpeg.py::test_size_against_pillow bounds (same generator, same seeds); its bound is the 96 x 128 ratio + 0.02
    for h, w in ((96, 128), (512, 512), (1024, 1536)):
        images = photo(60 + h % 7, 1, h, w).to(dev)
        out["size_ratio_%dx%d" % (h, w)] = {"q%d %s" % (quality, ss): round(len(codecs.jpeg_encode(images, quality, ss)[0]) / len(pillow_arm(images, quality, ss)[0]), 4)
                                            for quality in (90, 95) for ss in PILLOW_SS}
    # the images tests/test_jpeg_optimize.py::test_optimized_is_smaller asks to shrink (same generator, same seeds), Pillow's own pair beside them
    for h, w in ((96, 128), (256, 384), (512, 512), (1024, 1536)):
        images = photo(60 + h % 7, 1, h, w).to(dev)
        rec = {}
        for quality in (75, 95):
            for ss in PILLOW_SS:
                std, opt = codecs.jpeg_sizes(images, quality, ss)[0], codecs.jpeg_sizes(images, quality, ss, optimize=True)[0]
                rec["q%d %s" % (quality, ss)] = {"device": round(opt / std, 4),
                                                 "pillow": round(len(pillow_arm(images, quality, ss, True)[0]) / len(pillow_arm(images, quality, ss)[0]), 4)}
        out["optimize_ratio_%dx%d" % (h, w)] = rec
    out["optimize_not_slower_than_pillow_optimize_at_every_size"] = all(r[ss]["optimize"]["device_not_slower_than_pillow_optimize_beyond_spread"]
                                                                        for r in out["sizes"].values() for ss in PILLOW_SS)
    out["device_not_slower_at_every_size"] = all(r[ss]["device_not_slower_beyond_spread"] for r in out["sizes"].values() for ss in PILLOW_SS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
