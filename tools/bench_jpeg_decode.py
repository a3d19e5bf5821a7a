#!/usr/bin/env python3
"""Time the two ways a baseline JPEG file in host memory becomes 8-bit RGB pixels on the device, the arms alternating in one process (the method
of bench_jpeg.py):

    (a) pillow   Image.open(BytesIO(file)).convert("RGB") on the host, then the H2D copy of the pixels
    (b) device   codecs.jpeg_decode([file]): header parsed on the host, H2D copy of the file, every per-byte step on the device

on photograph-shaped images (low-pass noise plus grain, as bench_jpeg.py's) written by Pillow at quality 95 in 4:4:4 and 4:2:0, with and without
restart_marker_rows=1, at 512x512, 16 x 512x1536, 2048x4096 and 4096x6144.  Wall-clock ms per image after a synchronize, `--rounds` windows per arm,
sorted.  Per case also, from one more call: the HIP-event time of the device arm's launches split into unstuff / rounds / write pass / pixels, the
synchronisation rounds used and the sub-sequence count.  The pixels of both arms are compared (torch.equal) before anything is timed.

`loader`: images per second of data.get_train_loader alone (no training step) under either decoder with 16 workers, on a synthetic tree of
2-megapixel JPEG files (4:2:0, quality 95).

Writes one JSON document (default profiles/jpeg_decode_bench.json) and prints it as one line.

    python tools/bench_jpeg_decode.py [--rounds 5] [--out profiles/jpeg_decode_bench.json] [--sizes 512x512x1,...] [--loader-files 32]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import codecs, data  # noqa: E402

SIZES = [(512, 512, 1), (512, 1536, 16), (2048, 4096, 1), (4096, 6144, 1)]      # h, w, batch
PILLOW_SS = {"4:4:4": 0, "4:2:0": 2}


def photo(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(b, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    x = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False) + 0.03 * torch.randn(b, 3, h, w, generator=g)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def write(pixels, quality, ss, restart):
    f = io.BytesIO()
    kw = {"restart_marker_rows": 1} if restart else {}
    Image.fromarray(pixels, "RGB").save(f, format="JPEG", quality=quality, subsampling=PILLOW_SS[ss], **kw)
    return f.getvalue()


def pillow_arm(files, dev):
    out = []
    for blob in files:
        with Image.open(io.BytesIO(blob)) as im:
            out.append(torch.from_numpy(np.asarray(im.convert("RGB"))).to(dev))
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stages(blob, dev):
    info = codecs.jpeg_info(blob)
    f = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    px = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=dev)
    res = codecs.jpeg_decode_into(info, f, px, timings=True)
    names = ("unstuff", "rounds", "write_pass", "pixels")
    return {"rounds": res["rounds"], "subsequences": res["subsequences"], "intervals": res["intervals"], "file_bytes": len(blob),
            "event_ms": {n: round(v, 4) for n, v in zip(names, res["stage_ms"])}, "event_ms_total": round(sum(res["stage_ms"]), 4)}


def loader_rate(root, dec, dev, passes):
    loader = data.get_train_loader(root, 512, 256, batch_size=8, shuffle=True, num_workers=16, device=dev, generator=torch.Generator().manual_seed(1),
                                   decode=dec)
    try:
        n = sum(b.img_exp.shape[0] for b in loader)          # warm-up pass: sizes remembered, buffers made
        torch.cuda.synchronize()
        rates = []
        for _ in range(passes):
            t0 = time.perf_counter()
            n = sum(b.img_exp.shape[0] for b in loader)
            torch.cuda.synchronize()
            rates.append(2 * n / (time.perf_counter() - t0))          # two files per sample
        return sorted(round(r, 1) for r in rates), loader.fallbacks
    finally:
        loader.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    ap.add_argument("--sizes", default=",".join("%dx%dx%d" % s for s in SIZES))
    ap.add_argument("--loader-files", type=int, default=32, help="pairs of 2-megapixel files of the loader measurement (0: skip it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py needs a GPU")
    dev = torch.device("cuda:0")
    q = args.quality
    out = {"what": "baseline JPEG files in host memory -> 8-bit RGB pixels on the device: Pillow's decode + H2D copy of the pixels vs codecs.jpeg_decode, "
                   "wall-clock ms per image (sorted, one value per alternating window); every number measured on the device named here",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "quality": q, "subseq_bits": codecs.JPEG_SUBSEQ_BITS,
           "max_rounds": codecs.JPEG_MAX_ROUNDS, "sizes": {}}
    most_rounds = 0
    for spec in args.sizes.split(","):
        h, w, b = (int(v) for v in spec.split("x"))
        images = photo(1990 + h, b, h, w).numpy()
        rec = {"batch": b}
        for ss in PILLOW_SS:
            for restart in (False, True):
                files = [write(images[i], q, ss, restart) for i in range(b)]
                got, want = codecs.jpeg_decode(files, dev), pillow_arm(files, dev)          # (also the warm-up)
                assert all(torch.equal(g[0], x) for g, x in zip(got, want)), "the device's pixels are not Pillow's"
                del got, want
                t_host, t_dev = [], []
                for _ in range(args.rounds):
                    t_host.append(wall_ms(lambda: pillow_arm(files, dev)) / b)
                    t_dev.append(wall_ms(lambda: codecs.jpeg_decode(files, dev)) / b)
                t_host.sort()
                t_dev.sort()
                spread = max(t_host[-1] - t_host[0], t_dev[-1] - t_dev[0])
                med_host, med_dev = t_host[len(t_host) // 2], t_dev[len(t_dev) // 2]
                st = stages(files[0], dev)
                most_rounds = max(most_rounds, st["rounds"])
                rec["%s%s" % (ss, " restart rows" if restart else "")] = {
                    "pillow_ms_per_image": [round(t, 3) for t in t_host], "device_ms_per_image": [round(t, 3) for t in t_dev], "spread_ms": round(spread, 3),
                    "speedup_of_medians": round(med_host / med_dev, 2), "device_faster_beyond_spread": bool(med_dev + spread < med_host),
                    "device_slower_beyond_spread": bool(med_dev > med_host + spread), "first_file": st}
        out["sizes"]["%dx%dx%d" % (h, w, b)] = rec
        print(json.dumps({"%dx%dx%d" % (h, w, b): rec}), flush=True)
    out["largest_round_count"] = most_rounds
    out["device_faster_beyond_spread_at_every_size"] = all(c["device_faster_beyond_spread"] for r in out["sizes"].values() for k, c in r.items() if k != "batch")
    if args.loader_files > 0:
        with tempfile.TemporaryDirectory() as tmp:
            for d in ("exp", "raw"):
                os.makedirs(os.path.join(tmp, d))
            base = photo(7, 4, 1152, 1728).numpy()          # 2.0 megapixels
            for i in range(args.loader_files):
                for k, d in enumerate(("exp", "raw")):
                    with open(os.path.join(tmp, d, "im%03d.jpg" % i), "wb") as f:
                        f.write(write(np.roll(base[(i + k) % 4], 37 * i, axis=1), q, "4:2:0", False))
            lo = {}
            for dec in ("host", "device", "host", "device"):
                rates, fallbacks = loader_rate(tmp, dec, dev, 2)
                lo.setdefault(dec, []).extend(rates)
                assert fallbacks == 0
            out["loader"] = {"what": "get_train_loader alone, crop 512 -> 256, batch 8, 16 thread workers, %d pairs of 1152x1728 4:2:0 files: files decoded per "
                                     "second, one value per pass, the decoders alternating" % args.loader_files,
                             "host_files_per_s": sorted(lo["host"]), "device_files_per_s": sorted(lo["device"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
