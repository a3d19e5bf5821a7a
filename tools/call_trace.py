#!/usr/bin/env python3
"""Record which C-ABI entry points a fixed small workload reaches, in order, with their plain integer and float arguments (pointers, streams and
structs are left out; an integer result such as a workspace size is kept) -- and a hash of each leg's sequence.  Two trees that print the same hashes
issue the same calls in the same order: the check for a change that moves host code around without touching a kernel.

The only thing replaced is `_lib.load`: what it returns is wrapped in a recording proxy, so every module that finds the library through it is seen,
and the script runs unchanged on any commit that has the public API it drives.  Runs on the GPU when one is visible, else on the CPU emulator.

    legs   train_f32, train_bf16   two Trainer.train_step calls: conv_dim 8, batch 1, 96 x 96 (the smallest square the discriminator's five
                                   stride-2 stages and reflection padding accept), seeded VGG stand-in at 1/8 width
           eval_bf16               one eval-mode generator forward of a 64 x 64 image (the generator alone accepts the smaller size)
           test_png / test_jpeg / test_jpeg_opt   one tester.run_test batch (two 32 x 32 images) written by the device PNG encoder, as JPEG, as
                                   optimised JPEG
           tiled                   one tester.enhance_native(tile=32) of a 33 x 47 image (four tiles)

    python tools/call_trace.py [--calls] [--out trace.json]        --calls: print every call, not only the per-leg hashes
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import _lib, data, losses, models, ops, tester, trainer  # noqa: E402

LOG = []


def _plain(t):
    return isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t._type_ in "bBhHiIlLqQfd"


class _Recorder:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in _lib.SIGNATURES:
            return fn
        kinds = [_plain(t) for t in _lib.SIGNATURES[name][1]]

        def call(*args):
            res = fn(*args)
            vals = [a.value if isinstance(a, ctypes._SimpleCData) else a for a, k in zip(args, kinds) if k]
            LOG.append([name, vals, res if isinstance(res, int) else None])
            return res
        return call


def _device():
    if torch.cuda.is_available():
        return torch.device("cuda:0")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["bash", os.path.join(emu, "build_emu.sh")], check=True, capture_output=True)
    _lib._inject_for_tests(os.path.join(emu, "_build", "libuegan_emu.so"), os.path.join(emu, "_build", "libuegan_emu_f16.so"))
    return torch.device("cpu")


def _nets(dev):
    torch.manual_seed(1990)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    P = losses.PerceptualLoss(vgg_weights="seeded", width_div=8)
    if dev.type != "cpu":
        G, D, P = G.to(dev), D.to(dev), P.to(dev)
    return G, D, P


def _train(dev, dtype):
    ops.set_compute_dtype(dtype)
    G, D, P = _nets(dev)
    T = trainer.Trainer(G, D, P, pool_size=3, rng=random.Random(1990))
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        raw = (torch.rand(1, 3, 96, 96, generator=g) * 2 - 1).to(dev)
        exp = (torch.rand(1, 3, 96, 96, generator=g) * 2 - 1).to(dev)
        T.train_step(raw, exp)
        T.loss_items()
    T.sync()
    return G


def _tree(root):
    from PIL import Image
    rng = np.random.RandomState(5)
    for sub in ("exp", "raw"):
        os.makedirs(os.path.join(root, sub))
        for i in range(2):
            Image.fromarray(rng.randint(0, 256, (32, 32, 3)).astype(np.uint8), "RGB").save(os.path.join(root, sub, "im%02d.png" % i))


def _run_test(G, dev, root, out):
    loader = data.get_test_loader(root, 32, 2, False, 2, device=dev)
    try:
        tester.run_test(G, loader, save_dir=out, tag="1.00")
    finally:
        loader.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", action="store_true", help="print every recorded call")
    ap.add_argument("--out", default=None, help="also write the sequences and hashes to this JSON file")
    args = ap.parse_args()
    dev = _device()
    real = _lib.load
    _lib.load = lambda *a, **k: _Recorder(real(*a, **k))
    legs = {}

    def leg(name, fn):
        del LOG[:]
        res = fn()
        if dev.type != "cpu":
            torch.cuda.synchronize()
        legs[name] = list(LOG)
        return res

    leg("train_f32", lambda: _train(dev, torch.float32))
    G = leg("train_bf16", lambda: _train(dev, torch.bfloat16))
    x = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    with torch.no_grad():
        leg("eval_bf16", lambda: tester.enhance(G, x))
    ops.set_compute_dtype(torch.float32)
    with tempfile.TemporaryDirectory() as tmp:
        _tree(os.path.join(tmp, "src"))
        try:
            tester.set_png_encoder("device")
            leg("test_png", lambda: _run_test(G, dev, os.path.join(tmp, "src"), os.path.join(tmp, "png")))
            tester.set_image_format("jpeg", 90, "4:2:0")
            leg("test_jpeg", lambda: _run_test(G, dev, os.path.join(tmp, "src"), os.path.join(tmp, "jpg")))
            tester.set_image_format("jpeg", 90, "4:2:0", optimize=True)
            leg("test_jpeg_opt", lambda: _run_test(G, dev, os.path.join(tmp, "src"), os.path.join(tmp, "jpgo")))
        finally:
            tester.set_image_format("png")
            tester.set_png_encoder("pillow")
    pix = torch.randint(0, 256, (1, 33, 47, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).to(dev)
    G.eval()
    leg("tiled", lambda: tester.enhance_native(G, pix, tile=32))
    _lib.load = real

    hashes = {}
    for name, calls in legs.items():
        lines = ["%s %s -> %s" % (n, " ".join(repr(v) for v in vals), res) for n, vals, res in calls]
        if args.calls:
            print("== %s" % name)
            print("\n".join(lines))
        hashes[name] = {"calls": len(calls), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]}
    for name, h in hashes.items():
        print("%-14s %5d calls  %s" % (name, h["calls"], h["sha256"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"backend": dev.type, "hashes": hashes, "legs": legs}, f)


if __name__ == "__main__":
    main()
