"""What the command line costs on top of the step, and what the montage kernel buys (profiles/runner_overhead.json).

  runner   ms per step of `runner.train` with the loss line, samples, validation and checkpoints switched off, at 16 x 3 x 512^2 on a generated
           PNG tree, against a bare `InputFetcher` + `Trainer.train_step` loop over the same tree -- same process, alternating, --repeats windows
           each, medians; the bare loop's min..max is the run-to-run spread the difference has to be read against.
  montage  `tester.montage_u8(a, b, c)` for three 16 x 3 x 512^2 sources against three `to_uint8_image` launches + `torch.cat`, device time per call
           from event pairs around --iters calls (median of --repeats windows), and the achieved GB/s against the bytes that must move
           (per element 4 B read + 1 B written).

Both windows start and end at a device synchronisation, after --warmup steps / calls.

    python tools/bench_runner.py --out profiles/runner_overhead.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uegan_amd import config, data, losses, models, ops, runner, tester, trainer  # noqa: E402


def make_tree(root, n, side):
    """n PNG pairs of side x side: smooth fields + mild noise (photographs compress like this, white noise does not)"""
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float32) / side
    for d in ("exp", "raw"):
        os.makedirs(os.path.join(root, d))
        for i in range(n):
            ph = rng.uniform(0, 6.28, size=3)
            img = np.stack([127 + 100 * np.sin(6.28 * (xx * (1 + c) + yy * (i % 5 + 1)) + ph[c]) for c in range(3)], -1)
            img = img + rng.integers(-6, 7, size=img.shape)
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(os.path.join(root, d, "im%03d.png" % i))


class Window:
    """host time between the entry of call `first` and the entry of call `first + count` of a step function, device-synchronised at both"""

    def __init__(self, first, count):
        self.first, self.last, self.calls, self.t0, self.t1 = first, first + count, 0, None, None

    def tick(self):
        if self.calls in (self.first, self.last):
            torch.cuda.synchronize()
            if self.calls == self.first:
                self.t0 = time.perf_counter()
            else:
                self.t1 = time.perf_counter()
        self.calls += 1

    def ms_per_step(self):
        return (self.t1 - self.t0) * 1e3 / (self.last - self.first)


def runner_args(tree, out, steps, a):
    spe = a.pairs // a.batch
    return config.get_config([
        "--mode", "train", "--train_img_dir", tree, "--val_img_dir", tree, "--save_root_dir", out, "--image_size", str(a.size), "--resize_size", str(a.size),
        "--train_batch_size", str(a.batch), "--total_epochs", str((steps + spe - 1) // spe), "--vgg_weights", "seeded", "--compute_dtype", a.dtype,
        "--num_workers", str(a.workers), "--info_step", str(10 ** 9), "--sample_step", str(10 ** 9), "--model_save_epoch", "0",
        "--num_epochs_start_val", str(10 ** 6), "--is_test_nima", "False", "--is_print_network", "False"])


def time_runner(tree, out, a):
    steps = a.warmup + a.steps + 1
    args = runner_args(tree, out, steps, a)
    win = Window(a.warmup, a.steps)
    orig = trainer.Trainer.train_step

    def train_step(self, raw, exp):
        win.tick()
        return orig(self, raw, exp)

    trainer.Trainer.train_step = train_step
    try:
        runner.main(args)
    finally:
        trainer.Trainer.train_step = orig
    return win.ms_per_step()


def time_bare(tree, a):
    """the loop a user of the parent API writes: the same models, loader and Trainer, nothing else"""
    dev = torch.device("cuda:0")
    steps = a.warmup + a.steps + 1
    runner.setup_seed(1990)
    ops.set_compute_dtype(config.COMPUTE_DTYPES[a.dtype])
    G = models.Generator(32, "none", "LeakyReLU", False)
    D = models.Discriminator(32, "none", "LeakyReLU", True, "rahinge")
    runner.init_weights(G, "orthogonal", 0.02)
    runner.init_weights(D, "orthogonal", 0.02)
    P = losses.PerceptualLoss(vgg_weights="seeded")
    loader = data.get_train_loader(tree, a.size, a.size, a.batch, True, a.workers, True, device=dev, generator=runner.loader_generator(1990))
    T = trainer.Trainer(G.to(dev), D.to(dev), P.to(dev))
    fetcher = data.InputFetcher(loader)
    win = Window(a.warmup, a.steps)
    for _ in range(steps):
        batch = next(fetcher)
        win.tick()
        T.train_step(batch.img_raw, batch.img_exp)
    T.sync()
    torch.cuda.synchronize()
    loader.close()
    return win.ms_per_step()


def time_calls(fn, a):
    for _ in range(a.warmup):
        fn()
    out = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / a.iters)
    return sorted(out)


def bench_montage(a):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    xs = [(torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2.4 - 1.2).to(dev) for _ in range(3)]
    assert torch.equal(tester.montage_u8(*xs), torch.cat([tester.to_uint8_image(x) for x in xs], 2))
    one = time_calls(lambda: tester.montage_u8(*xs), a)
    three = time_calls(lambda: torch.cat([tester.to_uint8_image(x) for x in xs], 2), a)
    must = 3 * xs[0].numel() * 5
    return {"shape": [3, a.batch, 3, a.size, a.size], "montage_u8_ms": [round(t, 5) for t in one], "three_quantize_plus_cat_ms": [round(t, 5) for t in three],
            "bytes_that_must_move": must, "montage_u8_GBps": round(must / (statistics.median(one) * 1e-3) / 1e9, 1),
            "three_quantize_plus_cat_GBps_of_the_same_bytes": round(must / (statistics.median(three) * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-runner", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "montage": bench_montage(a)}
    ops.set_compute_dtype(torch.float32)
    if not a.skip_runner:
        with tempfile.TemporaryDirectory() as tmp:
            tree = os.path.join(tmp, "tree")
            make_tree(tree, a.pairs, a.size + 8)
            bare, run = [], []
            for r in range(a.repeats):                   # alternating, back to back, one process
                bare.append(time_bare(tree, a))
                run.append(time_runner(tree, os.path.join(tmp, "out%d" % r), a))
        bare_s, run_s = sorted(bare), sorted(run)
        res["runner"] = {"what": "ms per step, %d x 3 x %d^2 %s, %d timed steps after %d, windows in run order" % (a.batch, a.size, a.dtype, a.steps, a.warmup),
                         "bare_loop_ms": [round(t, 3) for t in bare], "runner_ms": [round(t, 3) for t in run],
                         "bare_median_ms": round(statistics.median(bare_s), 3), "runner_median_ms": round(statistics.median(run_s), 3),
                         "bare_spread_ms": round(bare_s[-1] - bare_s[0], 3),
                         "runner_minus_bare_ms": round(statistics.median(run_s) - statistics.median(bare_s), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
