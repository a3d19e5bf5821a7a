#!/usr/bin/env python3
"""What the dataset cache (DeviceLoader(cache="device")) buys on one MI355X, at the reference's default configuration: a seeded tree of PNG files
(512 x 768, 64 pairs), 512 x 512 crops -> 256 x 256, batch 16.  One process, the arms alternating, 5 windows per arm, every window ending in a
device synchronise; rates are image PAIRS per second (a training sample is a pair), as tools/soak.py counts them.

  loader alone     uncached with 16 thread workers | cached, first pass (a fresh loader and store per window: one pass is all a first pass is, so
                   these windows are short by nature) | cached, later passes
  loader -> step   Trainer.train_step in bf16 (the networks of tools/soak.py) fed by the uncached loader, by the cached loader (its store filled),
                   and the same steps on resident tensors
  transform call   HIP-event time per call of uegan_input_transform on 32 contiguous crops (the old route; the host crop and the copy that bring
                   them there are NOT in this number) and of uegan_input_transform_windows on the same 32 windows of resident images, the calls
                   queued behind a busy device so that the events bracket device work; and the host's time to issue a call

-> profiles/dataset_cache_bench.json (--out).  Needs the GPU: there is no fallback.  --rehearse runs the loader arms and the call timing at a toy
size on the CPU emulator with a host clock, to check the script itself; it writes nothing and its numbers mean nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import uegan_amd  # noqa: E402
from uegan_amd import _lib, data, losses, models, trainer  # noqa: E402

WINDOWS = 5


def make_tree(root, pairs, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for d in ("exp", "raw"):
        os.makedirs(os.path.join(root, d))
        for i in range(pairs):
            low = rng.integers(0, 256, size=(h // 32 + 2, w // 32 + 2, 3)).astype(np.uint8)      # smooth structure: files of a photo's size, not noise
            Image.fromarray(low, "RGB").resize((w, h), Image.BICUBIC).save(os.path.join(root, d, "im%03d.png" % i), compress_level=1)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "windows": values}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--resize", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--passes", type=int, default=6, help="passes per window of the uncached loader")
    ap.add_argument("--cached-passes", type=int, default=60, help="passes per window of the cached loader's later passes")
    ap.add_argument("--steps", type=int, default=24, help="training steps per window")
    ap.add_argument("--calls", type=int, default=50, help="transform calls per window")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_cache_bench.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    if args.rehearse:
        emu = os.path.join(ROOT, "tests", "emu")
        subprocess.run(["bash", os.path.join(emu, "build_emu.sh")], check=True, capture_output=True)
        _lib._inject_for_tests(os.path.join(emu, "_build", "libuegan_emu.so"), os.path.join(emu, "_build", "libuegan_emu_f16.so"))
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_dataset_cache.py measures on the GPU and none is visible (there is no fallback)")
        dev = torch.device("cuda:0")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    tmp = tempfile.mkdtemp(prefix="uegan_cache_bench_")
    make_tree(tmp, args.pairs, args.height, args.width, args.seed)
    per_pass = args.pairs // args.batch * args.batch

    def loader(cache):
        return data.get_train_loader(tmp, img_size=args.img, resize_size=args.resize, batch_size=args.batch, num_workers=args.workers,
                                     generator=torch.Generator().manual_seed(7), cache=cache)

    def run_passes(ld, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            for b in ld:
                pass
        sync()
        return n * per_pass / (time.perf_counter() - t0)

    # ---- the loader alone ----
    plain = loader("none")
    run_passes(plain, 1)                                   # warm-up: worker threads, pinned slots, the tables and the code objects
    warm = loader("device")
    run_passes(warm, 2)
    warm.close()
    rates = {"uncached": [], "cached_first_pass": [], "cached_later_passes": []}
    cached = None
    for _ in range(WINDOWS):
        rates["uncached"].append(run_passes(plain, args.passes))
        if cached is not None:
            cached.close()
        cached = loader("device")
        rates["cached_first_pass"].append(run_passes(cached, 1))
        assert cached.cache_hits == 0 and cached.cache_misses == 2 * per_pass
        rates["cached_later_passes"].append(run_passes(cached, args.cached_passes))
    assert cached.cache_declined == 0
    store = {"entries": cached.cache_entries, "bytes_used": cached.cache_bytes_used}
    for k, v in rates.items():
        print("loader alone, %-20s %9.1f pairs/s  (min %.1f, max %.1f)" % (k, statistics.median(v), min(v), max(v)), flush=True)

    # ---- the transform call, old and new, on the same windows ----
    g = np.random.default_rng(args.seed + 1)
    nwin = 2 * args.batch
    images = [torch.from_numpy(g.integers(0, 256, size=(args.height, args.width, 3), dtype=np.uint8)).to(dev) for _ in range(nwin)]
    origins = [(int(g.integers(0, args.height - args.img + 1)), int(g.integers(0, args.width - args.img + 1))) for _ in range(nwin)]
    flips = [int(f) for f in g.integers(0, 4, size=nwin)]
    crops = torch.stack([im[t:t + args.img, l:l + args.img] for im, (t, l) in zip(images, origins)]).contiguous()
    out_old = torch.empty((nwin, 3, args.resize, args.resize), dtype=torch.float32, device=dev)
    out_new = torch.empty_like(out_old)
    calls = {"input_transform": lambda: data.input_transform(crops, args.resize, flips, out=out_old),
             "input_transform_windows": lambda: data.input_transform_windows(images, origins, args.img, args.resize, flips, out=out_new)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    sync()
    assert torch.equal(out_old, out_new)

    # A call's launches are short next to what the host does to issue them, so events around a plain loop would time the host.  The calls of a window
    # are queued behind ballast that keeps the device busy until the host has issued all of them: the events then bracket device work alone.  The
    # host's own time per call (descriptors, two launches) is taken in the same loop, and a window in which the ballast ran out first is flagged.
    ballast = torch.zeros((1 << 28,), dtype=torch.float32, device=dev) if dev.type == "cuda" else None

    def time_calls(fn, n):
        if dev.type != "cuda":
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            host = (time.perf_counter() - t0) / n * 1e6
            return host, host, False
        first, start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        first.record()
        for _ in range(24):
            ballast.add_(1.0)
        start.record()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        host = time.perf_counter() - t0
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / n * 1e3, host / n * 1e6, host * 1e3 >= first.elapsed_time(start)

    call_us, host_us, starved = {k: [] for k in calls}, {k: [] for k in calls}, False
    for _ in range(WINDOWS):
        for k, fn in calls.items():
            d, h, bad = time_calls(fn, args.calls)
            call_us[k].append(d)
            host_us[k].append(h)
            starved = starved or bad
    for k in calls:
        print("%-26s %8.1f us on the device per call of %d windows (min %.1f, max %.1f); %.1f us for the host to issue it"
              % (k, statistics.median(call_us[k]), nwin, min(call_us[k]), max(call_us[k]), statistics.median(host_us[k])), flush=True)
    if starved:
        print("WARNING: the host was slower than the ballast in some window: its device time includes waiting for the host", flush=True)
    del ballast
    del images, crops

    result = {"tool": "tools/bench_dataset_cache.py", "device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "emulator",
              "config": {k: getattr(args, k) for k in ("pairs", "height", "width", "img", "resize", "batch", "workers", "passes", "cached_passes", "steps",
                                                       "calls", "seed")},
              "unit": "image pairs per second; transform calls in microseconds (device: HIP events; host: wall clock of the issuing loop)", "windows_per_arm": WINDOWS, "store": store,
              "loader_alone": {k: spread(v) for k, v in rates.items()}, "transform_call_us": {k: spread(v) for k, v in call_us.items()},
              "transform_call_host_us": {k: spread(v) for k, v in host_us.items()}, "transform_call_device_waited_for_host": starved}
    if args.rehearse:
        plain.close()
        cached.close()
        print("rehearsal ok (nothing written)")
        return

    # ---- loader -> Trainer.train_step in bf16, against the same steps on resident tensors ----
    uegan_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1990)
    G = models.Generator(32, "none", "LeakyReLU", False).to(dev)
    D = models.Discriminator(32, "none", "LeakyReLU", True, "rahinge").to(dev)
    P = losses.PerceptualLoss(vgg_weights="seeded").to(dev)
    T = trainer.Trainer(G, D, P, pool_size=50)
    fetchers = {"uncached": data.InputFetcher(plain), "cached": data.InputFetcher(cached)}
    b = next(fetchers["cached"])
    raw, exp = b.img_raw.clone(), b.img_exp.clone()

    def run_steps(arm, n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            if arm == "resident":
                T.train_step(raw, exp)
            else:
                bb = next(fetchers[arm])
                T.train_step(bb.img_raw, bb.img_exp)
        sync()
        return n * args.batch / (time.perf_counter() - t0)

    arms = ("resident", "uncached", "cached")
    for arm in arms:
        run_steps(arm, 3)
    step_rates = {arm: [] for arm in arms}
    for _ in range(WINDOWS):
        for arm in arms:
            step_rates[arm].append(run_steps(arm, args.steps))
    it = T.loss_items()
    assert all(np.isfinite(v) for v in it.values()), it
    for k, v in step_rates.items():
        print("loader -> train_step, %-9s %8.1f pairs/s  (min %.1f, max %.1f)" % (k, statistics.median(v), min(v), max(v)), flush=True)
    result["train_step_bf16"] = {k: spread(v) for k, v in step_rates.items()}
    plain.close()
    cached.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
