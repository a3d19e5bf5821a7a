#!/usr/bin/env python3
"""bench.py -- UEGAN training throughput on MI355X (BASELINE.json: "train imgs/sec @512px bs=16 on 1/2/4/8 MI355X; infer ms/img").

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]     (N > 1: launched by torch.distributed.run, one rank per GPU)

A "step" is one full training iteration of the reference (trainer.py:77-119): G over both image sets, D over all five
applications, VGG19 over both fidelity-loss images, rahinge + VGG-fidelity + multiscale-L1 losses, both backward sweeps, two
Adam updates -- on a synthetic FiveK-shaped batch (16 x 3 x 512 x 512 per GPU, uniform(-1,1), seed 1990+rank) already resident
in HBM, random-init G/D of the reference architecture (conv_dim 32) and the seeded stand-in VGG19 (no network: pretrained
weights unavailable).  Prints ONE JSON line (rank 0).

Timed region: W warm-up steps, barrier + synchronize, exactly K steps with NO per-launch instrumentation, barrier +
synchronize, max over ranks; `ms_per_step` = its time / K, `value` = images/s over all ranks.  A plain run does nothing else: set-up,
warm-up, the K steps, the --dump-outputs files, the line.

--dump-outputs DIR: right after the timed region rank 0 writes what the last timed step computed, as float32 DIR/<name>.npy -- the
five losses (d_loss, g_adv, g_percep, g_idt, g_loss), the enhanced images G(raw) and G(exp) (fake_exp, real_exp_idt) and the updated
weights of G and D (g_weights, d_weights: every floating state-dict tensor flattened, in state-dict order).  An array longer than its cap
(DUMP_CAP) is replaced by a fixed sample: the elements at seeded indices, ascending (< 64 MB in all).  The inputs, the initial weights
and the image pool's draws are seeded, so two builds run with the same arguments can be compared output for output.

--full adds, AFTER the timed region (and after the dump): the same K steps without the per-step loss readback (`no_readback`), and,
on rank 0:
  roofline     -- a second, instrumented pass (every convolution launch bracketed by HIP events on the launch stream):
                  * the dominant kernel (the MFMA implicit-GEMM instantiation with the most time): algorithmic FLOP/s vs dense
                    bf16 MFMA peak; `traffic` = HBM bytes per launch from separate rocprofv3 --pmc passes (profiles/pmc_traffic.json)
                  * `hbm_kernel`: the HBM-bound streaming-convolution instantiation with the most time: algorithmic bytes/s vs 8 TB/s
                  * `step`: the WHOLE step against both rooflines -- algorithmic FLOPs and bytes per step (SURVEY.md 8d:
                    1.106 TFLOP and 4.3 GB bf16 per 512^2 image) over the un-instrumented ms_per_step
  infer        -- single-image generator inference (tester.py:58-67) as one hipGraph replay: ms/img, its roofline fractions
                  (67.7 GFLOP, 0.40 GB bf16 per 512^2 image) and the CPU oracle's time for the same image
  cpu_baseline -- the CPU oracle (plain PyTorch-CPU restatement, kind "port") train step on this box's host cores on a bounded
                  sample (batch 2 @512^2, 16 threads: 1 warm-up + 2 timed steps, the faster one), N=1 only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# dense peaks from /opt/skills/guides/MI355X_MICROARCH.md
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3}
PEAK_HBM_GBS = 8000.0
# algorithmic work per 512 x 512 image, scaled by (S/512)^2: train step / inference
STEP_TFLOP_PER_IMG, STEP_GB_PER_IMG_BF16 = 1.1056, 4.3
INFER_GFLOP_PER_IMG, INFER_GB_PER_IMG_BF16 = 67.7, 0.40


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16, help="images per GPU (BASELINE config: 16)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", choices=["bf16", "f16", "f32"], default="bf16",
                    help="storage dtype of activations / packed weights: bf16 (the configuration BASELINE.json names), f16 (same bytes and MFMA "
                         "rate, 11 significant bits, loss scale 2^14: libuegan_hip_f16.so), f32 (parity mode)")
    ap.add_argument("--precise", action="store_true", help="uegan_amd.set_precise(True): the generator's full-resolution chain on hi + lo pairs (with --dtype f16)")
    ap.add_argument("--no-fuse-epilogues", action="store_true", help="A/B: y4 * x1 and the residual + clamp as separate kernels instead of in dec4's / dec5.1's epilogue")
    ap.add_argument("--conv-dim", type=int, default=32)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's losses, enhanced images and updated weights "
                                                                        "as float32 DIR/<name>.npy (rank 0; large arrays as a fixed seeded sample)")
    ap.add_argument("--full", action="store_true", help="after the headline: the no-readback rerun, the instrumented roofline pass, inference timing, the "
                                                        "fp32 / fp16 / fp16-precise legs, the CPU baseline and the recorded profiles (the --no-* options "
                                                        "below drop single parts of it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true", help="skip the instrumented pass (no roofline object)")
    ap.add_argument("--no-infer", dest="infer", action="store_false", help="skip the single-image G inference timing (tester.py:58-67)")
    ap.add_argument("--per-line", action="store_true", help="one module call per reference line instead of the batched passes (A/B)")
    ap.add_argument("--early-sn", action="store_true", help="A/B: the D update's spectral-norm rounds at the start of the step on the second stream instead of in "
                                                           "front of the discriminator pass (Trainer(early_sn=True))")
    ap.add_argument("--no-free-run", action="store_true", help="skip the second K steps without the per-step loss readback (profiling runs: the process then "
                                                              "executes exactly warmup + steps training steps)")
    ap.add_argument("--no-fp32", dest="fp32", action="store_false", help="skip the fp32 parity-mode and fp16-storage timings (N=1, bf16 runs only)")
    ap.add_argument("--fp32-steps", type=int, default=5)
    ap.add_argument("--one-stream", action="store_true", help="no second stream for the D-independent generator losses (kernel-time accounting "
                                                              "under rocprofv3: overlapping kernels share the CUs and each one runs longer)")
    ap.add_argument("--tune", default="", help="A/B runs: knob=value[,knob=value] passed to uegan_set_tuning (include/uegan_hip.h) before the first step")
    ap.add_argument("--comm-budget-ms", type=float, default=1.0, help="N > 1: all-reduce time per step that nothing on the training stream covered above which the "
                                                                       "line carries comm.exposed_over_budget and a warning goes to stderr")
    ap.add_argument("--strict-comm", action="store_true", help="N > 1: exit with code 3 (after printing the line) when the exposed all-reduce time is over the budget")
    ap.set_defaults(infer=True, fp32=True)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return ""


def cpu_baseline(args):
    """Oracle (port) train step on the host cores: bounded sample of the same workload."""
    import random
    from oracle import uegan_oracle as O
    # measured on the MI355X host (EPYC 9575F, 256 hw threads): 8 thr 6.0 s/step, 16 thr 5.3, 32 thr 5.6, 64 thr 9.3,
    # 256 thr 291 s (oneDNN oversubscription) -> use 16 worker threads
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cores = torch.get_num_threads()
    B, S, cd = args.cpu_batch, args.size, args.conv_dim
    PG = O.init_params(O.generator_param_shapes(cd), 41, "default")
    PD = O.init_params(O.discriminator_param_shapes(cd), 42, "default")
    V = O.make_vgg_weights(seed=1234, width_div=1)
    St = O.TrainState(PG, PD, V, pool_size=50, rng=random.Random(1990))
    g = torch.Generator().manual_seed(1990)
    times = []
    for it in range(3):
        raw = torch.rand(B, 3, S, S, generator=g) * 2 - 1
        exp = torch.rand(B, 3, S, S, generator=g) * 2 - 1
        t = time.time()
        O.train_step(St, raw, exp)
        times.append(time.time() - t)
    t_best = min(times[1:])
    # single-image inference (tester.py:58-67) on the same cores
    x = torch.rand(1, 3, S, S, generator=g) * 2 - 1
    ti = []
    with torch.no_grad():
        for it in range(6):
            t = time.time()
            O.generator_forward(PG, x)
            ti.append(time.time() - t)
    return {"value": round(B / t_best, 4), "unit": "imgs/sec", "cores": cores, "kind": "port",
            "sample": "oracle/uegan_oracle.py train_step (plain PyTorch-CPU fp32), batch %d @%dx%d, 1 warm-up + 2 timed steps, the faster "
                      "one: %.2f s/step (the other: %.2f)" % (B, S, S, t_best, max(times[1:])),
            "infer_ms_per_img": round(sorted(ti[1:])[len(ti[1:]) // 2] * 1e3, 1),
            "infer_sample": "oracle generator_forward, 1 x 3 x %d x %d, 1 warm-up + 5 runs, median" % (S, S),
            "cpu_model": _cpu_model()}


def roofline_from_profile(rows, args, ms_per_step, world):
    """rows: per kernel instantiation {name, launches, total_ms, total_flops, total_bytes} of the instrumented pass"""
    S, B = args.size, args.batch
    scale = (S / 512.0) ** 2
    es = 2.0 if args.dtype == "f32" else 1.0
    peak = PEAK_TFLOPS[args.dtype]
    step_tflop = STEP_TFLOP_PER_IMG * scale * B
    step_gb = STEP_GB_PER_IMG_BF16 * es * scale * B
    step = {"algorithmic_tflop": round(step_tflop, 2), "algorithmic_gb": round(step_gb, 1), "ms_per_step": round(ms_per_step, 3),
            "achieved_tflops": round(step_tflop / (ms_per_step * 1e-3), 1), "mfma_frac": round(step_tflop / (ms_per_step * 1e-3) / peak, 4),
            "achieved_gbs": round(step_gb / (ms_per_step * 1e-3), 1), "hbm_frac": round(step_gb / (ms_per_step * 1e-3) / PEAK_HBM_GBS, 4)}
    if not rows:
        return {"bound": "mfma", "achieved": None, "peak": peak, "unit": "TFLOP/s", "frac": None, "traffic": None, "step": step}
    nst = args.prof_steps
    mf = [r for r in rows if "conv_stream" not in r["name"]]
    hb = [r for r in rows if "conv_stream" in r["name"]]
    mf.sort(key=lambda r: -r["total_ms"])
    hb.sort(key=lambda r: -r["total_ms"])
    top = mf[0]
    ach = top["total_flops"] / (top["total_ms"] * 1e-3) / 1e12
    roof = {"bound": "mfma", "kernel": top["name"], "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "traffic": None, "launches_per_step": top["launches"] / nst, "avg_launch_ms": round(top["total_ms"] / top["launches"], 5),
            "gflop_per_launch": round(top["total_flops"] / top["launches"] / 1e9, 3),
            "algorithmic_bytes_per_launch": round(top["total_bytes"] / top["launches"]),
            "kernel_ms_per_step": round(top["total_ms"] / nst, 3),
            "all_conv_kernels_ms_per_step": round(sum(r["total_ms"] for r in rows) / nst, 3),
            "all_conv_kernels_tflops": round(sum(r["total_flops"] for r in rows) / (sum(r["total_ms"] for r in rows) * 1e-3) / 1e12, 2),
            "top5": [{"kernel": r["name"], "ms_per_step": round(r["total_ms"] / nst, 2),
                      "tflops": round(r["total_flops"] / (r["total_ms"] * 1e-3) / 1e12, 1),
                      "gbs": round(r["total_bytes"] / (r["total_ms"] * 1e-3) / 1e9, 0)} for r in sorted(rows, key=lambda r: -r["total_ms"])[:5]],
            "measured": "instrumented pass of %d steps after the timed region (HIP events around every convolution launch; single stream, "
                        "i.e. without the timed region's overlap of the VGG passes with the discriminator update)" % nst}
    try:
        # HBM traffic of that kernel comes from separate rocprofv3 --pmc passes (PMC collection cannot run inside this process)
        pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get(roof["kernel"])
        if pmc:
            roof["traffic"] = pmc["traffic_bytes"]
            roof["traffic_unit"] = "bytes/launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, %s)" % pmc.get("round", "")
    except (OSError, ValueError):
        pass
    if hb:
        h = hb[0]
        gbs = h["total_bytes"] / (h["total_ms"] * 1e-3) / 1e9
        roof["hbm_kernel"] = {"bound": "hbm", "kernel": h["name"], "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": round(gbs / PEAK_HBM_GBS, 4), "launches_per_step": h["launches"] / nst,
                              "avg_launch_ms": round(h["total_ms"] / h["launches"], 5),
                              "algorithmic_bytes_per_launch": round(h["total_bytes"] / h["launches"]),
                              "kernel_ms_per_step": round(h["total_ms"] / nst, 3)}
    roof["step"] = step
    return roof


# --dump-outputs: elements kept per array (float32): 2 x 4 MB of images, up to 2 x 21 MB of weights (G: 4.16 M, D: 4.65 M at conv_dim 32)
DUMP_CAP = {"image": 1 << 20, "weights": 5 << 20}
DUMP_SEED = 20240


def dump_outputs(dirname, T):
    """the last timed step's results as a caller of Trainer.train_step receives them (see the module docstring)"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)

    def flat_state(m):
        return torch.cat([t.detach().reshape(-1).float() for t in m.state_dict().values() if t.is_floating_point()])

    arrays = [(k, T.losses[k].reshape(1), None) for k in T.LOSS_KEYS]
    arrays += [("fake_exp", T.fake_exp, "image"), ("real_exp_idt", T.real_exp_idt, "image"),
               ("g_weights", flat_state(T.G), "weights"), ("d_weights", flat_state(T.D), "weights")]
    for name, t, kind in arrays:
        t = t.detach().reshape(-1)
        if kind is not None and t.numel() > DUMP_CAP[kind]:
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(DUMP_SEED))[:DUMP_CAP[kind]].sort().values
            t = t[idx.to(t.device)]
        np.save(os.path.join(dirname, name + ".npy"), t.float().cpu().numpy())


def main():
    args = parse()
    args.prof_steps = 2
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus %d needs `python -m torch.distributed.run --nproc-per-node %d bench.py ...`" % (args.gpus, args.gpus))
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # (backend "nccl" IS RCCL on ROCm) the job the driver asked for is the job that runs
        assert dist.get_world_size() == args.gpus and dist.get_backend() == "nccl", (dist.get_world_size(), dist.get_backend(), args.gpus)

    import random
    import uegan_amd
    from uegan_amd import _lib, losses, models, trainer

    TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
    uegan_amd.set_compute_dtype(TDT[args.dtype])
    uegan_amd.set_precise(args.precise)
    uegan_amd.ops.fuse_epilogues[0] = not args.no_fuse_epilogues
    lib = _lib.load()
    for kv in filter(None, args.tune.split(",")):
        _lib.check(lib.uegan_set_tuning(int(kv.split("=")[0]), int(kv.split("=")[1]), None))
    torch.manual_seed(1990)            # same init on every rank (also broadcast from rank 0 by the Trainer)
    G = models.Generator(args.conv_dim, "none", "LeakyReLU", False).to(dev)
    D = models.Discriminator(args.conv_dim, "none", "LeakyReLU", True, "rahinge").to(dev)
    P = losses.PerceptualLoss(vgg_weights="seeded").to(dev)      # explicit opt-in: no network, pretrained weights unavailable
    T = trainer.Trainer(G, D, P, pool_size=50, rng=random.Random(1990 + rank), fused_passes=not args.per_line, overlap=not args.one_stream, early_sn=args.early_sn)

    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(1990 + rank)
    nb = 2                                   # two resident synthetic batches, alternated
    raws = [(torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev) for _ in range(nb)]
    exps = [(torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev) for _ in range(nb)]

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        T.train_step(raws[i % nb], exps[i % nb])
    T.sync()
    sync()
    if world > 1:
        T.g_bucket.timing, T.d_bucket.timing = [], []       # event pairs around the all-reduce waits (no host sync, two events per wait)
    # The timed loop is the loop a user runs: every step ends with the single readback of its five logged losses (the reference
    # calls .item() five times per step, trainer.py:98-119), so the host never runs more than one step ahead of the device.
    calls0, host_issue = _lib.n_calls, 0.0
    t0 = time.perf_counter()
    for i in range(args.steps):
        th = time.perf_counter()
        T.train_step(raws[i % nb], exps[i % nb])
        host_issue += time.perf_counter() - th
        items = T.loss_items()
    T.sync()                                 # data parallel: the last step's deferred generator update belongs to the timed region
    sync()
    dt = time.perf_counter() - t0
    abi_calls_per_step = (_lib.n_calls - calls0) / float(args.steps)
    host_issue_ms = host_issue / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, T)
    # --full: the same K steps WITHOUT the per-step readback (the host free to run ahead; what rounds 1-4 reported as `value`), rank-local, after the timed region
    dt_free = dt
    if args.full and not args.no_free_run:
        t1 = time.perf_counter()
        for i in range(args.steps):
            T.train_step(raws[i % nb], exps[i % nb])
        T.sync()
        sync()
        dt_free = time.perf_counter() - t1
    comm = None
    if world > 1:
        comm = {"g_allreduce_exposed_ms_per_step": round(T.g_bucket.exposed_wait_ms() / args.steps, 4),
                "d_allreduce_exposed_ms_per_step": round(T.d_bucket.exposed_wait_ms() / args.steps, 4),
                "payload_mb_per_step": round((T.g_bucket.flat.numel() + T.d_bucket.flat.numel()) * 4 / 1e6, 2),
                "note": "stream time between an event before and one after the waits of GradBucket.finish(): the part of the RCCL "
                        "all-reduces that no kernel of the training stream covered (rank 0)"}
        exposed = comm["g_allreduce_exposed_ms_per_step"] + comm["d_allreduce_exposed_ms_per_step"]
        comm["exposed_ms_per_step"] = round(exposed, 4)
        comm["exposed_over_budget"] = bool(exposed > args.comm_budget_ms)
        # what RCCL itself reports: the communicator's size and version, and the box's link topology (rank 0) -- so that the first run on a multi-GPU
        # node says by itself whether the ring went over xGMI
        comm["rccl"] = {"ranks": dist.get_world_size(), "backend": dist.get_backend(), "version": ".".join(str(v) for v in torch.cuda.nccl.version()),
                        "devices": torch.cuda.device_count()}
        if rank == 0 and args.full:
            try:
                import subprocess
                topo = subprocess.run(["rocm-smi", "--showtopotype"], capture_output=True, text=True, timeout=20).stdout
                comm["rccl"]["link_types"] = [ln.strip() for ln in topo.splitlines() if ln.strip().startswith("GPU")][:9]
            except Exception as e:                                  # (rocm-smi missing or slow: the line is informational)
                comm["rccl"]["link_types"] = "unavailable: %s" % type(e).__name__
        T.g_bucket.timing = T.d_bucket.timing = None
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    host_per_rank = [[round(host_issue_ms, 3), round(abi_calls_per_step, 1)]]
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        # every rank's host-side issue time and C-ABI calls per step: with 8 ranks per host the Python + ctypes launch path is the first thing
        # that can become the limiter -- rank 0 prints all of them
        mine = torch.tensor([host_issue_ms, abi_calls_per_step], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        host_per_rank = [[round(float(t[0]), 3), round(float(t[1]), 1)] for t in allr]
    dt = float(tmax.item())
    ms_per_step = dt / args.steps * 1e3

    # ---- instrumented pass (every rank runs it so that the collectives stay matched; only rank 0 reports)
    rows = []
    if args.full and not args.no_profile:
        # (one stream for this pass: with the VGG passes beside the discriminator update -- Trainer.overlap, the timed region's setting --
        # an event pair around a launch would also time the other stream's kernels sharing the chip)
        overlap_was, T.overlap = T.overlap, False
        _lib.check(lib.uegan_profile_begin(1200 * args.prof_steps + 64))
        for i in range(args.prof_steps):
            T.train_step(raws[i % nb], exps[i % nb])
        sync()
        ents = (_lib.ProfileEntry * 128)()
        n = ctypes.c_int(0)
        _lib.check(lib.uegan_profile_end(ents, 128, ctypes.byref(n)))
        rows = [dict(name=ents[i].name.decode(), launches=int(ents[i].launches), total_ms=float(ents[i].total_ms),
                     total_flops=float(ents[i].total_flops), total_bytes=float(ents[i].total_bytes)) for i in range(n.value)]
        T.overlap = overlap_was

    infer = None
    if args.full and args.infer and rank == 0:
        from uegan_amd import tester
        x1 = raws[0][:1].contiguous()
        for _ in range(3):
            tester.enhance(G, x1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(20):
            tester.enhance(G, x1)
        torch.cuda.synchronize()
        eager_ms = (time.perf_counter() - t1) / 20 * 1e3
        GG = tester.GraphedGenerator(G, x1.shape)
        for _ in range(3):
            GG(x1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(50):
            GG(x1)
        torch.cuda.synchronize()
        graph_ms = (time.perf_counter() - t1) / 50 * 1e3
        scale = (S / 512.0) ** 2
        es = 2.0 if args.dtype == "f32" else 1.0
        # throughput form (tester.run_test works in batches of 8): one graph replay per batch
        xb = torch.cat([raws[0][:8], raws[1][:8]])[:8].contiguous() if B < 8 else raws[0][:8].contiguous()
        GB = tester.GraphedGenerator(G, xb.shape)
        for _ in range(3):
            GB(xb)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(20):
            GB(xb)
        torch.cuda.synchronize()
        b8_ms = (time.perf_counter() - t1) / 20 * 1e3 / xb.shape[0]
        infer = {"ms_per_img": round(graph_ms, 4), "mode": "hipGraph replay of the eval-mode forward (tester.GraphedGenerator), batch 1",
                 "eager_ms_per_img": round(eager_ms, 4),
                 "mfma_frac": round(INFER_GFLOP_PER_IMG * scale / 1e3 / (graph_ms * 1e-3) / PEAK_TFLOPS[args.dtype], 4),
                 "hbm_frac": round(INFER_GB_PER_IMG_BF16 * es * scale / (graph_ms * 1e-3) / PEAK_HBM_GBS, 4),
                 "algorithmic_gflop": round(INFER_GFLOP_PER_IMG * scale, 1), "algorithmic_gb": round(INFER_GB_PER_IMG_BF16 * es * scale, 3),
                 "batch8": {"ms_per_img": round(b8_ms, 4), "imgs_per_sec": round(1e3 / b8_ms, 1), "batch": int(xb.shape[0]),
                            "mfma_frac": round(INFER_GFLOP_PER_IMG * scale / 1e3 / (b8_ms * 1e-3) / PEAK_TFLOPS[args.dtype], 4),
                            "hbm_frac": round(INFER_GB_PER_IMG_BF16 * es * scale / (b8_ms * 1e-3) / PEAK_HBM_GBS, 4)}}

    # ---- the parity mode (fp32 storage: the mode that meets north_star's 1e-3 gate against the reference fixtures), timed the same way
    fp32 = fp16 = fp16p = None
    if args.full and world == 1 and args.fp32 and args.dtype == "bf16":
        del T
        uegan_amd.set_compute_dtype(torch.float32)
        torch.manual_seed(1990)
        G32 = models.Generator(args.conv_dim, "none", "LeakyReLU", False).to(dev)
        D32 = models.Discriminator(args.conv_dim, "none", "LeakyReLU", True, "rahinge").to(dev)
        T32 = trainer.Trainer(G32, D32, losses.PerceptualLoss(vgg_weights="seeded").to(dev), pool_size=50, rng=random.Random(1990),
                              fused_passes=not args.per_line)
        for i in range(2):
            T32.train_step(raws[i % nb], exps[i % nb])
        sync()
        t1 = time.perf_counter()
        for i in range(args.fp32_steps):
            T32.train_step(raws[i % nb], exps[i % nb])
        sync()
        d32 = time.perf_counter() - t1
        step_tflop = STEP_TFLOP_PER_IMG * (S / 512.0) ** 2 * B
        fp32 = {"value": round(B * args.fp32_steps / d32, 3), "unit": "imgs/sec", "steps": args.fp32_steps, "warmup": 2,
                "ms_per_step": round(d32 / args.fp32_steps * 1e3, 3), "dtype": "f32",
                "mfma_frac": round(step_tflop / (d32 / args.fp32_steps) / PEAK_TFLOPS["f32"], 4),
                "note": "same workload with fp32 activation storage and exact fp32 MFMA (v_mfma_f32_16x16x4_f32): the configuration the "
                        "1e-3 parity tests against the reference fixtures run in"}
        del T32, G32, D32
        # ---- the same bytes as fp16: libuegan_hip_f16.so (the same kernel sources with fp16 as the 16-bit storage format), loss scale 2^14.
        # 11 instead of 8 significant bits at the same MFMA rate: the 16-bit mode that IS inside north_star's tolerance
        for prec in (False, True):
            # (second leg: the `precise` mode of the fp16 build -- the generator's full-resolution chain on hi + lo pairs, uegan_conv2d_fwd_ex: the 16-bit-rate
            # mode whose enhanced pixels are inside north_star's 1e-3)
            uegan_amd.set_compute_dtype(torch.float16)
            uegan_amd.set_precise(prec)
            for kv in filter(None, args.tune.split(",")):      # (the fp16-format build is its own library: the knobs go to it too)
                _lib.check(_lib.load().uegan_set_tuning(int(kv.split("=")[0]), int(kv.split("=")[1]), None))
            torch.manual_seed(1990)
            G16 = models.Generator(args.conv_dim, "none", "LeakyReLU", False).to(dev)
            D16 = models.Discriminator(args.conv_dim, "none", "LeakyReLU", True, "rahinge").to(dev)
            T16 = trainer.Trainer(G16, D16, losses.PerceptualLoss(vgg_weights="seeded").to(dev), pool_size=50, rng=random.Random(1990),
                                  fused_passes=not args.per_line, overlap=not args.one_stream, early_sn=args.early_sn)
            for i in range(args.warmup):
                T16.train_step(raws[i % nb], exps[i % nb])
            sync()
            t1 = time.perf_counter()
            for i in range(args.steps):
                T16.train_step(raws[i % nb], exps[i % nb])
                it16 = T16.loss_items()
            sync()
            d16 = time.perf_counter() - t1
            fp16 = {"value": round(B * args.steps / d16, 3), "unit": "imgs/sec", "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step": round(d16 / args.steps * 1e3, 3), "dtype": "f16", "loss_scale": T16.loss_scale,
                    "mfma_frac": round(step_tflop / (d16 / args.steps) / PEAK_TFLOPS["f16"], 4),
                    "roofline_step": {"algorithmic_tflop": round(step_tflop, 2), "algorithmic_gb": round(STEP_GB_PER_IMG_BF16 * (S / 512.0) ** 2 * B, 1),
                                      "mfma_frac": round(step_tflop / (d16 / args.steps) / PEAK_TFLOPS["f16"], 4),
                                      "hbm_frac": round(STEP_GB_PER_IMG_BF16 * (S / 512.0) ** 2 * B / (d16 / args.steps) / PEAK_HBM_GBS, 4)},
                    "losses_last_step": {k: round(v, 6) for k, v in it16.items()},
                    "note": "same workload, same bytes, fp16 instead of bf16 storage (the kernel library rebuilt with -DUEGAN_HALF_FP16; weight "
                            "gradients, statistics, losses and master weights fp32 as in every mode): measured against the fp32 path one full "
                            "16x3x512^2 step deviates by <= 1e-4 on the five losses and 2.2e-3 on the enhanced pixels (bf16: 2.2e-3 / 1.5e-2), "
                            "inference 66.1 dB (bf16 57.1) -- profiles/*_bf16_deviation.json"}
            if args.infer:
                from uegan_amd import tester
                x1 = raws[0][:1].contiguous()
                GG16 = tester.GraphedGenerator(G16, x1.shape)
                for _ in range(3):
                    GG16(x1)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(50):
                    GG16(x1)
                torch.cuda.synchronize()
                fp16["infer_ms_per_img"] = round((time.perf_counter() - t1) / 50 * 1e3, 4)
                del GG16
            del T16, G16, D16
            if prec:
                fp16["precise"] = True
                fp16["note"] = "the fp16 leg with uegan_amd.set_precise(True): image, x1, ga1, y4 * x1 and dec5.0's result as hi + lo pairs, thin-layer weights as pairs"
                fp16p, fp16 = fp16, fp16_plain
            else:
                fp16_plain = fp16
        uegan_amd.set_precise(False)
        uegan_amd.set_compute_dtype(torch.bfloat16)

    def _profile_json(name):
        try:
            return json.load(open(os.path.join(ROOT, "profiles", name)))
        except (OSError, ValueError):
            return None

    over_budget = False
    if rank == 0:
        out = {
            "metric": "train imgs/sec @512px bs=16 on 1/2/4/8 MI355X; infer ms/img",
            "value": round(world * B * args.steps / dt, 3), "unit": "imgs/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "FiveK-shaped %dx%d batch=%d/GPU, full G/D/VGG train step (trainer.py:77-119), conv_dim=%d, "
                                   "seeded stand-in VGG19" % (S, S, B, args.conv_dim),
                       "global_batch": world * B, "parallelism": "dp%d" % world, "pool_size": 50,
                       "collective": ("RCCL (torch.distributed nccl backend), %d ranks" % dist.get_world_size()) if world > 1 else "none (1 rank)",
                       "passes": "per reference line" if args.per_line else "batched (fused.py)"},
            "losses_last_step": {k: round(v, 6) for k, v in items.items()},
            **({"tune": args.tune} if args.tune else {}),
            "loss_readback": "one 5-float device-to-host copy per step inside the timed loop (Trainer.loss_items)",
            "host": {"issue_ms_per_step": round(host_issue_ms, 3), "abi_calls_per_step": round(abi_calls_per_step, 1),
                     "per_rank": host_per_rank,
                     "note": "rank 0: wall time inside train_step() (Python + ctypes launch path; the device runs behind it) and C-ABI calls per "
                             "step (one call = one to four kernel launches)"},
        }
        if args.full:
            out["no_readback"] = {"ms_per_step": round(dt_free / args.steps * 1e3, 3), "value": round(world * B * args.steps / dt_free, 3),
                                  "note": "the same K steps with the host free to run ahead (no per-step loss readback; rank 0's clock)"}
        if args.full and not args.no_profile:
            out["roofline"] = roofline_from_profile(rows, args, ms_per_step, world)
            st = (_profile_json("pmc_traffic.json") or {}).get("step")
            if st and args.dtype == "bf16" and (B, S) == (16, 512):
                # whole-step HBM traffic from separate rocprofv3 --pmc passes over this same step (tools/gpu_step_traffic.sh)
                out["roofline"]["step"]["traffic_bytes"] = st["traffic_bytes"]
                out["roofline"]["step"]["traffic_over_algorithmic"] = round(st["traffic_bytes"] / (out["roofline"]["step"]["algorithmic_gb"] * 1e9), 3)
                out["roofline"]["step"]["traffic_source"] = st.get("source", "")
        if comm is not None:
            out["comm"] = comm
        gaps_name = "r06_step_gaps.json" if _profile_json("r06_step_gaps.json") else "r05_step_gaps.json"
        gaps = _profile_json(gaps_name) or _profile_json("r04_step_gaps.json")
        if gaps and args.full and not args.no_profile and args.dtype == "bf16" and (B, S) == (16, 512):
            # GPU idle time of the step (rocprofv3 kernel trace of this command, tools/gpu_gaps.sh): wall - union of kernel intervals
            m = gaps["mean"]
            out["roofline"]["step"]["gpu_idle"] = {"idle_ms_per_step": m["idle_ms"], "busy_ms_per_step": m["busy_ms"], "wall_ms_per_step": m["wall_ms"],
                                                   "launches_per_step": m["launches"], "kernel_sum_ms_per_step": m["kernel_sum_ms"],
                                                   "source": "profiles/" + gaps_name + " (tools/gap_analysis.py over a rocprofv3 --kernel-trace of "
                                                             "bench.py --steps 6 --warmup 2, two streams)"}
        if fp32 is not None:
            out["fp32"] = fp32
        if fp16 is not None:
            out["fp16"] = fp16
        if fp16p is not None:
            out["fp16_precise"] = fp16p
        dev_rec = (_profile_json("r06_bf16_deviation.json") or _profile_json("r05_bf16_deviation.json") or _profile_json("r04_bf16_deviation.json") or _profile_json("r03_bf16_deviation.json")
                   or _profile_json("r02_bf16_deviation.json"))
        if dev_rec and args.full and args.dtype == "bf16":
            out["bf16_deviation"] = {"source": "tests/test_parity_full.py on an MI355X (profiles/*_bf16_deviation.json): bf16 storage against the fp32 "
                                               "path / the fp32 reference fixtures", "records": dev_rec}
        vo = (dev_rec or {}).get("full_step_16x512_vs_oracle")
        if vo and args.full and args.dtype == "bf16":
            # which legs of this line are inside north_star's tolerance (1e-3 relative: the five losses; the enhanced pixels) -- one full 16 x 512^2 step
            # of each storage mode against the CPU ORACLE (tests/test_oracle_at_size.py::test_train_step_full_size_16x512_against_oracle)
            def leg(m):
                r = vo.get(m)
                if not r:
                    return None
                worst_loss = max(r[k] for k in ("d_loss_rel", "g_adv_rel", "g_percep_rel", "g_idt_rel", "g_loss_rel"))
                return {"worst_loss_rel": worst_loss, "losses_inside_1e-3": worst_loss <= 1e-3, "pixels_max_abs": r["fake_abs"],
                        "pixels_elementwise_rel_floor_1e-2": r["fake_elem_rel_floor1e-2"], "pixels_inside_1e-3": r["fake_elem_rel_floor1e-2"] <= 1e-3}
            def with_rate(l, rec):
                if l is not None and rec is not None:
                    l["imgs_per_sec_this_run"] = rec["value"]
                    l["pixels_max_norm_inside_1e-3"] = l["pixels_max_abs"] <= 1e-3      # (pixels in [-1, 1]: max abs = max-norm relative)
                return l
            out["tolerance_legs"] = {"value (bf16 storage)": with_rate(leg("bf16"), {"value": out["value"]}), "fp16 (fp16 storage)": with_rate(leg("f16"), fp16),
                                     "fp16_precise (fp16 storage, set_precise: hi + lo pairs)": with_rate(leg("f16p"), fp16p),
                                     "fp32 (parity mode)": with_rate(leg("f32"), fp32),
                                     "note": "against the fp32 CPU oracle at the benchmark's own size (tests/test_oracle_at_size.py, profiles/r06_bf16_deviation.json): "
                                             "fp32 is inside north_star's 1e-3 on losses and pixels (element-wise); the PRECISE fp16 mode on the losses and on the pixels "
                                             "in max-norm (7.8e-4 on this configuration; weight-dependent tail, 1.02e-3 with another initialisation: DESIGN.md section 4), at 16-bit rate; plain fp16 on the losses only; bf16 (the dtype BASELINE.json names, the headline) on neither"}
        if infer is not None:
            out["infer_ms_per_img"] = infer["ms_per_img"]
            out["infer"] = infer
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args)
        print(json.dumps(out), flush=True)
        if comm is not None and comm["exposed_over_budget"]:
            sys.stderr.write("bench.py: EXPOSED ALL-REDUCE %.3f ms/step > %.3f ms budget (G %.3f + D %.3f): the RCCL reductions are not hidden behind the backward "
                             "sweeps -- check comm.rccl.link_types (xGMI?) and the chunk order (trainer.GradBucket.launch_log)\n"
                             % (comm["exposed_ms_per_step"], args.comm_budget_ms, comm["g_allreduce_exposed_ms_per_step"], comm["d_allreduce_exposed_ms_per_step"]))
            over_budget = True
    if world > 1:
        dist.barrier()              # (rank 0 is still timing the inference forms while the others are done: leave together)
        dist.destroy_process_group()
    if over_budget and args.strict_comm:
        sys.exit(3)


if __name__ == "__main__":
    main()
