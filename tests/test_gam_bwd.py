"""One-pass backward of the full-resolution attention modules (uegan_gam_bwd, csrc/gam_bwd.hip, UEGAN_TUNE_GAM_BWD) against an fp64 reference
computed from the same rounded inputs, with dz rounded to the storage dtype in the reference too.

Tolerance: on every case the separate passes the kernel replaces (uegan_instnorm_bwd, the 1x1 data gradient, the 1x1 weight gradient,
uegan_act_bwd3) run on the same inputs and their maximum error against the same reference is measured; the one-pass kernel must stay within
TWICE that error, for dz_enc and for dW separately.  Both errors are fp32 summation-order noise plus single-ulp roundings of the storage format.
Observed (max abs error against the reference: one pass / separate passes; GPU, the emulator within a few per cent):
    bf16  dz_enc 1.56e-2 / 1.56e-2 at max |ref| 5.7 (33 x 50, C = 32, two addends): one unit in the last place of the stored value, on both routes
    f16   dz_enc 2.00e-3 / 2.00e-3 at max |ref| 6.5
    (the one pass rounds W^T dz to the storage format before it adds the other gradients, in act_bwd_kernel's order: it stores the separate passes' value,
    and on the GPU the two dz_enc tensors are bit-equal on every case, as on 3 x 512 x 512 x 32 and 3 x 256 x 256 x 64 tensors with the default grid)
    dW where an element of dz rounds differently from the fp64 reference's (one ulp of dz, shared by both routes): bf16 5.49e-4 / 5.49e-4, f16 1.64e-4 / 1.64e-4
    at max |ref| 15; where none does, fp32 summation noise: 1.4e-6 / 1.3e-6 (33 x 50, max |ref| 13.5), 3.4e-7 / 4.5e-7 (5 x 13, max |ref| 3.3)
The emulator's MFMA adds its 32 products one after the other; with one running accumulator per wave that chain made the one pass's dW noise 2.2 times the
separate passes' on one case (8.6e-7 / 3.9e-7, f16, 3 x 65 pixels, C = 32, accumulate) -- the kernel now sums every 32-pixel k-step from zero and adds the k-steps
pairwise, which is also the better order on the hardware."""
import ctypes

import pytest
import torch

from helpers import BACKENDS, use_backend
from uegan_amd import _lib, models, ops

GAM_BWD = 13                     # UEGAN_TUNE_GAM_BWD (include/uegan_hip.h)
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
SENTINEL = -7.25


def _set_knob(value):
    """the knob on the library of the current compute dtype; returns the previous value"""
    prev = ctypes.c_int(0)
    _lib.check(_lib.load().uegan_set_tuning(GAM_BWD, int(value), ctypes.byref(prev)))
    return prev.value


def _inputs(seed, dtype, dev, B, H, W, C, n_add):
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(B, H, W, C, generator=g).to(dtype) for k in ("g", "y", "x", "add1", "add2")}
    t["x"].view(-1)[::7] = 0                                   # LeakyReLU'(0) = 0.2: some activations exactly on the kink
    t["g"] = (t["g"].float() * 0.05 + 0.01).to(dtype)          # (gradients: small, with a mean)
    adds = [t["add1"], t["add2"]][:n_add]
    rstd = torch.rand(B * C, generator=g) * 1.5 + 0.5
    weight = torch.randn(C, 2 * C, 1, 1, generator=g) * 0.2
    bucket = torch.randn(C, 2 * C, 1, 1, generator=g)
    return {"g": t["g"].to(dev), "y": t["y"].to(dev), "x": t["x"].to(dev), "adds": [a.to(dev) for a in adds], "rstd": rstd.to(dev),
            "weight": weight.to(dev), "bucket": bucket.to(dev)}


def _reference(I, dtype, act, acc):
    """fp64 from the rounded inputs; dz rounded to the storage dtype, as both routes store / multiply it"""
    g, y, x = (I[k].cpu().double() for k in ("g", "y", "x"))
    B, H, W, C = g.shape
    rstd = I["rstd"].cpu().double().view(B, 1, 1, C)
    m0, m1 = g.mean(dim=(1, 2), keepdim=True), (g * y).mean(dim=(1, 2), keepdim=True)
    dz = (rstd * (g - m0 - y * m1)).to(dtype).double()
    Wr = I["weight"].cpu()[:, :C, 0, 0].to(dtype).double()     # [co][ci], as packed
    dx = dz.view(-1, C) @ Wr
    for a in I["adds"]:
        dx = dx + a.cpu().double().view(-1, C)
    if act == ops.ACT_LRELU:
        dx = dx * torch.where(x.view(-1, C) > 0, 1.0, 0.2)
    dw = dz.view(-1, C).t() @ x.view(-1, C)                    # [co][ci]
    if acc:
        dw = dw + I["bucket"].cpu()[:, :C, 0, 0].double()
    return dx.view(B, H, W, C), dw


def _dw_start(I, acc, dev):
    """the weight-gradient destination before the call: a live bucket (acc) or NaN in the columns to be written; sentinels in the others"""
    C = I["weight"].shape[0]
    dw = I["bucket"].clone() if acc else torch.full_like(I["bucket"], float("nan"))
    dw[:, C:] = SENTINEL
    return dw


def _one_pass(I, cfg, act, acc, wsb):
    lib = _lib.load()
    x = I["x"]
    B, H, W, C = x.shape
    _, ihwo = cfg.packed.get(I["weight"], x.dtype, C, C, None, C)
    out = torch.full_like(x, float("nan"))
    ws = torch.full(((wsb + 3) // 4,), float("nan"), dtype=torch.float32, device=x.device)
    dw = _dw_start(I, acc, x.device)
    adds = I["adds"]
    _lib.check(lib.uegan_gam_bwd(ops._dt(x), ops._p(I["g"]), ops._p(I["y"]), ops._p(x), ops._p(I["rstd"]), ops._p(ihwo), ops._p(adds[0]) if adds else None,
                                 ops._p(adds[1]) if len(adds) > 1 else None, act, ops._p(out), ops._p(dw), 2 * C, C, 1 if acc else 0, ops._p(ws), wsb,
                                 B, H * W, C, ops._stream()))
    return out, dw


def _separate_passes(I, cfg, act, acc):
    """today's route: InstanceNorm backward, 1x1 data gradient, 1x1 weight gradient, activation backward over x's consumers"""
    lib = _lib.load()
    x, g, y = I["x"], I["g"], I["y"]
    B, H, W, C = x.shape
    d = ops._desc(x, None, I["weight"], cfg)
    _, ihwo = cfg.packed.get(I["weight"], x.dtype, C, C, None, C)
    dz = torch.empty_like(x)
    tmp = torch.empty((lib.uegan_reduce_workspace_floats(B, H * W, C),), dtype=torch.float32, device=x.device)
    _lib.check(lib.uegan_instnorm_bwd(ops._dt(x), ops._p(g), ops._p(y), ops._p(I["rstd"]), ops._p(dz), ops._p(tmp), B, H * W, C, ops._stream()))
    dxb, _ = ops.raw_conv_dgrad(d, dz, ihwo)
    dw = _dw_start(I, acc, x.device)
    wsb = lib.uegan_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(((max(wsb, 4) + 3) // 4,), dtype=torch.float32, device=x.device)
    _lib.check(lib.uegan_conv2d_wgrad_acc(ctypes.byref(d), ops._p(x), None, ops._p(dz), None, ops._p(dw), None, ops._p(ws), wsb, 1 if acc else 0, ops._stream()))
    adds = I["adds"]
    if adds or act != ops.ACT_NONE:
        out = torch.empty_like(x)
        _lib.check(lib.uegan_act_bwd3(ops._dt(x), act, ops._p(dxb), ops._p(adds[0]) if adds else None, ops._p(adds[1]) if len(adds) > 1 else None, ops._p(x),
                                      ops._p(out), x.numel(), ops._stream()))
    else:
        out = dxb
    return out, dw


# (B, H, W, grid cap through the knob; 1 = the default grid).  5 x 13 = 65 pixels: ragged and smaller than a tile (C = 32) or one tile + one pixel (C = 64); three
# images on two blocks: a block range that crosses an image boundary inside ragged tiles.  33 x 50 = 1650 pixels on 2 / 3 blocks: multi-tile ranges, with 3 blocks
# one that crosses from image 0 into image 1.
SHAPES = [pytest.param((2, 5, 13, 1), id="2x65"), pytest.param((3, 5, 13, 2), id="3x65cap2"), pytest.param((2, 33, 50, 2), id="2x1650cap2"),
          pytest.param((2, 33, 50, 3), id="2x1650cap3")]
# (addends, activation of x, accumulate into a live bucket)
COMBOS_SMALL = [(0, ops.ACT_NONE, 0), (1, ops.ACT_LRELU, 1), (2, ops.ACT_LRELU, 0), (2, ops.ACT_NONE, 1), (0, ops.ACT_LRELU, 0), (1, ops.ACT_NONE, 0)]
COMBOS_LARGE = [(2, ops.ACT_LRELU, 1), (1, ops.ACT_NONE, 0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_pass_within_twice_the_separate_passes(backend, dtype, C, shape):
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    B, H, W, cap = shape
    prev = _set_knob(cap)
    try:
        for n_add, act, acc in (COMBOS_SMALL if H * W < 100 else COMBOS_LARGE):
            I = _inputs(100 * C + 10 * n_add + act + acc, dtype, dev, B, H, W, C, n_add)
            cfg = ops.ConvCfg(1, ops.PAD_REFLECT, ops.ACT_NONE, cin_used=C)
            wsb = lib.uegan_gam_bwd_ws_bytes(1, B, H * W, C, act)
            assert wsb > 0
            out, dw = _one_pass(I, cfg, act, acc, wsb)
            out2, dw2 = _one_pass(I, cfg, act, acc, wsb)
            old_out, old_dw = _separate_passes(I, cfg, act, acc)
            ref_out, ref_dw = _reference(I, dtype, act, acc)
            tag = "C=%d %s adds=%d act=%d acc=%d" % (C, shape, n_add, act, acc)
            # everything written, nothing unfilled read, the unused columns untouched; bit-reproducible
            assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dw).all()), tag
            assert bool((dw[:, C:] == SENTINEL).all()) and bool((old_dw[:, C:] == SENTINEL).all()), tag
            assert torch.equal(out, out2) and torch.equal(dw, dw2), tag
            e_new = float((out.cpu().double() - ref_out).abs().max())
            e_old = float((old_out.cpu().double() - ref_out).abs().max())
            w_new = float((dw.cpu()[:, :C, 0, 0].double() - ref_dw).abs().max())
            w_old = float((old_dw.cpu()[:, :C, 0, 0].double() - ref_dw).abs().max())
            print("gam_bwd %s %s: dz_enc err %.3e (separate passes %.3e, max |ref| %.3e); dW err %.3e (separate %.3e, max |ref| %.3e)"
                  % (backend, tag, e_new, e_old, float(ref_out.abs().max()), w_new, w_old, float(ref_dw.abs().max())))
            assert e_new <= 2 * e_old, (tag, e_new, e_old)
            assert w_new <= 2 * w_old, (tag, w_new, w_old)
    finally:
        _set_knob(prev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_size_query_declines(backend):
    use_backend(backend)
    ops.set_compute_dtype(torch.bfloat16)
    lib = _lib.load()
    prev = _set_knob(1)
    try:
        assert lib.uegan_gam_bwd_ws_bytes(1, 2, 65, 32, ops.ACT_LRELU) > 0
        assert lib.uegan_gam_bwd_ws_bytes(0, 2, 65, 32, ops.ACT_LRELU) == 0          # fp32 storage
        assert lib.uegan_gam_bwd_ws_bytes(1, 2, 65, 128, ops.ACT_LRELU) == 0         # C = 128
        assert lib.uegan_gam_bwd_ws_bytes(1, 2, 65, 32, ops.ACT_TANH) == 0           # an activation the kernel does not cover
        assert ops.gam_bwd_ws_bytes(torch.float32, 2, 65, 32, ops.ACT_LRELU) == 0
        _set_knob(0)
        assert lib.uegan_gam_bwd_ws_bytes(1, 2, 65, 32, ops.ACT_LRELU) == 0          # knob off
        assert lib.uegan_gam_bwd_ws_bytes(1, 2, 65, 64, ops.ACT_NONE) == 0
    finally:
        _set_knob(prev)


def _generator_grads(dev, x, wts):
    torch.manual_seed(5)
    G = models.Generator(32, "none", "LeakyReLU", False).to(dev)
    xx = x.clone().requires_grad_(True)
    (G(xx) * wts).sum().backward()
    return [xx.grad.detach().cpu()] + [p.grad.detach().cpu() for p in G.parameters()], [n for n, _ in G.named_parameters()]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_generator_gradients_knob_on_against_off(backend, dtype, monkeypatch):
    """The generator at conv_dim 32 on 2 x 3 x 32 x 32: every parameter gradient and the input gradient with the (enc1, ga1) and (enc2, ga2) nodes against the
    separate passes.  The two routes may differ by summation order and by roundings of the storage format in the tensors handed on, each at most one unit
    in the last place = 2^-7 (bf16) / 2^-10 (f16) of the value; a gradient downstream is a sum of such terms, so per tensor
    max |on - off| <= 2 ulp(max |off|) is the bound (1.6e-2 / 2.0e-3 of max |off|).  Observed: with dz_enc kept in fp32 until its one rounding the worst tensor
    was at 5.0e-3 (bf16) / 7.9e-4 (f16); the kernel as it is stores the separate passes' dz_enc, only the two attention weight gradients differ (fp32
    summation order, a few 1e-7 of max |off|) and every other tensor is bit-equal."""
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    wts = torch.randn(2, 3, 32, 32, generator=g).to(dev)
    calls = []
    hub = ops.gam_hub
    monkeypatch.setattr(ops, "gam_hub", lambda *a: (calls.append(1), hub(*a))[1])
    prev = _set_knob(1)
    try:
        on, names = _generator_grads(dev, x, wts)
        assert len(calls) == 2
        _set_knob(0)
        off, _ = _generator_grads(dev, x, wts)
        assert len(calls) == 2
    finally:
        _set_knob(prev)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    worst = 0.0
    for name, a, b in zip(["input"] + names, on, off):
        assert bool(torch.isfinite(a).all()), name
        scale = float(b.abs().max())
        diff = float((a - b).abs().max())
        if scale == 0.0:
            assert diff == 0.0, name          # (the forward-dead gate parameters: exactly zero on both routes)
            continue
        worst = max(worst, diff / scale)
        assert diff <= 2 * ulp * scale, (name, diff, scale)
    print("gam_bwd generator %s %s: worst max|on - off| / max|off| = %.3e" % (backend, dtype, worst))
