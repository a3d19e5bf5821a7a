"""The fidelity loss's backward with the tap gradient and the max-pool backward folded into conv_tall_kernel's data-gradient epilogues
(uegan_conv2d_dgrad_act_tap / uegan_conv2d_dgrad_unpool, UEGAN_TUNE_VGG_EPI): bit-identical to the two passes they replace."""
import ctypes

import pytest
import torch

from helpers import BACKENDS, set_tuning, use_backend
from uegan_amd import _lib, fused, losses, ops

VGG_EPI = 12                     # UEGAN_TUNE_VGG_EPI (include/uegan_hip.h)
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]


def _set_epi(value):
    """the knob on the library of the current compute dtype; returns the previous value"""
    prev = ctypes.c_int(0)
    _lib.check(_lib.load().uegan_set_tuning(VGG_EPI, int(value), ctypes.byref(prev)))
    return prev.value


def _vgg(width_div=1):
    return losses.PerceptualLoss(vgg_weights="seeded", width_div=width_div)


def _conv(P, idx, h):
    """forward of VGG conv `idx` on h (NHWC): its descriptor and the packed weights of its data gradient"""
    conv = P.vgg.features[str(idx)]
    _, d, ihwo = ops.raw_conv_fwd(h, None, conv.weight, conv.bias, conv.cfg)
    return d, ihwo


def _nhwc(g, shape, dtype, dev, relu=False):
    t = torch.randn(*shape, generator=g)
    return (t.clamp(min=0) if relu else t).to(dtype).to(dev)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dgrad_tap_equals_two_passes(backend, dtype):
    """conv1_2's data gradient * relu'(relu1_1) + relu1_1's fidelity-loss gradient in one launch == uegan_conv2d_dgrad_act + uegan_percep_tap_bwd_acc"""
    set_tuning("TALL_MIN_GRID", 1)
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    P = _vgg().to(dev)
    g = torch.Generator().manual_seed(3)
    B, H, W, C = 1, 16, 32, 64
    t = _nhwc(g, (2 * B, H, W, C), dtype, dev, relu=True)          # relu1_1 of [x; y]
    d, ihwo = _conv(P, 2, t)
    dz = _nhwc(g, (B, H, W, C), dtype, dev)
    ty = t[B:]
    gs = torch.tensor([0.75], dtype=torch.float32, device=dev)
    loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    tmp = torch.empty((3 * lib.uegan_reduce_workspace_floats(B, H * W, C),), dtype=torch.float32, device=dev)
    _lib.check(lib.uegan_percep_tap_fwd(ops._dt(t), ops._p(t), ops._p(ty), 1.0 / 64, ops._p(loss), ops._p(tmp), B, H * W, C, ops.IN_EPS, ops._stream()))
    ref, _ = ops.raw_conv_dgrad(d, dz, ihwo, in_act=ops.ACT_RELU, x_act=t, nb=B)
    _lib.check(lib.uegan_percep_tap_bwd_acc(ops._dt(t), ops.ACT_RELU, ops._p(t), ops._p(ty), 1.0 / 64, ops._p(gs), ops._p(ref), ops._p(tmp), B, H * W, C,
                                            ops.IN_EPS, 1, ops._stream()))
    got = fused._dgrad_tap(d, dz, ihwo, t, ty, 1.0 / 64, gs, tmp, B)
    assert got is not None, "conv_tall_kernel should take conv1_2's data gradient here"
    assert torch.equal(got.cpu(), ref.cpu())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dgrad_unpool_equals_two_passes(backend, dtype):
    """conv2_1's data gradient routed through pool1's window positions in one launch == uegan_conv2d_dgrad + uegan_maxpool2x2_bwd_idx"""
    set_tuning("TALL_MIN_GRID", 1)
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    P = _vgg().to(dev)
    g = torch.Generator().manual_seed(5)
    B, H, W, C, Co = 1, 16, 32, 64, 128
    yp = _nhwc(g, (2 * B, H, W, C), dtype, dev, relu=True)         # pool1's output of [x; y] = conv2_1's input
    idx = torch.randint(0, 4, (B, H, W, C), generator=g, dtype=torch.uint8).to(dev)
    d, ihwo = _conv(P, 5, yp)
    dz = _nhwc(g, (B, H, W, Co), dtype, dev)
    cur, _ = ops.raw_conv_dgrad(d, dz, ihwo, nb=B)
    ref = torch.empty((B, 2 * H, 2 * W, C), dtype=dtype, device=dev)
    _lib.check(lib.uegan_maxpool2x2_bwd_idx(ops._dt(yp), ops.ACT_RELU, ops._p(yp), ops._p(idx), ops._p(cur), ops._p(ref), B, 2 * H, 2 * W, C, ops._stream()))
    got = fused._dgrad_unpool(d, dz, ihwo, yp, idx, (B, 2 * H, 2 * W, C), B)
    assert got is not None, "conv_tall_kernel should take conv2_1's data gradient here"
    assert torch.equal(got.cpu(), ref.cpu())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES + [pytest.param(torch.float32, id="f32")])
def test_fused_dgrads_decline_and_write_nothing(backend, dtype):
    """with the knob off (and in the fp32 build, and for an activation other than ReLU) both entry points report 'not applied' and leave the
    destination as it was"""
    set_tuning("TALL_MIN_GRID", 1)
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    P = _vgg().to(dev)
    g = torch.Generator().manual_seed(7)
    B, H, W, C = 1, 16, 32, 64
    t = _nhwc(g, (2 * B, H, W, C), dtype, dev, relu=True)
    d, ihwo = _conv(P, 2, t)
    d5, ihwo5 = _conv(P, 5, t)
    dz = _nhwc(g, (B, H, W, C), dtype, dev)
    dz5 = _nhwc(g, (B, H, W, 128), dtype, dev)
    tmp = torch.zeros((3 * lib.uegan_reduce_workspace_floats(B, H * W, C),), dtype=torch.float32, device=dev)
    idx = torch.zeros((B, H, W, C), dtype=torch.uint8, device=dev)
    db, db5 = ops._sub_desc(d, B), ops._sub_desc(d5, B)
    settings = [(0, ops.ACT_RELU), (1, ops.ACT_LRELU)] if dtype != torch.float32 else [(1, ops.ACT_RELU)]
    prev = _set_epi(1)
    try:
        for epi, act in settings:
            _set_epi(epi)
            out = torch.full((B, H, W, C), 3.0, dtype=dtype, device=dev)
            ok = ctypes.c_int(-1)
            _lib.check(lib.uegan_conv2d_dgrad_act_tap(ctypes.byref(db), ops._p(dz), ops._p(ihwo), None, ops._p(out), act, ops._p(t), ops._p(t[B:]), 1.0,
                                                      None, ops._p(tmp), ctypes.byref(ok), ops._stream()))
            assert ok.value == 0 and bool((out == 3.0).all())
            full = torch.full((B, 2 * H, 2 * W, C), 3.0, dtype=dtype, device=dev)
            ok = ctypes.c_int(-1)
            _lib.check(lib.uegan_conv2d_dgrad_unpool(ctypes.byref(db5), ops._p(dz5), ops._p(ihwo5), None, ops._p(full), act, ops._p(t), ops._p(idx),
                                                     ctypes.byref(ok), ops._stream()))
            assert ok.value == 0 and bool((full == 3.0).all())
    finally:
        _set_epi(prev)


def _fidelity(P, x, y, with_taps):
    xx = x.clone().requires_grad_(True)
    taps = P.reference_taps(y) if with_taps else None
    loss = P(xx, y, y_taps=taps)
    loss.backward()
    return loss.detach().clone(), xx.grad.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_taps", [False, True], ids=["y_half", "y_taps"])
@pytest.mark.parametrize("size", [(2, 256, 7), (1, 512, 8)], ids=["2x256", "1x512"])
def test_vgg_fidelity_backward_bit_identical(monkeypatch, dtype, with_taps, size):
    """the whole fidelity loss, forward and backward, with the epilogue folds on and off: the loss and dx are bit-equal.  At 512^2 every data gradient
    behind a tap or a pool runs on conv_tall_kernel (all eight folds apply); at 256^2 conv5_1's 16^2 map does not (pool4 takes the two passes)."""
    set_tuning("TALL_MIN_GRID", 1)
    dev = use_backend("gpu")
    ops.set_compute_dtype(dtype)
    P = _vgg().to(dev)
    B, S, n_folds = size
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, S, S, generator=g).to(dev)
    y = torch.rand(B, 3, S, S, generator=g).to(dev)
    applied = []
    for name in ("_dgrad_tap", "_dgrad_unpool"):
        def counted(*args, _f=getattr(fused, name)):
            r = _f(*args)
            applied.append(r is not None)
            return r
        monkeypatch.setattr(fused, name, counted)
    prev = _set_epi(1)
    try:
        on = _fidelity(P, x, y, with_taps)
        assert sum(applied) == n_folds, applied
        applied.clear()
        _set_epi(0)
        off = _fidelity(P, x, y, with_taps)
        assert sum(applied) == 0, applied
    finally:
        _set_epi(prev)
    torch.cuda.synchronize()
    assert torch.equal(on[0], off[0])
    assert torch.equal(on[1], off[1])
    assert bool(torch.isfinite(on[1]).all()) and float(on[1].abs().max()) > 0
