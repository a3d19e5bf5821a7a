"""The layout of uegan_amd/ops/ itself: the facade hands out the objects of the home modules, `_lib.load` is the one place where
"did anything reach the kernel library" can be watched, and the autograd convolution and the graph-free raw_conv_* launchers issue the
same launches (one set of launchers in ops/conv.py).  CPU emulator only; images 1 x 3 x 8 x 8, features 1 x 8 x 8 x 8.

Numerical correctness of the paths used here is pinned elsewhere and not repeated: tests/test_ops.py::test_conv_fwd_dgrad_wgrad (the plain
launches against F.conv2d), ::test_conv_dgrad_pad_grid_fold (the data gradient through a workspace) and ::test_conv_fwd_stats (the forward
that emits InstanceNorm moments).  What this file adds is that the two callers of each launcher agree to the bit."""
import ctypes

import pytest
import torch

from helpers import set_tuning, use_backend
from uegan_amd import _lib, codecs, data, fused, nima, ops, tester, variants
from uegan_amd.ops import conv, core, elementwise, layout, loss, optim

HOMES = {
    core: ["ACT_NONE", "ACT_LRELU", "ACT_RELU", "ACT_TANH", "PAD_ZERO", "PAD_REFLECT", "IN_EPS", "SN_EPS", "set_compute_dtype", "get_compute_dtype",
           "set_precise", "precise", "fuse_epilogues", "_weight_epoch", "invalidate_weight_caches", "GradSink", "_sink_of", "_dt", "_p", "_stream",
           "_chk", "lib", "chunk_elems", "cpad", "_farr", "_ptr_table", "workspace"],
    layout: ["to_nhwc", "to_nhwc_pair", "to_nchw", "raw_to_nhwc", "raw_to_nchw_grad", "copy_images"],
    conv: ["PackedWeight", "PackTable", "ConvCfg", "SNCall", "ConvExtras", "StatsHolder", "_desc", "_sub_desc", "split_k", "_ConvFn", "conv2d",
           "specnorm_sigma", "raw_conv_fwd", "raw_conv_dgrad", "raw_conv_wgrad", "refuse_stale_pack"],
    elementwise: ["upsample2x", "maxpool2x2", "instnorm", "instnorm_pair", "moments_acc_new", "moments_window_acc", "moments_finish", "gam_hub",
                  "gam_bwd_ws_bytes", "mul", "residual_clamp", "residual_clamp_pair", "raw_act_bwd", "zero_"],
    loss: ["rahinge", "REC_KINDS", "multiscale_rec", "multiscale_l1", "perceptual_taps_loss", "gather_scalars", "loss_sum"],
    optim: ["FusedAdamL2"],
    codecs: ["PNG_MAX_BAND", "png_encode", "deflate_bands", "JPEG_SUBSAMPLINGS", "JPEG_MAX_SIDE", "jpeg_qtables", "jpeg_capacity", "jpeg_coeffs",
             "jpeg_histogram", "jpeg_build_tables", "jpeg_sizes", "jpeg_encode"],
}


@pytest.fixture
def emu():
    dev = use_backend("emu")
    yield dev
    ops.set_precise(False)
    ops.set_compute_dtype(torch.float32)


def test_facade_exports(emu):
    import uegan_amd
    for home, names in HOMES.items():
        for n in names:
            if n == "set_compute_dtype":
                continue          # (tests/helpers.py wraps this one attribute of the facade; checked through its effect below)
            assert getattr(ops, n) is getattr(home, n), n
    assert ops.L is _lib
    assert uegan_amd.get_compute_dtype is core.get_compute_dtype and uegan_amd.precise is core.precise
    # the flags are lists edited in place: the facade's name is the object the readers hold
    assert ops.split_k is conv.split_k and conv._fwd.__globals__["split_k"] is ops.split_k
    assert ops.fuse_epilogues is core.fuse_epilogues
    assert ops._weight_epoch is core._weight_epoch is conv._weight_epoch
    before = conv._weight_epoch[0]
    ops.invalidate_weight_caches()
    assert conv._weight_epoch[0] == before + 1 == core._weight_epoch[0]
    # the compute dtype is read through its getter everywhere
    img = torch.zeros(1, 3, 8, 8)
    ops.set_compute_dtype(torch.float32)
    assert ops.get_compute_dtype() is torch.float32 and ops.to_nhwc(img).dtype == torch.float32
    ops.set_precise(True)
    assert ops.precise() is False
    ops.set_compute_dtype(torch.bfloat16)
    assert ops.get_compute_dtype() is torch.bfloat16 and core.get_compute_dtype() is torch.bfloat16 and uegan_amd.get_compute_dtype() is torch.bfloat16
    assert ops.to_nhwc(img).dtype == torch.bfloat16 and tuple(ops.to_nhwc(img).shape) == (1, 8, 8, 8)
    assert ops.to_nhwc_pair(img, img).dtype == torch.bfloat16
    assert ops.precise() is True and core.precise() is True


class _Reached(Exception):
    pass


def test_single_patch_point(emu, monkeypatch):
    """every module that launches kernels finds the library through _lib.load at call time"""
    img = torch.zeros(1, 3, 8, 8)
    feat = torch.zeros(1, 8, 8, 8)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    w = torch.nn.Parameter(torch.zeros(8, 8, 3, 3))
    opt = ops.FusedAdamL2([w], lr=1e-3)
    calls = {
        "ops.layout": lambda: ops.to_nhwc(img),
        "ops.conv": lambda: ops.conv2d(feat, None, torch.zeros(8, 8, 3, 3), None, ops.ConvCfg(1, ops.PAD_REFLECT, ops.ACT_NONE)),
        "ops.elementwise": lambda: ops.upsample2x(feat),
        "ops.loss": lambda: ops.multiscale_l1(img, img),
        "ops.optim": lambda: opt.step(),
        "codecs": lambda: codecs.png_encode(u8),
        "tester": lambda: tester.to_uint8_image(img),
        "data": lambda: data.native_input(torch.zeros(1, 32, 32, 3, dtype=torch.uint8)),
        "variants": lambda: variants.rals([torch.zeros(1, 8, 8, 1)], [torch.zeros(1, 8, 8, 1)], True),
        "fused": lambda: fused.discriminator_input([img, img]),
        "nima": lambda: nima.prepare_image(torch.zeros(1, 256, 256, 3, dtype=torch.uint8)),
    }

    def reached(*a, **k):
        raise _Reached()
    monkeypatch.setattr(_lib, "load", reached)
    for name, call in calls.items():
        with pytest.raises(_Reached):
            call()
            pytest.fail("%s reached the library without going through _lib.load" % name)


# (B, C, H, W, Cout, k, pad_mode, which workspace query must be non-zero), dtype
_BASE = (2, 8, 8, 8, 8, 3, ops.PAD_REFLECT, None)
_DGRAD = (2, 8, 8, 8, 8, 3, ops.PAD_REFLECT, "dgrad")          # the same layer with the pad-grid + fold route switched on (as test_ops.py does)
_STATS = (1, 32, 16, 32, 32, 1, ops.PAD_REFLECT, "stats")      # the smallest map whose moments the streaming kernel emits
PARITY_CASES = [
    pytest.param(_BASE, torch.float32, id="2x8x8-3x3-reflect-f32"), pytest.param(_BASE, torch.bfloat16, id="2x8x8-3x3-reflect-bf16"),
    pytest.param(_DGRAD, torch.float32, id="dgrad-workspace-f32"), pytest.param(_DGRAD, torch.bfloat16, id="dgrad-workspace-bf16"),
    # (the fp32 build has no forward that emits moments -- uegan_conv2d_fwd_stats_workspace_bytes is 0 for every fp32 shape -- so this shape runs in bf16)
    pytest.param(_STATS, torch.bfloat16, id="fwd-stats-bf16"),
]


@pytest.mark.parametrize("case,dtype", PARITY_CASES)
def test_launcher_parity(emu, case, dtype):
    """conv2d + backward() and raw_conv_fwd / raw_conv_dgrad / raw_conv_wgrad: bit-equal y, dx, dW, db -- into fresh tensors, into an optimizer
    bucket on first touch, and accumulated there on second touch"""
    B, Cc, H, W, Co, k, pm, query = case
    ops.set_compute_dtype(dtype)
    if query == "dgrad":
        set_tuning("FOLD_MAX", 16384)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, H, W, Cc, generator=g).to(dtype)
    r = torch.randn(B, H, W, Co, generator=g).to(dtype)
    w0 = torch.randn(Co, Cc, k, k, generator=g) * 0.1
    b0 = torch.randn(Co, generator=g)
    d = ops._desc(x, None, w0, ops.ConvCfg(1, pm, ops.ACT_NONE))
    dws = ops.lib().uegan_conv2d_dgrad_workspace_bytes(ctypes.byref(d))
    sws = ops.lib().uegan_conv2d_fwd_stats_workspace_bytes(ctypes.byref(d))
    assert (dws > 0) == (query == "dgrad") and (sws > 0) == (query == "stats"), (dws, sws)

    def params(bucket):
        w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
        opt = ops.FusedAdamL2([w, b], lr=1e-3) if bucket else None
        if opt is not None:
            opt.zero_grad()
        return w, b

    def holder():
        return ops.StatsHolder() if query == "stats" else None

    def via_autograd(w, b):
        cfg, st = ops.ConvCfg(1, pm, ops.ACT_NONE), holder()
        x1 = x.clone().requires_grad_(True)
        y = ops.conv2d(x1, None, w, b, cfg, stats=st)
        y.backward(r)
        return y.detach(), x1.grad, st

    def via_raw(w, b):
        cfg, st = ops.ConvCfg(1, pm, ops.ACT_NONE), holder()
        with torch.no_grad():
            y, desc, ihwo = ops.raw_conv_fwd(x, None, w, b, cfg, stats=st)
            dx, _ = ops.raw_conv_dgrad(desc, r, ihwo)
            dw, db = ops.raw_conv_wgrad(desc, x, None, r, w, b)
        return y, dx, st, dw, db

    # 1. no gradient sink: autograd receives fresh tensors
    wa, ba = params(False)
    ya, dxa, sta = via_autograd(wa, ba)
    wr, br = params(False)
    yr, dxr, str_, dwr, dbr = via_raw(wr, br)
    assert torch.equal(ya, yr) and torch.equal(dxa, dxr) and torch.equal(wa.grad, dwr) and torch.equal(ba.grad, dbr)
    if query == "stats":
        assert sta.value is not None and torch.equal(sta.value, str_.value)
    # 2. a FusedAdamL2 bucket, first touch: both write the bucket and hand autograd nothing
    wa2, ba2 = params(True)
    via_autograd(wa2, ba2)
    wr2, br2 = params(True)
    _, _, _, dw2, db2 = via_raw(wr2, br2)
    assert dw2 is None and db2 is None and wr2._uegan_sink.dirty and br2._uegan_sink.dirty and wa2._uegan_sink.dirty
    assert torch.equal(wa2.grad, wr2.grad) and torch.equal(ba2.grad, br2.grad)
    assert torch.equal(wa2.grad, dwr) and torch.equal(ba2.grad, dbr)           # beta = 0: the bits of a fresh tensor
    # 3. second touch: both accumulate
    via_autograd(wa2, ba2)
    _, _, _, dw3, db3 = via_raw(wr2, br2)
    assert dw3 is None and db3 is None
    assert torch.equal(wa2.grad, wr2.grad) and torch.equal(ba2.grad, br2.grad)
    # (accumulated, not overwritten.  g + g against 2 g: the accumulating launch may add its partial sums to the bucket in another order than it sums
    # them alone -- at most B * H * W <= 512 fp32 additions per element, each within 2^-24 relative: 512 * 6e-8 = 3e-5 of the largest magnitude)
    for acc, one in ((wa2.grad, dwr), (ba2.grad, dbr)):
        assert float((acc - 2 * one).abs().max()) <= 3e-5 * float((2 * one).abs().max())
