"""Tiled native-size inference: uegan_upsample2x_fwd_at (csrc/elementwise.hip) through ops.upsample2x(at=), uegan_moments_window_acc /
uegan_moments_finish (csrc/norm.hip) through ops.moments_window_acc / ops.moments_finish, uegan_montage_place_u8 (csrc/metrics.hip) through
tester.montage_place_u8, Generator.tile_moments / forward(tile=), tester.enhance_tiled, tester.enhance_native(tile=) and run_test(native_tile=).

Tiling is an evaluation strategy of the native mode's definition crop(G(reflect_extend(normalise(pixels)))), not an approximation: section 4 shows on
the CPU, in fp64, that the two-pass composition with halos (32, 80) reproduces the untiled oracle to 1e-10 and that either halo one grid step
shorter leaves a visible seam with these weights; section 5 holds the kernels' composition against the same oracle with the untiled forward's own
error as the yardstick.

Backends: the kernel tests (1-3) and the refusals run on both helpers.BACKENDS.  Everything that runs the generator tile by tile (5, and the
run_test cases of 6) runs on the GPU only: the emulator needs ~160 s for ONE tiled 208 x 272 forward at conv_dim 8.

With UEGAN_TILED_PARITY_OUT=<file> in the environment the measured figures (window-moment errors, tiled / untiled error ratios) are written there as
JSON when the module finishes: that is how profiles/tiled_parity.json is made."""
import functools
import json
import math
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import BACKENDS, use_backend
from oracle import uegan_oracle as O
from test_montage import _images
from test_native import _photo, _png, _tree
from uegan_amd import _lib, data, models, ops, tester

_RECORD = {"window_moments": {}, "end_to_end": {}}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("UEGAN_TILED_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _plain_mode():
    yield
    ops.set_precise(False)


DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
# one unit in the last place of the storage format, relative to the value
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


# ---- 1. positioned up-sampling ----
def _src(o, n):
    """bilinear_src (csrc/elementwise.hip) in numpy fp32: source indices and the second weight of GLOBAL output index o of an n -> 2n up-sampling"""
    scale = np.float32(n - 1) / np.float32(2 * n - 1)
    s = scale * o.astype(np.float32)
    i0 = s.astype(np.int32)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float64)


def _check_upsample_tile(x, oy, ox, H, W, dev):
    """the tile [oy, oy+H) x [ox, ox+W) of the NHWC map x against the global result: bit-identical where no source index was clamped into the tile,
    and everywhere the clamped gather: an fp64 blend of the stored values with the weights of _src.  The kernel is away from it by (a) its weights: the
    source coordinate s = scale * o is an fp32 product, and whether the compiler contracts `s - i0` into a fused multiply-add or not, the weight moves
    by at most one unit in the last place of s <= 2^-23 * max(GH, GW), which moves the blend by that times |v1 - v0| <= 2 max|x|, once per axis; (b) the
    fp32 blend itself, 4 roundings of 2^-24 max|x|; (c) one rounding to the storage format, a unit in its last place"""
    GH, GW = x.shape[1:3]
    full = ops.upsample2x(x)
    got = ops.upsample2x(x[:, oy:oy + H, ox:ox + W].contiguous(), at=(oy, ox, GH, GW))
    assert tuple(got.shape) == (x.shape[0], 2 * H, 2 * W, x.shape[3]) and got.dtype == x.dtype
    y0, y1, ly = _src(np.arange(2 * oy, 2 * oy + 2 * H), GH)
    x0, x1, lx = _src(np.arange(2 * ox, 2 * ox + 2 * W), GW)
    free_y = (y0 >= oy) & (y1 <= oy + H - 1)
    free_x = (x0 >= ox) & (x1 <= ox + W - 1)
    free = torch.from_numpy(free_y[:, None] & free_x[None, :])
    assert bool(free.any()) and not bool(free.all())          # the tile has an interior and a halo that asks for sources it does not hold
    want = full[:, 2 * oy:2 * oy + 2 * H, 2 * ox:2 * ox + 2 * W].cpu()
    assert torch.equal(got.cpu()[:, free], want[:, free])
    t = x[:, oy:oy + H, ox:ox + W].cpu().double()
    cy0, cy1 = np.clip(y0 - oy, 0, H - 1), np.clip(y1 - oy, 0, H - 1)
    cx0, cx1 = np.clip(x0 - ox, 0, W - 1), np.clip(x1 - ox, 0, W - 1)
    wy, wx = torch.from_numpy(ly)[None, :, None, None], torch.from_numpy(lx)[None, None, :, None]
    top = (1 - wx) * t[:, cy0][:, :, cx0] + wx * t[:, cy0][:, :, cx1]
    bot = (1 - wx) * t[:, cy1][:, :, cx0] + wx * t[:, cy1][:, :, cx1]
    ref = (1 - wy) * top + wy * bot
    tol = (4 * 2.0 ** -24 + 2 * 2 * 2.0 ** -23 * max(GH, GW)) * float(x.abs().max()) + ULP[x.dtype] * ref.abs()
    assert bool(((got.cpu().double() - ref).abs() <= tol).all())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24, 12])
def test_upsample_at(backend, dtype, C):
    """C = 8, 24: one 16-byte chunk per thread in every format; C = 12: the scalar path of the 16-bit formats.  12 x 20 map: a tile strictly inside,
    and one touching the bottom-right corner, where the global sampling phase has drifted furthest from a tile-local one"""
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(100 + C)
    x = (torch.rand(2, 12, 20, C, generator=g) * 4 - 2).to(dtype).to(dev)
    with torch.no_grad():
        assert torch.equal(ops.upsample2x(x, at=(0, 0, 12, 20)), ops.upsample2x(x))          # the whole map: bit-identical to uegan_upsample2x_fwd
        _check_upsample_tile(x, 4, 8, 6, 8, dev)
        _check_upsample_tile(x, 6, 12, 6, 8, dev)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.upsample2x(x, at=(0, 0, 12, 20))
    with torch.no_grad(), pytest.raises(ValueError):
        ops.upsample2x(x, at=(4, 8, 12, 20))          # 12 rows from row 4 of a 12-row map


# ---- 2. window moments ----
# The launcher (csrc/norm.hip make_win_plan): V channels per thread (one 16-byte chunk: 4 fp32 / 8 half; 1 when C is no multiple or a pointer is
# misaligned), CG = pow2 >= C / V channel lanes (<= 64; beyond that ncg > 1 channel groups), PL = 256 / CG pixel lanes, S = ceil(n / (4 PL)) pixel
# splits of the window's n pixels, capped at 512 (then a split is longer than 4 pixels per lane).  The fold adds the S partials in split order.
WINDOW_CASES = {
    # name: (dtype, B, H, W, C, what engages)
    "f32_c8": (torch.float32, 2, 40, 52, 8),            # V 4, CG 2, PL 128: S = 1 for the inner window (96 px <= 512), 5 for the whole map (2080 px)
    "half_c24": (torch.bfloat16, 2, 40, 52, 24),        # V 8, CG 4 (3 of 4 channel lanes live), PL 64: S = 1 and 9
    "f16_c24": (torch.float16, 2, 40, 52, 24),
    "half_c12_scalar": (torch.bfloat16, 1, 40, 52, 12), # C % 8 != 0: V 1, CG 16, PL 16: S = 2 and 33
    "f32_c260_two_groups": (torch.float32, 1, 10, 12, 260),   # V 4, 65 lanes: CG 64, ncg 2 (one live lane in the second group), PL 4: S = 8
    "f32_c64_split_cap": (torch.float32, 1, 184, 184, 64),    # V 4, CG 16, PL 16: 33856 px > 512 * 64: the split cap, 67 px per split
}


def _windows(H, W):
    return {"inside": (3, 11, 5, 17) if H >= 20 else (2, 7, 3, 9), "two_edges": (H // 2, H, W // 3, W), "whole": (0, H, 0, W)}


def _old_moments(z, dev):
    """uegan_moments on a contiguous NHWC tensor -> (mean, var) [B, C] fp32"""
    B, H, W, C = z.shape
    st = torch.empty((2, B, C), dtype=torch.float32, device=dev)
    tmp = torch.empty((ops.lib().uegan_reduce_workspace_floats(B, H * W, C),), dtype=torch.float32, device=dev)
    ops.L.check(ops.lib().uegan_moments(ops._dt(z), z.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), tmp.data_ptr(), B, H * W, C, ops._stream()))
    return st.cpu().double()


def _new_moments(x, win, x_lo=None):
    acc = ops.moments_acc_new(x.shape[0], x.shape[3], x.device)
    ops.moments_window_acc(x, win, acc, x_lo=x_lo)
    n = (win[1] - win[0]) * (win[3] - win[2])
    return ops.moments_finish(acc, n, eps=-1.0).cpu().double(), ops.moments_finish(acc, n).cpu().double(), acc


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", sorted(WINDOW_CASES))
def test_window_moments(backend, case):
    """accuracy bar: the error of uegan_moments on a contiguous copy of the window against fp64 numpy; the new mean and variance may have at most
    twice that error (they are the double-precision sums rounded once, so they should have no more)"""
    dev = use_backend(backend)
    dtype, B, H, W, C = WINDOW_CASES[case]
    ops.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(len(case))
    x = (torch.randn(B, H, W, C, generator=g) * 0.5 + torch.linspace(-3, 3, C)).to(dtype).to(dev)
    for name, win in _windows(H, W).items():
        y0, y1, x0, x1 = win
        z = x[:, y0:y1, x0:x1].contiguous()
        ref = z.cpu().double().reshape(B, -1, C)
        mean64, var64 = ref.mean(1), ref.var(1, unbiased=False)
        old = _old_moments(z, dev)
        new, new_rstd, acc = _new_moments(x, win)
        e_old = (float((old[0] - mean64).abs().max()), float((old[1] - var64).abs().max()))
        e_new = (float((new[0] - mean64).abs().max()), float((new[1] - var64).abs().max()))
        print("window moments %s/%s: mean error old %.3e new %.3e, variance error old %.3e new %.3e" % (case, name, e_old[0], e_new[0], e_old[1], e_new[1]))
        _RECORD["window_moments"]["%s/%s/%s" % (backend, case, name)] = {"mean_err_uegan_moments": e_old[0], "mean_err_window": e_new[0],
                                                                        "var_err_uegan_moments": e_old[1], "var_err_window": e_new[1]}
        assert e_new[0] <= 2 * e_old[0] and e_new[1] <= 2 * e_old[1]
        assert torch.equal(new_rstd[0], new[0])
        rstd64 = 1 / torch.sqrt(var64 + 1e-5)
        assert float(((new_rstd[1] - rstd64).abs() / rstd64).max()) <= 2.0 ** -22          # rounded once from double; var's own error is ~1e-16 relative
        # the same call again: the same bits
        assert torch.equal(_new_moments(x, win)[2], acc)
    # two windows in sequence = the sum of the two alone (each alone is 0 + t, and the sequence adds the second t to the first)
    top, bottom = (0, H // 2, 0, W), (H // 2, H, 0, W)
    both = ops.moments_acc_new(B, C, dev)
    ops.moments_window_acc(x, top, both)
    ops.moments_window_acc(x, bottom, both)
    assert torch.equal(both, _new_moments(x, top)[2] + _new_moments(x, bottom)[2])
    # ... and the two halves together are the whole map's moments up to double rounding: n terms of at most amax^2, each sum good to ~n * 2^-53
    whole = _new_moments(x, (0, H, 0, W))[2]
    amax = max(1.0, float(x.float().abs().max()))
    assert float((both - whole).abs().max()) <= 2.0 ** -40 * H * W * amax * amax


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_window_moments_pair(backend, dtype):
    """z = hi + lo: against fp64 of the two stored planes added (exact in double).  The result is the double sum rounded to fp32 once"""
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(7)
    v = torch.randn(2, 20, 24, 8, generator=g) * 0.5 + 1.5
    hi = v.to(dtype)
    lo = (v - hi.float()).to(dtype)
    win = (3, 20, 0, 17)
    new = _new_moments(hi.to(dev), win, x_lo=lo.to(dev))[0]
    ref = (hi.double() + lo.double())[:, 3:20, 0:17].reshape(2, -1, 8)
    mean64, var64 = ref.mean(1), ref.var(1, unbiased=False)
    assert float((new[0] - mean64).abs().max()) <= 2.0 ** -24 * float(mean64.abs().max())
    assert float((new[1] - var64).abs().max()) <= 2.0 ** -24 * float(var64.abs().max())
    assert not torch.equal(new, _new_moments(hi.to(dev), win)[0])          # the lo plane counts


@pytest.mark.parametrize("backend", BACKENDS)
def test_window_moments_misaligned_and_refusals(backend):
    """a map that starts 4 bytes into its buffer: 16-byte loads would be misaligned, the launcher takes one channel per thread"""
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    x = torch.randn(1, 20, 24, 8, generator=torch.Generator().manual_seed(8))
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=dev)
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    win = (3, 11, 5, 17)
    a, b = _new_moments(view, win)[0], _new_moments(x.to(dev), win)[0]
    ref = x[:, 3:11, 5:17].double().reshape(1, -1, 8)
    assert float((a[0] - ref.mean(1)).abs().max()) <= 2.0 ** -24 * 4 and float((a - b).abs().max()) <= 2.0 ** -22
    acc = ops.moments_acc_new(1, 8, dev)
    for bad in ((3, 3, 0, 4), (0, 21, 0, 4), (-1, 4, 0, 4), (0, 4, 5, 25)):
        with pytest.raises(ValueError):
            ops.moments_window_acc(x.to(dev), bad, acc)
    with pytest.raises(ValueError):
        ops.moments_window_acc(x.to(dev), win, acc.float())
    assert float(acc.abs().max()) == 0.0


# ---- 3. placement ----
def _check_place(images, src_window, dst_hw, origin, panel, dev, on_device=None):
    sy, sx, h, w = src_window
    dy, dx = origin
    B = images[0].shape[0]
    g = torch.Generator().manual_seed(3)
    dst = torch.randint(0, 256, (B,) + tuple(dst_hw) + (3,), generator=g, dtype=torch.uint8)
    want = dst.clone()
    for k, x in enumerate(images):
        x[:, :, sy, sx], x[:, :, sy + h - 1, sx + w - 1] = -1.5, 1.5          # both clamps act inside the window, at its first and last pixel
        q = O.to_uint8_image(x[:, :, sy:sy + h, sx:sx + w])
        assert int(q.min()) == 0 and int(q.max()) == 255
        want[:, dy:dy + h, dx + k * panel:dx + k * panel + w] = q
    assert not torch.equal(want, dst)
    if on_device is not None:
        for x, d in zip(images, on_device):
            d.copy_(x)
    got = tester.montage_place_u8(dst.to(dev), on_device if on_device is not None else [x.to(dev) for x in images], src_window, origin, panel=panel)
    assert torch.equal(got.cpu(), want)          # the window bit for bit, every other byte as it was


PLACE_CASES = {
    # name: (source H x W, window (sy, sx, h, w), destination H x W, origin, panel)
    "vector": ((48, 64), (5, 4, 30, 24), (50, 80), (7, 8), 32),
    "scalar_odd_width": ((48, 64), (5, 4, 30, 21), (50, 80), (7, 8), 32),
    "scalar_odd_source_offset": ((48, 64), (5, 3, 30, 24), (50, 80), (7, 8), 32),
    "scalar_odd_destination": ((48, 64), (5, 4, 30, 24), (50, 77), (7, 5), 29),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("case", sorted(PLACE_CASES))
def test_montage_place_bit_exact(backend, n, case):
    dev = use_backend(backend)
    src, window, dst, origin, panel = PLACE_CASES[case]
    _check_place(_images(60 + n, n, 2, *src), window, dst, origin, panel, dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_place_misaligned_source_and_crop_equivalence(backend):
    dev = use_backend(backend)
    a, b = _images(63, 2, 2, 48, 64)
    buf = torch.empty(a.numel() + 8, dtype=torch.float32, device=dev)
    view = buf[1:1 + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4
    _check_place([a, b], (5, 4, 30, 24), (50, 80), (7, 8), 32, dev, on_device=[view, b.to(dev)])
    # the whole destination from the top-left window: uegan_montage_crop_u8
    dst = torch.zeros((2, 40, 104, 3), dtype=torch.uint8, device=dev)
    assert torch.equal(tester.montage_place_u8(dst, [a.to(dev), b.to(dev)], (0, 0, 40, 52), (0, 0)), tester.montage_u8(a.to(dev), b.to(dev), window=(40, 52)))
    for window, origin, panel in (((0, 0, 49, 8), (0, 0), None), ((0, 60, 8, 8), (0, 0), None), ((0, 0, 8, 8), (33, 0), None), ((0, 0, 8, 52), (0, 1), None),
                                  ((0, 0, 8, 8), (0, 0), 7), ((-1, 0, 8, 8), (0, 0), None)):
        with pytest.raises(ValueError):
            tester.montage_place_u8(dst, [a.to(dev), b.to(dev)], window, origin, panel=panel)


@pytest.mark.gpu
@pytest.mark.parametrize("src,window,dst,origin", [((1040, 1040), (8, 16, 1028, 1024), (1040, 1056), (4, 12)), ((528, 528), (9, 7, 513, 513), (530, 531), (11, 13))],
                         ids=["vector", "scalar"])
def test_montage_place_past_the_grid_cap(src, window, dst, origin):
    """uegan_montage_u8's caps (test_montage_past_the_grid_cap), counted in pixels of the window"""
    dev = use_backend("gpu")
    h, w = window[2:]
    per_thread = tester.MONTAGE_VEC if w % tester.MONTAGE_VEC == 0 else 1
    cap = tester.MONTAGE_MAX_BLOCKS * tester.MONTAGE_THREADS * per_thread
    assert cap < h * w <= cap * 1.01
    _check_place(_images(64, 1, 1, *src), window, dst, origin, w, dev)


# ---- 4. the halo constants, CPU only: a tiled composition of the oracle's layer functions in fp64 ----
def _seam_weights(cd, std=0.15, seed=5):
    """every parameter, biases included, from N(0, std): the default orthogonal gain 0.02 makes G ~ identity and a missing halo invisible"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * std for k, s in O.generator_param_shapes(cd).items()}


def _up_at64(x, oy, ox, GH, GW):
    """NCHW fp64: the tile's window of the global x2 align_corners up-sampling, sources clamped into the tile"""
    H, W = x.shape[2:]

    def src(o, n, lo, size):
        s = o.double() * (n - 1) / (2 * n - 1)
        i0 = s.floor().long()
        i1 = (i0 + 1).clamp(max=n - 1)
        return (i0 - lo).clamp(0, size - 1), (i1 - lo).clamp(0, size - 1), s - i0
    y0, y1, ly = src(torch.arange(2 * oy, 2 * oy + 2 * H), GH, oy, H)
    x0, x1, lx = src(torch.arange(2 * ox, 2 * ox + 2 * W), GW, ox, W)
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def _oracle_tiled(P, x, core, halo_enc, halo):
    """the two-pass scheme written with the oracle's layers: pass 1 the encoder per tile and sum z, sum z^2 of z_k = W_fuse[:, :C] x_k over each
    core; pass 2 the whole network per tile with IN(z_k) on the global moments and the positioned up-sampling, keeping the core"""
    Hp, Wp = x.shape[2:]

    def encoder(t):
        acts = [O.conv_block(P, "enc1", t, 1)]
        for k in range(2, 6):
            acts.append(O.conv_block(P, "enc%d" % k, acts[-1], 2))
        return acts

    def fuse_in(k, a):
        return F.conv2d(a, P["ga%d.fuse.0.weight" % (k + 1)][:, :a.shape[1]])
    sums = [0, 0, 0, 0, 0]
    sqs = [0, 0, 0, 0, 0]
    for cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1 in data.native_tiles(Hp, Wp, core, halo_enc):
        for k, a in enumerate(encoder(x[:, :, ty0:ty1, tx0:tx1])):
            z = fuse_in(k, a)[:, :, (cy0 - ty0) >> k:(cy1 - ty0) >> k, (cx0 - tx0) >> k:(cx1 - tx0) >> k]
            sums[k] = sums[k] + z.sum((2, 3))
            sqs[k] = sqs[k] + (z * z).sum((2, 3))
    norm = []
    for k in range(5):
        n = (Hp >> k) * (Wp >> k)
        mean = sums[k] / n
        norm.append((mean[:, :, None, None], 1 / torch.sqrt(sqs[k] / n - mean * mean + O.IN_EPS)[:, :, None, None]))
    out = torch.empty_like(x)
    for cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1 in data.native_tiles(Hp, Wp, core, halo):
        t = x[:, :, ty0:ty1, tx0:tx1]
        acts = encoder(t)
        ga = [(fuse_in(k, a) - norm[k][0]) * norm[k][1] for k, a in enumerate(acts)]
        y = ga[4]
        for k in (4, 3, 2, 1):      # upsample(5 - k): the map at stride 2^k -> 2^(k-1)
            pre = "upsample%d.1.main.1" % (5 - k)
            y = F.conv2d(_up_at64(y, ty0 >> k, tx0 >> k, Hp >> k, Wp >> k), P[pre + ".weight"], P[pre + ".bias"])
            y = O.conv_block(P, "dec%d" % (5 - k), torch.cat([y, ga[k - 1]], 1), 1)
        res = torch.tanh(O.sn_conv(P, "dec5.1", O.sn_conv(P, "dec5.0", y * acts[0])))
        out[:, :, cy0:cy1, cx0:cx1] = torch.clamp(res + t, -1, 1)[:, :, cy0 - ty0:cy1 - ty0, cx0 - tx0:cx1 - tx0]
    return out


@functools.lru_cache(maxsize=None)
def _seam_case64():
    P = {k: v.double() for k, v in _seam_weights(8).items()}
    x = torch.rand(1, 3, 208, 272, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        return P, x, O.generator_forward(P, x)


@pytest.mark.parametrize("core", [32, 64, 96])
def test_halo_constants(core):
    """halos (NATIVE_TILE_HALO_ENC, NATIVE_TILE_HALO) = (32, 80) reproduce the untiled oracle to rounding; either one a stride-16 grid step shorter
    leaves a seam -- which is also what shows that these weights make a seam visible at all"""
    assert (data.NATIVE_TILE_HALO_ENC, data.NATIVE_TILE_HALO, data.NATIVE_TILE) == (32, 80, 1024)
    P, x, ref = _seam_case64()
    with torch.no_grad():
        exact = float((_oracle_tiled(P, x, core, 32, 80) - ref).abs().max())
        short_dec = float((_oracle_tiled(P, x, core, 32, 64) - ref).abs().max())
        short_enc = float((_oracle_tiled(P, x, core, 16, 80) - ref).abs().max())
    print("core %d: halos (32, 80) %.2e, (32, 64) %.2e, (16, 80) %.2e" % (core, exact, short_dec, short_enc))
    assert exact < 1e-10
    assert short_dec > 1e-4 and short_enc > 1e-4


# ---- 5. end to end on the GPU ----
MODES = {"f32": (torch.float32, False, 8), "bf16": (torch.bfloat16, False, 8), "f16": (torch.float16, False, 8), "f16_precise": (torch.float16, True, 32)}
IMAGES = {"208x272": (208, 272), "ragged_203x267": (203, 267)}


def _seam_std(cd):
    """N(0, 0.15) is the issue's draw for conv_dim 8.  The precise mode exists at conv_dim 32 only (Generator._precise): there the same per-layer gain
    needs 0.15 * sqrt(8 / 32), since every fan-in but the image's grows with conv_dim -- at 0.15 the activations double per layer more and tanh saturates"""
    return 0.15 * math.sqrt(8.0 / cd)


@functools.lru_cache(maxsize=None)
def _e2e_case(cd, image):
    """(weights, uint8 pixels, fp64 oracle on the reflect-extended image): computed once per module run"""
    h, w = IMAGES[image]
    P = _seam_weights(cd, _seam_std(cd))
    pix = _photo(90 + h, h, w)
    hp, wp = data.padded_size(h, w)
    x = F.pad((pix.permute(0, 3, 1, 2).double() / 255 - 0.5) / 0.5, (0, wp - w, 0, hp - h), mode="reflect")
    with torch.no_grad():
        ref = O.generator_forward({k: v.double() for k, v in P.items()}, x)
    return P, pix, ref


def _generator(P, cd, dev, flags=("none", "LeakyReLU", False)):
    G = models.Generator(cd, *flags)
    G.load_state_dict(P)
    return G.to(dev).eval()


def _errors(y, ref):
    d = (y.detach().cpu().double() - ref).abs()
    return float(d.max()), float((d * d).mean().sqrt())


def _bar(mode, tiled, untiled):
    """fp32 storage: the moments' summation order is the only difference -> max error at most 2 e0.  16-bit storage: rounding flips move individual
    pixels, not the distribution -> rms at most 1.25 x, max at most 2 x the untiled error"""
    ratios = {"max": tiled[0] / untiled[0], "rms": tiled[1] / untiled[1]}
    ok = ratios["max"] <= 2.0 and (mode == "f32" or ratios["rms"] <= 1.25)
    return ratios, ok


@pytest.mark.gpu
@pytest.mark.parametrize("core", [64, 96])
@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_enhance_tiled_against_oracle(mode, image, core):
    dev = use_backend("gpu")
    dtype, precise, cd = MODES[mode]
    ops.set_compute_dtype(dtype)
    ops.set_precise(precise)
    P, pix, ref = _e2e_case(cd, image)
    G = _generator(P, cd, dev)
    x = data.native_input(pix.to(dev))
    assert tuple(x.shape) == (1, 3, 208, 272)
    with torch.no_grad():
        untiled = _errors(tester.enhance(G, x), ref)
        tiled = _errors(tester.enhance_tiled(G, x, core), ref)
    assert untiled[0] > 0 and untiled[1] > 0, untiled
    ratios, ok = _bar(mode, tiled, untiled)
    print("%s %s core %d: untiled max %.3e rms %.3e, tiled max %.3e rms %.3e, ratios max %.3f rms %.3f"
          % (mode, image, core, untiled[0], untiled[1], tiled[0], tiled[1], ratios["max"], ratios["rms"]))
    _RECORD["end_to_end"]["%s/%s/core%d" % (mode, image, core)] = {"untiled_max": untiled[0], "untiled_rms": untiled[1], "tiled_max": tiled[0],
                                                                  "tiled_rms": tiled[1], "ratio_max": ratios["max"], "ratio_rms": ratios["rms"]}
    assert untiled[0] > 0 and ok, (untiled, tiled, ratios)


@pytest.mark.gpu
@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_enhance_native_tiled(mode, image):
    """the uint8 path is the fp32 path, tile for tile: bit-equal to quantising enhance_tiled's result; in fp32 within one level of the untiled call"""
    dev = use_backend("gpu")
    dtype, precise, cd = MODES[mode]
    ops.set_compute_dtype(dtype)
    ops.set_precise(precise)
    P, pix, _ = _e2e_case(cd, image)
    G = _generator(P, cd, dev)
    pix = pix.to(dev)
    h, w = pix.shape[1:3]
    got, pair = tester.enhance_native(G, pix, compare=True, tile=64)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 3) and tuple(pair.shape) == (1, h, 2 * w, 3)
    with torch.no_grad():
        want = tester.to_uint8_image(tester.enhance_tiled(G, data.native_input(pix), 64), window=(h, w))
    assert torch.equal(got, want)
    assert torch.equal(got, tester.enhance_native(G, pix, tile=64))
    plain, plain_pair = tester.enhance_native(G, pix, compare=True)
    assert torch.equal(pair[:, :, w:], got) and torch.equal(pair[:, :, :w], plain_pair[:, :, :w]) and torch.equal(pair[:, :, :w], pix)
    diff = int((got.int() - plain.int()).abs().max())
    print("%s %s: tiled against untiled uint8, max difference %d levels, %d bytes differ" % (mode, image, diff, int((got != plain).sum())))
    if mode == "f32":
        assert diff <= 1


def _plain_reference(sd, x):
    """eval-mode forward of the reference generator with g_use_sn True, InstanceNorm(affine, running statistics), SELU in fp64: spectral norm without a
    power iteration (sigma = u^T W v), the norm on its running statistics, the attention modules in full (gate branch included)"""
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}

    def block(pre, t, stride):
        y = O.reflect_conv(t, O.spectral_norm_weight(P, pre + ".main.1", False), P[pre + ".main.1.bias"], stride)
        y = F.instance_norm(y, P[pre + ".main.2.running_mean"], P[pre + ".main.2.running_var"], P[pre + ".main.2.weight"], P[pre + ".main.2.bias"],
                            use_input_stats=False, eps=1e-5)
        return F.selu(y)

    def gam(pre, t):
        mean, std = O.calc_mean_std(t)
        g = F.conv2d(F.relu(F.conv2d(torch.cat([mean, std], 1), P[pre + ".conv.0.weight"])), P[pre + ".conv.2.weight"])
        y = F.conv2d(torch.cat([t, g.expand_as(t)], 1), O.spectral_norm_weight(P, pre + ".fuse.0", False), P[pre + ".fuse.0.bias"])
        return F.instance_norm(y, eps=O.IN_EPS)

    def up(pre, t):
        t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
        return F.conv2d(t, O.spectral_norm_weight(P, pre + ".1.main.1", False), P[pre + ".1.main.1.bias"])
    a = [block("enc1", x, 1)]
    for k in range(2, 6):
        a.append(block("enc%d" % k, a[-1], 2))
    y = gam("ga5", a[4])
    for k in (4, 3, 2, 1):
        y = block("dec%d" % (5 - k), torch.cat([up("upsample%d" % (5 - k), y), gam("ga%d" % k, a[k - 1])], 1), 1)
    res = torch.tanh(O.sn_conv(P, "dec5.1", O.sn_conv(P, "dec5.0", y * a[0])))
    return torch.clamp(res + x, -1, 1)


@pytest.mark.gpu
def test_enhance_tiled_non_default_generator():
    """g_use_sn True, InstanceNorm, SELU: Generator._body_plain.  In eval mode its norms use running statistics and spectral norm does not iterate, so
    the attention modules are again the only non-local layers.  fp32, the fp32 bar"""
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    G = models.Generator(8, "InstanceNorm", "SELU", True)
    g = torch.Generator().manual_seed(9)
    sd = {}
    for k, v in G.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v
        elif k.endswith(("weight_u", "weight_v")):
            sd[k] = F.normalize(torch.randn(v.shape, generator=g), dim=0)
        elif k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif ".main.2.weight" in k:
            sd[k] = 1 + torch.randn(v.shape, generator=g) * 0.15
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.15
    # u, v as a checkpoint holds them: power-iterated on weight_orig (three training forwards' worth).  With u, v independent of the weight,
    # sigma = u^T W v is ~0, W / sigma ~1e2 per layer, tanh saturates everywhere and both errors are exactly 0: nothing would be compared
    for k in sd:
        if k.endswith("weight_orig"):
            for _ in range(3):
                O.spectral_norm_weight(sd, k[:-len(".weight_orig")], True)
    G.load_state_dict(sd)
    G = G.to(dev).eval()
    assert not G.default_flags
    x = torch.rand(1, 3, 208, 272, generator=g) * 2 - 1
    with torch.no_grad():
        ref = _plain_reference(sd, x.double())
        untiled = _errors(tester.enhance(G, x.to(dev)), ref)
        tiled = _errors(tester.enhance_tiled(G, x.to(dev), 64), ref)
    assert 0 < untiled[0] < 1e-3, untiled          # (exactly 0: a saturated network, whose output is +-1 + x whatever the tiles do)
    ratios, ok = _bar("f32", tiled, untiled)
    print("non-default generator: untiled max %.3e, tiled max %.3e, ratio %.3f" % (untiled[0], tiled[0], ratios["max"]))
    _RECORD["end_to_end"]["f32_in_selu_sn/208x272/core64"] = {"untiled_max": untiled[0], "tiled_max": tiled[0], "ratio_max": ratios["max"]}
    assert ok, (untiled, tiled)


# ---- 6. plumbing ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_tiled_refusals(backend, monkeypatch):
    """training mode and enabled gradients raise; a bad core or size raises ValueError; all before any launch"""
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    G = models.Generator(8, "none", "LeakyReLU", False)
    G = G.to(dev) if dev.type != "cpu" else G
    x = torch.zeros(1, 3, 64, 96, device=dev)
    pix = torch.zeros(1, 64, 96, 3, dtype=torch.uint8, device=dev)
    moments = [torch.zeros(2, 1, 8 << k, device=dev) for k in range(5)]
    launched = []
    real = _lib.load

    class _Spy:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: _Spy())
    tile = models.Tile(0, 0, 64, 96, moments)
    G.eval()
    with pytest.raises(RuntimeError, match="no_grad"):          # eval mode, gradients enabled
        tester.enhance_tiled(G, x, 32)
    with pytest.raises(RuntimeError, match="no_grad"):
        G(x, tile=tile)
    with pytest.raises(RuntimeError, match="no_grad"):
        G.tile_moments(x, (0, 64, 0, 96), G.tile_moments_new(1, dev))
    with torch.no_grad():
        G.train()
        with pytest.raises(RuntimeError, match="eval"):         # no gradients, training mode
            tester.enhance_tiled(G, x, 32)
        with pytest.raises(RuntimeError, match="eval"):
            G(x, tile=tile)
        G.eval()
        for core in (16, 40, 0, 33):
            with pytest.raises(ValueError, match="multiple of 16"):
                tester.enhance_tiled(G, x, core)
            with pytest.raises(ValueError, match="multiple of 16"):
                tester.enhance_native(G, pix, tile=core)
        with pytest.raises(ValueError):
            tester.enhance_tiled(G, x[:, :, :60], 32)
        with pytest.raises(ValueError):
            G(x, tile=models.Tile(16, 0, 64, 96, moments))      # the tile does not lie inside the image
        with pytest.raises(ValueError):
            models.Tile(8, 0, 64, 96, moments)
        for window in ((0, 8, 0, 96), (0, 64, 16, 112), (32, 32, 0, 96)):
            with pytest.raises(ValueError, match="multiples of 16"):
                G.tile_moments(x, window, G.tile_moments_new(1, dev))
        # the caps are predicates of their own: no test allocates an image that large
        assert data.NATIVE_TILED_MAX_PIXELS == 4096 * 6144
        assert data.check_native_tiled_size(4096, 6144) == (4096, 6144) and data.check_native_tiled_size(4090, 6130) == (4096, 6144)
        with pytest.raises(ValueError, match=str(4096 * 6160)):
            data.check_native_tiled_size(4096, 6145)
        monkeypatch.setattr(data, "NATIVE_MAX_PIXELS", 64 * 64)
        with pytest.raises(ValueError, match="exercised"):      # a tile (core + halos, clipped: the whole 64 x 96 image) above the per-forward cap
            tester.enhance_tiled(G, x, 32)
    assert launched == []


def _run(G, root, dev, **kw):
    loader = data.get_test_loader(root, 0, batch_size=2, num_workers=2, device=dev)
    try:
        return tester.run_test(G, loader, **kw)
    finally:
        loader.close()


@pytest.mark.gpu
def test_run_test_native_tile(tmp_path, monkeypatch):
    """run_test(native_tile=64) on a two-image native directory: PNGs of the source sizes; PSNR / SSIM against the untiled run.  In fp32 the tiled and
    untiled results are each within 2 e0 and e0 of the oracle (test_enhance_tiled_against_oracle), e0 ~ 1e-4 = 0.013 grey levels: a byte can differ
    only where the value lies within 3 e0 = 0.04 levels of a rounding boundary, so at most ~4 % of the bytes differ, by one level.  A changed byte
    moves the squared error against the label by 2 |d| + 1 <= 511; 5 % of them move a mean squared error of 10^3 .. 10^4 (random weights against an
    unrelated label) by under 0.3 %, 0.012 dB.  SSIM is a mean of local terms each Lipschitz in its 7 x 7 window's bytes: one level on 5 % of the
    bytes of windows whose variance is hundreds of levels^2 stays below 1e-3."""
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    sizes = [(203, 267), (176, 208)]
    _tree(Path("tiled"), sizes)
    G = _generator(_seam_weights(8), 8, dev)
    plain = _run(G, "tiled", dev, save_dir="plain", tag="1.00")
    tiled = _run(G, "tiled", dev, save_dir="out", tag="1.00", compare_dir="cmp", native_tile=64)
    assert tiled["names"] == plain["names"] and tiled["sizes"] == plain["sizes"] == [list(sizes[int(n[2:])]) for n in tiled["names"]]
    for k, name in enumerate(tiled["names"]):
        h, w = sizes[int(name[2:])]
        a, b = _png(Path("out") / (name + "_1.00_testFakeExp.png")), _png(Path("plain") / (name + "_1.00_testFakeExp.png"))
        assert a.shape == b.shape == (h, w, 3)
        off = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert off.max() <= 1 and (off > 0).mean() <= 0.05
        assert _png(Path("cmp") / (name + "_1.00_testRealRaw_testFakeExp.png")).shape == (h, 2 * w, 3)
        assert abs(tiled["psnr"][k] - plain["psnr"][k]) < 0.02 and abs(tiled["ssim"][k] - plain["ssim"][k]) < 1e-3


@pytest.mark.gpu
def test_run_test_tiles_above_the_cap(tmp_path, monkeypatch):
    """the automatic path: a sample whose padded area exceeds NATIVE_MAX_PIXELS used to abort the run with ValueError; it is now enhanced tile by tile"""
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    _tree(Path("big"), [(260, 270), (64, 80)])
    G = _generator(_seam_weights(8), 8, dev)
    monkeypatch.setattr(data, "NATIVE_MAX_PIXELS", 65536)
    monkeypatch.setattr(data, "NATIVE_TILE", 32)
    with pytest.raises(ValueError, match="exercised"):
        tester.enhance_native(G, torch.zeros(1, 260, 270, 3, dtype=torch.uint8, device=dev))          # 272 x 272 = 73984 > 65536: the untiled path refuses
    calls = []
    real = tester.enhance_native
    monkeypatch.setattr(tester, "enhance_native", lambda G, p, compare=False, tile=None: (calls.append((tuple(p.shape[1:3]), tile)), real(G, p, compare, tile))[1])
    res = _run(G, "big", dev, save_dir="out", tag="1.00")
    assert sorted(res["sizes"]) == [[64, 80], [260, 270]] and len(res["psnr"]) == 2
    assert sorted(calls) == [((64, 80), None), ((260, 270), 32)]          # only the sample above the cap is tiled
    assert _png(Path("out") / "im00_1.00_testFakeExp.png").shape == (260, 270, 3)
