"""NIMA aesthetic scorer (uegan_amd/nima.py, csrc/nima.h): the depthwise / pointwise / head / preparation kernels against torch and Pillow,
state-dict parity with the reference's key set, and the whole network against results the reference's own code produced
(tools/make_golden_nima.py -> tests/golden/nima_mbv2*.npz).

Kernel-level tolerance: the a-priori bound of an fp32 dot product of K terms in ANY summation order, (K + 4) * 2^-24 * sum |x||w| * |scale|
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5; + 4 for the affine, the clamp-free residual add and torch's own rounding),
evaluated per test from its operands.  Whole-network tolerance: nima_helpers.bounds()."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nima_helpers as NH
from helpers import BACKENDS, ROOT, golden, use_backend
from uegan_amd import _lib as L
from uegan_amd import nima as N
from uegan_amd import ops

INF = float("inf")
U = 2.0 ** -24


def _pad_c(t, cp):          # pad the last dimension with zeros
    return F.pad(t, (0, cp - t.shape[-1])).contiguous()


# ---- 1. depthwise ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("stride,H,W,C,B,clamp", [
    (1, 14, 14, 144, 1, (0.0, 6.0)), (2, 14, 14, 144, 3, (0.0, 6.0)), (1, 7, 9, 24, 3, (0.0, 6.0)), (2, 7, 9, 24, 1, (0.0, INF)),
    (2, 15, 13, 32, 1, (-INF, INF)), (1, 57, 55, 144, 3, (0.0, 6.0)),       # 4 output rows per lane, a 1-row last strip
    (2, 112, 112, 96, 2, (0.0, 6.0)),                                       # stride 2 with 2 output rows per lane
])
def test_depthwise(backend, stride, H, W, C, B, clamp):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(H * 131 + C + stride)
    cp = N._cp(C)
    x = torch.randn(B, C, H, W, generator=g) * 3.0
    w = torch.randn(C, 1, 3, 3, generator=g)
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    pre = F.conv2d(x.double(), w.double(), stride=stride, padding=1, groups=C) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    ref = pre.clamp(clamp[0], clamp[1])
    if clamp == (0.0, 6.0):
        assert bool((ref == 0).any()) and bool((ref == 6).any())          # both clamp sides are exercised
    mag = F.conv2d(x.abs().double(), w.abs().double(), stride=stride, padding=1, groups=C) * scale.double()[None, :, None, None]
    tol = float((9 + 4) * U * (mag + shift.abs().double()[None, :, None, None]).max())
    xd = _pad_c(x.permute(0, 2, 3, 1), cp).to(dev)
    wd = _pad_c(w.permute(2, 3, 1, 0).reshape(9, C), cp).to(dev)
    sd, hd = _pad_c(scale, cp).to(dev), _pad_c(shift, cp).to(dev)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, cp), float("nan"), device=dev)
    L.check(ops.lib().uegan_nima_dwconv3x3(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y.data_ptr(), B, H, W, cp, stride,
                                           clamp[0], clamp[1], ops._stream()))
    y = y.cpu()
    assert tuple(ref.shape[2:]) == (Ho, Wo)
    err = float((y[..., :C].permute(0, 3, 1, 2).double() - ref).abs().max())
    print("depthwise max error %.3g (bound %.3g)" % (err, tol))
    assert err <= tol
    assert bool((y[..., C:] == 0).all())                                   # padded channels stay exactly zero


# ---- 2. pointwise ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("M,Cin,Cout,residual,clamp", [
    (49, 24, 144, False, (0.0, 6.0)),            # padded Cin, one channel tile per wave
    (200, 144, 24, True, (-INF, INF)),           # the project layer: padded Cout, residual, no activation
    (49, 960, 160, True, (-INF, INF)),
    (3136, 32, 192, False, (0.0, 6.0)),          # two channel tiles per wave
    (1568, 64, 1280, False, (0.0, INF)),         # four: the last 1x1 at batch 32
    (37627, 16, 96, False, (0.0, 6.0)),          # three channel tiles x two pixel tiles, a ragged last row tile
    (37627, 16, 64, False, (0.0, 6.0)),          # four x two
])
def test_pointwise(backend, M, Cin, Cout, residual, clamp):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(M + Cin * 7 + Cout)
    kp, np_ = N._cp(Cin), N._cp(Cout)
    x = torch.randn(M, Cin, generator=g)
    w = torch.randn(Cout, Cin, generator=g) * (3.0 / math.sqrt(Cin))
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    res = torch.randn(M, Cout, generator=g) if residual else None
    conv = F.conv2d(x.double().t().reshape(1, Cin, M, 1), w.double().reshape(Cout, Cin, 1, 1))[0, :, :, 0].t()
    ref = (conv * scale.double() + shift.double()).clamp(clamp[0], clamp[1])
    if clamp == (0.0, 6.0):
        assert bool((ref == 0).any()) and bool((ref == 6).any())
    if residual:
        ref = ref + res.double()
    mag = (x.abs().double() @ w.abs().double().t()) * scale.double() + shift.abs().double() + (res.abs().double() if residual else 0.0)
    tol = float((Cin + 4) * U * mag.max())
    xd = _pad_c(x, kp).to(dev)
    wd = torch.zeros(np_, kp)
    wd[:Cout, :Cin] = w
    wd = wd.to(dev)
    sd, hd = _pad_c(scale, np_).to(dev), _pad_c(shift, np_).to(dev)
    rd = _pad_c(res, np_).to(dev) if residual else None
    y = torch.full((M, np_), float("nan"), device=dev)
    L.check(ops.lib().uegan_nima_pwconv(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), ops._p(rd), y.data_ptr(), M, kp, np_, clamp[0], clamp[1],
                                        ops._stream()))
    y = y.cpu()
    err = float((y[:, :Cout].double() - ref).abs().max())
    print("pointwise max error %.3g (bound %.3g)" % (err, tol))
    assert err <= tol
    assert bool((y[:, Cout:] == 0).all())                                  # padded output channels are exactly 0


def test_kernel_argument_checks():
    use_backend("emu")
    t = torch.zeros(64 * 64)
    p = t.data_ptr()
    with pytest.raises(RuntimeError, match="multiples of 16"):
        L.check(ops.lib().uegan_nima_pwconv(p, p, p, p, None, p, 4, 24, 16, 0.0, 6.0, None))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        L.check(ops.lib().uegan_nima_dwconv3x3(p, p, p, p, p, 1, 4, 4, 20, 1, 0.0, 6.0, None))
    with pytest.raises(RuntimeError, match="bad geometry"):
        L.check(ops.lib().uegan_nima_dwconv3x3(p, p, p, p, p, 1, 4, 4, 16, 3, 0.0, 6.0, None))
    with pytest.raises(RuntimeError, match="classes"):
        L.check(ops.lib().uegan_nima_head(p, p, p, None, p, p, p, 1, 4, 16, 16, 17, None))


# ---- 3. head ----
def _head(dev, x, w, b):
    B, HW, cp = x.shape
    C, n = w.shape[1], w.shape[0]
    pooled = torch.empty(B, C, device=dev)
    probs = torch.empty(B, n, device=dev)
    mean, std = torch.empty(B, device=dev), torch.empty(B, device=dev)
    x, w, b = x.to(dev), w.to(dev), b.to(dev)
    L.check(ops.lib().uegan_nima_head(x.data_ptr(), w.data_ptr(), b.data_ptr(), pooled.data_ptr(), probs.data_ptr(), mean.data_ptr(),
                                      std.data_ptr(), B, HW, cp, C, n, ops._stream()))
    return pooled.cpu(), probs.cpu(), mean.cpu(), std.cpu()


@pytest.mark.parametrize("backend", BACKENDS)
def test_head_matches_torch(backend):
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(11)
    B, C = 3, 1280
    x = torch.randn(B, 49, C, generator=g) + 0.3            # pooled values of both signs: the ReLU matters
    w, b = torch.randn(10, C, generator=g) * 0.08, torch.randn(10, generator=g) * 0.08
    pooled, probs, mean, std = _head(dev, x, w, b)
    xd = x.double()
    rp = F.avg_pool2d(xd.permute(0, 2, 1).reshape(B, C, 7, 7), 7).reshape(B, C)
    assert bool((rp < 0).any())
    rq = torch.softmax(F.linear(torch.relu(rp), w.double(), b.double()), dim=1)
    j = torch.arange(1, 11, dtype=torch.float64)
    rm = (rq * j).sum(1)
    rs = (rq * (j[None] - rm[:, None]) ** 2).sum(1).sqrt()
    # fp32: a 49-term mean (53 u relative), 1280-term logits (a-priori bound on sum |f||w|); |d softmax| <= 2 max |d logit|;
    # |d mean| <= sum_j j |dp_j| <= 55 pt; d std = d var / (2 std) with |d var| <= sum_j (j - m)^2 |dp_j| <= 10 * 81 pt (d mean enters at second order)
    assert float((pooled.double() - rp).abs().max()) <= 53 * U * float(xd.abs().mean(1).max())
    lt = (1280 + 53 + 4) * U * float((torch.relu(rp).abs() @ w.double().abs().t() + b.double().abs()).max())
    pt = 2 * lt + 8 * U
    errs = [float((probs.double() - rq).abs().max()), float((mean.double() - rm).abs().max()), float((std.double() - rs).abs().max())]
    print("head errors probs %.3g mean %.3g std %.3g (bounds %.3g %.3g %.3g)" % (*errs, pt, 55 * pt, 810 * pt / (2 * float(rs.min()))))
    assert errs[0] <= pt and errs[1] <= 55 * pt + 16 * U and errs[2] <= 810 * pt / (2 * float(rs.min())) + 16 * U


@pytest.mark.parametrize("backend", BACKENDS)
def test_head_known_answers(backend):
    dev = use_backend(backend)
    x = torch.rand(2, 49, 1280, generator=torch.Generator().manual_seed(2))
    zero_w = torch.zeros(10, 1280)
    _, probs, mean, std = _head(dev, x, zero_w, torch.zeros(10))           # uniform probabilities
    assert float((probs - 0.1).abs().max()) < 1e-7
    assert float((mean - 5.5).abs().max()) < 1e-5 and float((std - math.sqrt(8.25)).abs().max()) < 1e-5
    for j in (1, 4, 10):                                                    # a one-hot logit at +40: exp(-40) vanishes in fp32
        b = torch.zeros(10)
        b[j - 1] = 40.0
        _, probs, mean, std = _head(dev, x, zero_w, b)
        assert float(probs[0, j - 1]) == 1.0 and float(mean[0]) == float(j) and float(std[0]) < 1e-6


# ---- 4. preparation ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_prepare_image_is_pillow_bit_exact(backend):
    dev = use_backend(backend)
    for n in range(3):
        z = golden("nima_mbv2_prep%d.npz" % n)
        raw = torch.from_numpy(z["raw"])[None].to(dev)
        want = torch.from_numpy(z["out"]).permute(2, 0, 1)[None].float() / 255.0          # ToTensor
        got = N.prepare_image(raw)
        assert got.shape == (1, 3, 224, 224) and torch.equal(got.cpu(), want), "size %s" % (tuple(z["raw"].shape),)
        nhwc = N._prepare(torch.cat([raw, raw]), 4).cpu()                                   # the layout score() feeds the first layer
        assert torch.equal(nhwc[1, :, :, :3].permute(2, 0, 1), want[0]) and bool((nhwc[..., 3] == 0).all())
    # an image that already has a 256-pixel short side is only cropped
    sq = torch.from_numpy(NH.images_u8().numpy()[0])
    big = torch.zeros(1, 256, 300, 3, dtype=torch.uint8)
    big[0, 16:240, 38:262] = sq
    assert torch.equal(N.prepare_image(big.to(dev)).cpu()[0], sq.permute(2, 0, 1).float() / 255.0)


# ---- 5. state-dict parity ----
def test_state_dict_matches_reference_keys():
    z = NH.fixture()
    model = N.NIMA()
    sd = model.state_dict()
    assert len(sd) == 320
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in z["shapes"]]
    assert [str(v.dtype) for v in sd.values()] == [str(d) for d in z["dtypes"]]
    assert list(sd)[0] == "base_model.0.0.0.weight" and list(sd)[-3:] == ["base_model.0.18.1.num_batches_tracked", "head.2.weight", "head.2.bias"]
    full = NH.state_dict()
    model.load_state_dict(full, strict=True)
    seeded = N.seeded_state_dict(int(z["seed"]))
    for k, want in zip(z["checksum_keys"], z["checksums"]):
        got = N.tensor_checksum(seeded[str(k)])
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12), k


# ---- 6. whole network ----
def _deviations(model, x, dev, first_only=False):
    z, blk = NH.fixture(), golden("nima_mbv2_blocks.npz")
    n = x.shape[0]
    taps = {int(i): None for i in blk["indices"]}
    pooled, probs, mean, std = model.forward_all(x.to(dev), taps)
    out = {"pooled": float(np.abs(pooled.cpu().numpy() - z["pooled"][:n]).max() / np.abs(z["pooled"][:n]).max()),
           "probs": float(np.abs(probs.cpu().numpy() - z["probs"][:n]).max()),
           "mean": float(np.abs(mean.cpu().numpy() - z["mean"][:n]).max()),
           "std": float(np.abs(std.cpu().numpy() - z["std"][:n]).max())}
    chans = [N.FIRST_CHANNELS] + [s[1] for s in N.block_specs()]
    for i, step in zip(blk["indices"], blk["steps"]):
        got = taps[int(i)][0, ::step, ::step, :chans[i]].permute(2, 0, 1).cpu().numpy()
        assert bool((taps[int(i)][..., chans[i]:] == 0).all())
        ref = blk["block%d" % i]
        out["block%d" % i] = float(np.abs(got - ref).max() / np.abs(ref).max())
    return out


@pytest.mark.parametrize("backend", BACKENDS)
def test_whole_network_against_reference(backend):
    """Pooled features, probabilities, mean, std and the outputs of blocks 1, 3, 6, 13, 17 against the reference's fp32 results, within
    10 x the reference's own fp32-vs-float64 deviation (nima_helpers.bounds).  The emulator runs the first fixture image only: one forward
    takes about 4 s on the CPU fiber emulator (measured), eight would not fit CPU CI; the GPU runs all eight and records what it saw in
    profiles/nima_parity.json."""
    dev = use_backend(backend)
    model = N.NIMA()
    model.load_state_dict(NH.state_dict(), strict=True)
    model = model.to(dev)
    x = NH.inputs() if backend == "gpu" else NH.inputs()[:1]
    got = _deviations(model, x, dev)
    bound, ref_dev = NH.bounds()
    for k in sorted(got):
        print("%-8s deviation %.3g   bound %.3g   (reference fp32 vs float64 %.3g)" % (k, got[k], bound[k], ref_dev[k]))
    if backend == "gpu":
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "nima_parity.json"), "w") as f:
            json.dump({"what": "NIMA scorer on the device vs the reference's fp32 CPU results on the 8 fixture images (tests/test_nima.py); pooled and "
                               "blocks relative to the quantity's max, probs / mean / std absolute", "device": torch.cuda.get_device_name(0),
                       "deviation": got, "bound": bound, "reference_fp32_vs_float64": ref_dev}, f, indent=1, sort_keys=True)
            f.write("\n")
    for k in got:
        assert got[k] <= bound[k], (k, got[k], bound[k])


# ---- 7. cache invalidation ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_load_state_dict_drops_the_folded_weights(backend):
    dev = use_backend(backend)
    z = NH.fixture()
    model = N.NIMA().to(dev)
    model.load_state_dict(NH.state_dict(perturb_bn=True), strict=True)
    x = NH.inputs()[:1].to(dev)
    stale = model(x).cpu().numpy()
    assert float(np.abs(stale - z["probs"][:1]).max()) > 100 * NH.bounds()[0]["probs"]         # other statistics, another answer
    model.load_state_dict(NH.state_dict(), strict=True)                                         # ... and no stale fold afterwards
    fresh = model(x).cpu().numpy()
    assert float(np.abs(fresh - z["probs"][:1]).max()) <= NH.bounds()[0]["probs"]
    # an in-place edit behind the module's back needs the explicit invalidation, as for every packed weight of the project
    with torch.no_grad():
        model.base_model[0][18][1].running_var.mul_(4.0)
    ops.invalidate_weight_caches()
    assert float(np.abs(model(x).cpu().numpy() - fresh).max()) > 1e-4


# ---- 8. launch budget ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_forward_makes_at_most_54_calls(backend):
    dev = use_backend(backend)
    model = N.NIMA().to(dev)
    x = NH.inputs()[:1].to(dev)
    model(x)                                     # folds and packs the weights
    n0 = L.n_calls
    model(x)
    assert L.n_calls - n0 <= 54                  # 1 first conv + 17 blocks x 3 + 1 last conv + 1 head: nothing runs in a pass of its own


# ---- 9. graph ----
@pytest.mark.gpu
def test_graphed_forward_is_bit_identical():
    dev = use_backend("gpu")
    model = N.NIMA()
    model.load_state_dict(NH.state_dict(), strict=True)
    model = model.to(dev)
    x = NH.inputs().to(dev)
    gr = N.GraphedNIMA(model, 4)
    for xs in (x[:4], x[4:]):
        eager = [t.clone() for t in model.forward_all(xs)]
        replay = gr.forward_all(xs)
        for a, b in zip(eager, replay):
            assert torch.equal(a, b)
        assert torch.equal(gr(xs), eager[1])


# ---- 10. run_test ----
@pytest.mark.gpu
def test_run_test_reports_nima(tmp_path):
    from PIL import Image
    from uegan_amd import data, models, tester
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    G = models.Generator(8, "none", "LeakyReLU", False).to(dev)
    scorer = N.NIMA()
    scorer.load_state_dict(NH.state_dict(), strict=True)
    scorer = scorer.to(dev)
    g = torch.Generator().manual_seed(5)
    raws = [F.interpolate(torch.rand(2, 3, 6, 9, generator=g), size=(64, 96), mode="bilinear", align_corners=True) * 2 - 1 for _ in range(2)]
    paired = [data.Batch(r.flip(0).to(dev), r.to(dev), ["a%d" % (2 * i), "a%d" % (2 * i + 1)]) for i, r in enumerate(raws)]
    unpaired = [data.Batch(None, b.img_raw, b.img_name) for b in paired]                       # no usable labels
    plain = tester.run_test(G, paired)
    assert sorted(plain) == ["mean_psnr", "mean_ssim", "names", "psnr", "ssim"]                # nima=None: what it returned before
    both = tester.run_test(G, paired, nima=scorer)
    assert sorted(both) == ["mean_nima", "mean_psnr", "mean_ssim", "names", "nima", "nima_std", "psnr", "ssim"] and both["psnr"] == plain["psnr"]
    out = tester.run_test(G, unpaired, save_dir=str(tmp_path), tag="1.00", metrics=False, nima=scorer)
    assert out["psnr"] == [] and len(out["nima"]) == 4 and len(out["nima_std"]) == 4 and out["nima"] == both["nima"]
    assert abs(out["mean_nima"] - sum(out["nima"]) / 4) < 1e-12
    saved = [torch.from_numpy(np.array(Image.open(tmp_path / ("%s_1.00_testFakeExp.png" % n)))).to(dev) for n in out["names"]]
    mean, std = N.calc_nima(scorer, saved)
    assert abs(mean - out["mean_nima"]) < 1e-6 and abs(std - sum(out["nima_std"]) / 4) < 1e-6
    assert 1.0 < mean < 10.0
    assert ops.get_compute_dtype() == torch.float32


def test_scorer_ignores_the_compute_dtype():
    """fp32 whatever ops.get_compute_dtype() says, and the setting is left untouched"""
    dev = use_backend("emu")
    model = N.NIMA().to(dev)
    x = NH.inputs()[:1].to(dev)
    want = model(x)
    ops.set_compute_dtype(torch.bfloat16)
    try:
        got = model(x)
        assert ops.get_compute_dtype() == torch.bfloat16 and got.dtype == torch.float32 and torch.equal(got, want)
    finally:
        ops.set_compute_dtype(torch.float32)


# ---- 11. misuse ----
def test_misuse():
    dev = use_backend("emu")
    model = N.NIMA().to(dev)
    x = torch.zeros(1, 3, 224, 224)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model(x)
    model.eval()
    with pytest.raises(ValueError, match="224x224"):
        model(torch.zeros(1, 3, 256, 224))
    with pytest.raises(TypeError):
        model(torch.zeros(1, 3, 224, 224, dtype=torch.float64))
    with pytest.raises(TypeError):
        N.prepare_image(torch.zeros(1, 3, 300, 300))
    with pytest.raises(ValueError):
        N.NIMA(pretrained_base_model=True)


def test_cpu_tensors_without_emulator_raise():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L._reset_for_tests()
    try:
        with pytest.raises(RuntimeError, match="no CPU path"):
            N.NIMA()(torch.zeros(1, 3, 224, 224))
        with pytest.raises(RuntimeError, match="no CPU path"):
            N.prepare_image(torch.zeros(1, 300, 260, 3, dtype=torch.uint8))
    finally:
        L._reset_for_tests()
