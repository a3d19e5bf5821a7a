"""Native-size inference (`--test_img_size 0`): uegan_native_input (csrc/input.hip) through data.native_input, uegan_montage_crop_u8
(csrc/metrics.hip) through tester.montage_u8(window=) / to_uint8_image(window=), tester.enhance_native, the native mode of the test loader,
tester.run_test on its batches and the command line.

The mode is defined as crop(G(reflect_extend(normalise(pixels)))).  The two kernels are pinned bit for bit against the composition of pieces
that existed before them (data.input_transform at the image's own size + F.pad(mode="reflect"); a slice + the oracle's to_uint8_image), the
whole path bit for bit against the same composition through the public API, and against the CPU oracle with the project's fp32 bar."""
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
from uegan_amd import _lib, data, models, ops, runner, tester


def _pixels(seed, B, h, w):
    """random bytes; 0 and 255 are planted so that both ends of the normalisation are exercised whatever the draw"""
    g = torch.Generator().manual_seed(seed)
    pix = torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8)
    pix[:, 0, 0, :] = 0
    pix[:, -1, -1, :] = 255          # the corner every extended row and column reflects about
    pix[:, h // 2, w // 2, 0], pix[:, h // 2, w // 2, 1] = 0, 255
    return pix


def _photo(seed, h, w):
    """a photograph-shaped 8-bit image [1,h,w,3]: low-pass noise plus a little grain (cf. test_parity_full._smooth_images)"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(1, 3, max(h // 16, 2), max(w // 16, 2), generator=g)
    x = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False) + 0.03 * torch.randn(1, 3, h, w, generator=g)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _composed_input(pix):
    """the parent commit's pieces: a same-size resize is Pillow's identity (one unit tap per output), then torch's reflection padding"""
    h, w = pix.shape[1:3]
    hp, wp = data.padded_size(h, w)
    return F.pad(data.input_transform(pix, (h, w)), (0, wp - w, 0, hp - h), mode="reflect")


def _check_input(pix):
    got = data.native_input(pix)
    want = _composed_input(pix)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0
    assert torch.equal(got, want)


# ---- 1. the input kernel, bit-exact ----
def test_padded_size():
    assert data.padded_size(32, 48) == (32, 48) and data.padded_size(33, 47) == (48, 48) and data.padded_size(40, 52) == (48, 64)
    assert data.padded_size(336, 500) == (336, 512) and data.padded_size(2000, 3008) == (2000, 3008)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(1, 32, 48), (1, 33, 47), (1, 40, 52), (1, 47, 33), (2, 40, 52)], ids=lambda s: "x".join(map(str, s)))
def test_native_input_bit_exact(backend, shape):
    """(32,48): nothing is extended.  (33,47): 15 rows and 1 column, odd width: bytes throughout.  (40,52): w % 4 == 0: dwords inside the image,
    bytes in the 12 extended columns and 8 extended rows.  (47,33): the transpose.  B = 2: the image stride."""
    dev = use_backend(backend)
    B, h, w = shape
    _check_input(_pixels(30 + h, B, h, w).to(dev))


@pytest.mark.parametrize("backend", BACKENDS)
def test_native_input_misaligned_source_falls_back(backend):
    """the shape qualifies for the dword path, but the image starts 1 byte into its buffer: 4-byte loads would be misaligned"""
    dev = use_backend(backend)
    pix = _pixels(35, 1, 40, 52)
    buf = torch.empty(pix.numel() + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    view = buf[1:1 + pix.numel()].view(pix.shape)
    view.copy_(pix)
    assert view.is_contiguous() and view.data_ptr() % 4 == 1
    _check_input(view)


# ---- 2. the crop montage, bit-exact ----
def _check_crop(images, window, dev, on_device=None):
    H, W = window
    want = O.to_uint8_image(torch.cat([x[:, :, :H, :W] for x in images], 3))
    assert int(want.min()) == 0 and int(want.max()) == 255          # both clamps are exercised
    got = tester.montage_u8(*(on_device if on_device is not None else [x.to(dev) for x in images]), window=window)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    return got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("src,window", [((48, 48), (33, 47)), ((48, 64), (40, 52))], ids=["scalar", "vector"])
def test_montage_crop_bit_exact(backend, n, src, window):
    dev = use_backend(backend)
    imgs = _images(40 + n, n, 2, *src)
    got = _check_crop(imgs, window, dev)
    if n == 1:
        assert torch.equal(tester.to_uint8_image(imgs[0].to(dev), window=window), got)


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_crop_full_window_is_montage(backend):
    dev = use_backend(backend)
    for shape in ((48, 64), (33, 47)):
        imgs = [x.to(dev) for x in _images(43, 2, 2, *shape)]
        assert torch.equal(tester.montage_u8(*imgs, window=shape), tester.montage_u8(*imgs))
        assert torch.equal(tester.to_uint8_image(imgs[0], window=shape), tester.to_uint8_image(imgs[0]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_crop_misaligned_source_falls_back(backend):
    """shape and window qualify for the vector path, but the first source starts 1 float into its buffer"""
    dev = use_backend(backend)
    a, b = _images(44, 2, 2, 48, 64)
    buf = torch.empty(a.numel() + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _check_crop([a, b], (40, 52), dev, on_device=[view, b.to(dev)])


# ---- 3. past the grid caps (GPU) ----
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1150, 1820), (1139, 1811)], ids=["dword", "byte"])
def test_native_input_past_the_grid_cap(shape):
    """the launcher caps its grid at NATIVE_MAX_BLOCKS blocks of NATIVE_THREADS threads, NATIVE_VEC output pixels per thread: just above that
    count of PADDED pixels the kernel takes its grid-stride loop a second time (both sizes pad to 1152 x 1824)"""
    dev = use_backend("gpu")
    h, w = shape
    hp, wp = data.padded_size(h, w)
    cap = data.NATIVE_MAX_BLOCKS * data.NATIVE_THREADS * data.NATIVE_VEC
    assert cap < hp * wp <= cap * 1.01 and (w % 4 == 0) == (shape == (1150, 1820))
    _check_input(_pixels(50, 1, h, w).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("src,window", [((1040, 1040), (1028, 1024)), ((528, 528), (513, 513))], ids=["vector", "scalar"])
def test_montage_crop_past_the_grid_cap(src, window):
    """uegan_montage_u8's caps (test_montage_past_the_grid_cap), counted in pixels of the WINDOW"""
    dev = use_backend("gpu")
    H, W = window
    per_thread = tester.MONTAGE_VEC if W % tester.MONTAGE_VEC == 0 else 1
    cap = tester.MONTAGE_MAX_BLOCKS * tester.MONTAGE_THREADS * per_thread
    assert cap < H * W <= cap * 1.01
    _check_crop(_images(51, 1, 1, *src), window, dev)


# ---- 4. refusals, all before any launch ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_native_refusals(backend, monkeypatch):
    dev = use_backend(backend)
    launched = []
    real = _lib.load

    class _Spy:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: _Spy())
    G = models.Generator(8, "none", "LeakyReLU", False)
    for shape in ((1, 31, 48), (1, 48, 31)):
        pix = torch.zeros(shape + (3,), dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError, match="31"):
            data.native_input(pix)
        with pytest.raises(ValueError, match="31"):
            tester.enhance_native(G, pix)
    x = torch.zeros(1, 3, 48, 64, device=dev)
    for window in ((49, 64), (48, 65), (0, 8)):
        with pytest.raises(ValueError):
            tester.montage_u8(x, x, window=window)
        with pytest.raises(ValueError):
            tester.to_uint8_image(x, window=window)
    # the area cap is a predicate of its own: no test allocates an image that large
    assert data.NATIVE_MAX_PIXELS == 8 * 1024 * 1024
    assert data.check_native_size(2048, 4096) == (2048, 4096) and data.check_native_size(2000, 3008) == (2000, 3008)
    with pytest.raises(ValueError, match=str(2048 * 4112)):
        data.check_native_size(2048, 4097)
    with pytest.raises(ValueError, match=str(2064 * 4096)):
        data.check_native_size(2049, 4096)
    for bad in (torch.zeros(1, 40, 52, 3, device=dev), torch.zeros(1, 40, 52, 3, dtype=torch.int32, device=dev),
                torch.zeros(1, 40, 52, 4, dtype=torch.uint8, device=dev), torch.zeros(40, 52, 3, dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            data.native_input(bad)
        with pytest.raises(ValueError):
            tester.enhance_native(G, bad)
    assert launched == []


# ---- 5. end to end against the composition and the oracle ----
def _generator(cd, dev):
    PG = O.init_params(O.generator_param_shapes(cd), 41, "default")
    G = models.Generator(cd, "none", "LeakyReLU", False)
    G.load_state_dict(PG)
    return PG, (G.to(dev) if dev.type != "cpu" else G)


def _composed_enhance(G, pix):
    h, w = pix.shape[1:3]
    return tester.to_uint8_image(tester.enhance(G, _composed_input(pix)))[:, :h, :w]


def _psnr_u8(a, b):
    """CalcPSNR.py:85-92 without the border crop"""
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _check_against_oracle(PG, pix, got):
    """the project's fp32 bar (test_inference_psnr_ssim_against_oracle: >= 60 dB), and no byte further than 1 from the oracle's"""
    h, w = pix.shape[1:3]
    hp, wp = data.padded_size(h, w)
    x = (pix.cpu().permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5
    with torch.no_grad():
        ref = O.generator_forward(PG, F.pad(x, (0, wp - w, 0, hp - h), mode="reflect"))
    ref8 = O.to_uint8_image(ref[:, :, :h, :w])
    diff = int((got.cpu().int() - ref8.int()).abs().max())
    psnr = _psnr_u8(got.cpu(), ref8)
    print("native %dx%d vs oracle: max 8-bit difference %d, PSNR %.2f dB" % (h, w, diff, psnr))
    assert diff <= 1 and psnr >= 60.0, (diff, psnr)


@pytest.mark.parametrize("backend", BACKENDS)
def test_enhance_native_against_composition_and_oracle(backend):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    PG, G = _generator(8, dev)
    pix = _photo(60, 40, 52).to(dev)
    got, pair = tester.enhance_native(G, pix, compare=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 40, 52, 3) and tuple(pair.shape) == (1, 40, 104, 3)
    assert torch.equal(got, tester.enhance_native(G, pix))
    assert torch.equal(got, _composed_enhance(G, pix))                                   # (a)
    assert torch.equal(pair[:, :, 52:], got) and torch.equal(pair[:, :, :52], pix)       # raw | enhanced; the raw panel is the file's bytes
    _check_against_oracle(PG, pix, got)                                                  # (b)
    pix = _photo(61, 32, 48).to(dev)                                                     # (c) nothing to extend: the plain path
    assert torch.equal(tester.enhance_native(G, pix), tester.to_uint8_image(tester.enhance(G, data.input_transform(pix, (32, 48)))))


# ---- 6. a photograph-shaped size (GPU): the first non-square, non-power-of-two full-width run of G ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_enhance_native_336x500(dtype):
    dev = use_backend("gpu")
    ops.set_compute_dtype(dtype)
    PG, G = _generator(32, dev)
    pix = _photo(62, 336, 500).to(dev)
    assert data.padded_size(336, 500) == (336, 512)
    got = tester.enhance_native(G, pix)
    assert tuple(got.shape) == (1, 336, 500, 3)
    assert torch.equal(got, _composed_enhance(G, pix))
    if dtype == torch.float32:
        _check_against_oracle(PG, pix, got)


# ---- 7. the loader's native mode and run_test ----
def _tree(root, sizes, label_sizes=None):
    from PIL import Image
    for d in ("label", "raw"):
        (root / d).mkdir(parents=True)
    arrs = {}
    for i, (h, w) in enumerate(sizes):
        lh, lw = (label_sizes or sizes)[i]
        for d, hh, ww in (("label", lh, lw), ("raw", h, w)):
            a = _photo(70 + i + 10 * (d == "raw"), hh, ww)[0].numpy()
            Image.fromarray(a, "RGB").save(root / d / ("im%02d.png" % i))
            arrs[(d, i)] = a
    return arrs


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


@pytest.mark.parametrize("backend", BACKENDS)
def test_native_loader_and_run_test(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    # a relative, dot-free data root: the sample name is the path up to its first '.'.  The loader remembers image sizes per path and other
    # modules' trees are "data/raw/im00.png" too, with other sizes: these trees have roots of their own
    monkeypatch.chdir(tmp_path)
    sizes = [(40, 52), (33, 47)]
    arrs = _tree(Path("native"), sizes)
    _, G = _generator(8, dev)

    loader = data.get_test_loader("native", 0, batch_size=2, num_workers=2, device=dev)
    batches = list(loader)
    assert len(batches) == 1 and sorted(batches[0].img_name) == ["im00", "im01"]      # (in listing order, which is the file system's)
    for k, name in enumerate(batches[0].img_name):
        i = int(name[2:])
        h, w = sizes[i]
        assert batches[0].paths[k] == ("native/label/%s.png" % name, "native/raw/%s.png" % name)
        for got, key in ((batches[0].img_exp[k], "label"), (batches[0].img_raw[k], "raw")):
            assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 3) and got.data_ptr() % 4 == 0
            assert np.array_equal(got[0].cpu().numpy(), arrs[(key, i)])
    res = tester.run_test(G, loader, save_dir="out", tag="2.00", compare_dir="cmp")
    loader.close()
    assert res["names"] == batches[0].img_name and res["sizes"] == [list(sizes[int(name[2:])]) for name in res["names"]]
    for k, name in enumerate(res["names"]):
        i = int(name[2:])
        h, w = sizes[i]
        want = tester.enhance_native(G, torch.from_numpy(arrs[("raw", i)])[None].to(dev))
        img = _png(Path("out") / ("im%02d_2.00_testFakeExp.png" % i))
        assert img.shape == (h, w, 3) and np.array_equal(img, want[0].cpu().numpy())
        pair = _png(Path("cmp") / ("im%02d_2.00_testRealRaw_testFakeExp.png" % i))
        assert pair.shape == (h, 2 * w, 3) and np.array_equal(pair[:, w:], img) and np.array_equal(pair[:, :w], arrs[("raw", i)])
        label = torch.from_numpy(_png(Path("native") / "label" / ("im%02d.png" % i))).to(dev)      # the label FILE, decoded with Pillow
        assert res["psnr"][k] == tester.calculate_psnr(want[0], label)
        assert res["ssim"][k] == tester.calculate_ssim(want[0], label)
    assert res["mean_psnr"] == tester.mean_metric(res["psnr"]) and res["mean_ssim"] == tester.mean_metric(res["ssim"])

    # the resizing mode is where it was: the same tree at 32 through get_test_loader and through a loader built the way get_test_loader built it
    new = data.get_test_loader("native", 32, batch_size=2, num_workers=2, device=dev)
    old = data.DeviceLoader(data.ReferenceDataset("native"), 2, 32, 32, False, False, False, 2, dev)
    got, want = tester.run_test(G, new, save_dir="new32", tag="2.00"), tester.run_test(G, old, save_dir="old32", tag="2.00")
    for b_new, b_old in zip(new, old):
        assert isinstance(b_new, data.Batch) and tuple(b_new.img_raw.shape) == (2, 3, 32, 32)
        assert torch.equal(b_new.img_raw, b_old.img_raw) and torch.equal(b_new.img_exp, b_old.img_exp)
    new.close()
    old.close()
    assert got == want and "sizes" not in got and len(got["psnr"]) == 2
    for f in sorted(os.listdir("old32")):
        assert _png(Path("new32") / f).shape == (32, 32, 3) and np.array_equal(_png(Path("new32") / f), _png(Path("old32") / f))


@pytest.mark.parametrize("backend", BACKENDS)
def test_native_run_test_refuses_label_of_another_size(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    _tree(Path("mixed"), [(40, 52), (33, 47)], label_sizes=[(40, 52), (47, 33)])
    _, G = _generator(8, dev)
    loader = data.get_test_loader("mixed", 0, batch_size=2, num_workers=2, device=dev)
    try:
        with pytest.raises(ValueError, match=r"label/im01\.png.*raw/im01\.png"):
            tester.run_test(G, loader)
        res = tester.run_test(G, loader, metrics=False)          # the unpaired setting needs no label
        assert sorted(res["sizes"]) == [[33, 47], [40, 52]] and res["psnr"] == []
    finally:
        loader.close()


# ---- 8. the command line ----
def test_test_mode_native_size(tmp_path, monkeypatch):
    dev = use_backend("emu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    sizes = [(40, 52), (33, 47), (36, 36)]
    arrs = _tree(Path("photos"), sizes)
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    mdir = Path("results") / "UEGAN-FiveK" / "models"
    mdir.mkdir(parents=True)
    torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    got = runner.main(["--mode", "test", "--test_img_dir", "photos", "--test_img_size", "0", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
                       "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "2", "--is_test_nima", "False"])
    out = Path("results") / "UEGAN-FiveK" / "test"
    assert sorted(os.listdir(out / "test_results")) == ["im%02d_2.00_testFakeExp.png" % i for i in range(3)]
    assert sorted(os.listdir(out / "test_compare")) == ["im%02d_2.00_testRealRaw_testFakeExp.png" % i for i in range(3)]
    with open(out / "test_metrics.json") as f:
        saved = json.load(f)
    assert sorted(saved["names"]) == ["im00", "im01", "im02"]
    psnr, ssim = [], []
    for name in saved["names"]:
        i = int(name[2:])
        h, w = sizes[i]
        want = tester.enhance_native(G, torch.from_numpy(arrs[("raw", i)])[None].to(dev))
        img = _png(out / "test_results" / ("im%02d_2.00_testFakeExp.png" % i))
        assert img.shape == (h, w, 3) and np.array_equal(img, want[0].numpy())
        pair = _png(out / "test_compare" / ("im%02d_2.00_testRealRaw_testFakeExp.png" % i))
        assert pair.shape == (h, 2 * w, 3) and np.array_equal(pair[:, w:], img) and np.array_equal(pair[:, :w], arrs[("raw", i)])
        psnr.append(tester.calculate_psnr(want[0], torch.from_numpy(arrs[("label", i)])))
        ssim.append(tester.calculate_ssim(want[0], torch.from_numpy(arrs[("label", i)])))
    assert saved["sizes"] == [list(sizes[int(name[2:])]) for name in saved["names"]] and got["sizes"] == saved["sizes"]
    assert saved["psnr"] == psnr and saved["ssim"] == ssim
    assert saved["mean_psnr"] == pytest.approx(tester.mean_metric(psnr), rel=1e-12) and got["mean_psnr"] == saved["mean_psnr"]
    assert saved["mean_ssim"] == pytest.approx(tester.mean_metric(ssim), rel=1e-12) and got["mean_ssim"] == saved["mean_ssim"]
