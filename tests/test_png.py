"""PNG files encoded on the device: csrc/png.hip through ops.png_encode / ops.deflate_bands, tester.write_pngs with its encoder selection, and the
command line with UEGAN_PNG_ENCODER=device.

The oracle is independent of the code under test: Pillow's decoder and zlib.decompress.  Every file is decoded with Pillow and compared with the
pixels, and walked chunk by chunk here: every chunk CRC against zlib.crc32, one IDAT per band, the concatenated IDAT payloads inflated with zlib
(which also checks the Adler-32 and refuses incomplete or over-subscribed codes), H * (3W + 1) filtered bytes, filter types in 0..4."""
import io
import os
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import BACKENDS, use_backend
from test_data import _make_tree
from test_native import _generator, _photo, _pixels, _tree
from test_runner import _png
from uegan_amd import data, models, ops, runner, tester
import uegan_amd

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FIXED = 8 + 25 + 12 + 6          # signature, IHDR, IEND, zlib header + Adler-32


def _chunks(png):
    assert png[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        kind, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(kind + body) == crc, (kind, len(out))
        out.append((kind, body))
        pos += 12 + n
    assert pos == len(png)
    return out


def _check_file(png, pixels, bands=None):
    """pixels: uint8 [H,W,3] numpy.  -> the IDAT payloads"""
    from PIL import Image
    H, W, _ = pixels.shape
    with Image.open(io.BytesIO(png)) as im:
        assert im.mode == "RGB" and im.size == (W, H)
        assert np.array_equal(np.array(im), pixels)
    chunks = _chunks(png)
    assert chunks[0] == (b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) and chunks[-1] == (b"IEND", b"")
    idat = [body for kind, body in chunks[1:-1]]
    assert all(kind == b"IDAT" for kind, _ in chunks[1:-1]) and len(idat) >= 1
    if bands is not None:
        assert len(idat) == bands
    raw = zlib.decompress(b"".join(idat))
    assert len(raw) == H * (3 * W + 1)
    assert all(t <= 4 for t in raw[::3 * W + 1])
    return idat


def _n_bands(H, W, band_bytes=65535):
    rows = band_bytes // (3 * W + 1)
    return -(-H // rows)


def _blocks(idat):
    """'stored' / 'coded' per band, from the block header every byte-aligned band starts with (the first band after the 2-byte zlib header)"""
    kinds = []
    for k, body in enumerate(idat):
        first = body[2 if k == 0 else 0]
        assert (first >> 1) & 3 in (0, 2)
        kinds.append("stored" if (first >> 1) & 3 == 0 else "coded")
    return kinds


# ---- 1. smallest shapes, default band ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 7), (1, 5, 1), (1, 3, 5), (1, 33, 47), (2, 40, 52)], ids=lambda s: "x".join(map(str, s)))
def test_smallest_shapes(backend, shape):
    """(33, 47): a row of 142 bytes, no multiple of 4.  B = 2: other content per image, so other sizes, and each file is its own image.  _pixels draws
    noise, which every encoder stores (n + 5 bytes per band whatever the bytes are), so the second image keeps 16 of its levels (0 and 255 among
    them): its bands are coded, and the two sizes can differ at all."""
    dev = use_backend(backend)
    B, H, W = shape
    pix = _pixels(50 + H, B, H, W)
    if B == 2:
        pix[1] = pix[1] // 17 * 17
    files = ops.png_encode(pix.to(dev))
    assert len(files) == B and all(isinstance(f, bytes) for f in files)
    for b in range(B):
        _check_file(files[b], pix[b].numpy(), bands=1)
    if B == 2:
        assert not torch.equal(pix[0], pix[1]) and len(files[0]) != len(files[1])


# ---- 2. band structure ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("band_bytes,bands", [(142, 33), (142 * 4, 9), (142 * 33, 1), (142 * 33 - 1, 2)], ids=["rows", "ragged", "one", "32+1"])
def test_band_structure(backend, band_bytes, bands):
    dev = use_backend(backend)
    pix = _photo(51, 33, 47)
    assert _n_bands(33, 47, band_bytes) == bands
    png, = ops.png_encode(pix.to(dev), band_bytes=band_bytes)
    _check_file(png, pix[0].numpy(), bands=bands)


# ---- 3. degenerate histograms ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["zeros", "ones", "ramp"])
def test_degenerate_histograms(backend, kind):
    """2-3 used symbols per band: a near-trivial code, which must still be complete (zlib refuses an incomplete literal code)"""
    dev = use_backend(backend)
    H, W = 12, 40
    if kind == "ramp":
        pix = (torch.arange(W, dtype=torch.int32) * 5).clamp(max=255).to(torch.uint8).view(1, 1, W, 1).expand(1, H, W, 3).contiguous()
    else:
        pix = torch.full((1, H, W, 3), 0 if kind == "zeros" else 255, dtype=torch.uint8)
    for band_bytes in (None, 121 * 5):
        png, = ops.png_encode(pix.to(dev), band_bytes=band_bytes)
        idat = _check_file(png, pix[0].numpy(), bands=_n_bands(H, W, band_bytes or 65535))
        assert set(_blocks(idat)) == {"coded"}


# ---- 4. the length limit ----
def _fibonacci_bytes():
    counts = [1, 1]
    while len(counts) < 22:
        counts.append(counts[-1] + counts[-2])
    buf = np.concatenate([np.full(c, 7 * s + 3, dtype=np.uint8) for s, c in enumerate(counts)])
    np.random.default_rng(4).shuffle(buf)
    assert buf.size == 46367
    return buf


@pytest.mark.parametrize("backend", BACKENDS)
def test_length_limit(backend):
    """22 symbols with Fibonacci counts (and the end of block): an unconstrained Huffman code is 21+ bits deep.  The repaired 15-bit code must inflate
    and stay below 0.40 n (zlib's own length-limited literal-only coding of this shape: 0.328 n).  Measured: 15 319 bytes = 0.3304 n, on the
    emulator and on the MI355X alike (the stream is a function of the bytes alone)."""
    dev = use_backend(backend)
    buf = _fibonacci_bytes()
    z = ops.deflate_bands(torch.from_numpy(buf).to(dev))
    assert zlib.decompress(z) == buf.tobytes()
    print("length limit: %d bytes of %d = %.4f n" % (len(z), buf.size, len(z) / buf.size))
    assert len(z) < 0.40 * buf.size


@pytest.mark.parametrize("backend", BACKENDS)
def test_deflate_bands_many_bands(backend):
    """the bare stream over several bands with a short last one; text-like bytes and a band of noise in the middle (stored)"""
    dev = use_backend(backend)
    rng = np.random.default_rng(6)
    buf = np.concatenate([rng.integers(97, 105, 2500, dtype=np.uint8), rng.integers(0, 256, 1000, dtype=np.uint8), rng.integers(48, 52, 777, dtype=np.uint8)])
    for band_bytes in (1000, 500, 4277, 4276):
        z = ops.deflate_bands(torch.from_numpy(buf).to(dev), band_bytes=band_bytes)
        assert zlib.decompress(z) == buf.tobytes()
        assert len(z) <= buf.size + 5 * -(-buf.size // band_bytes) + 6


# ---- 5. stored fallback ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("band_bytes", [None, 241 * 8])
def test_stored_fallback(backend, band_bytes):
    dev = use_backend(backend)
    H, W = 64, 80
    pix = torch.randint(0, 256, (1, H, W, 3), generator=torch.Generator().manual_seed(52), dtype=torch.uint8)
    bands = _n_bands(H, W, band_bytes or 65535)
    png, = ops.png_encode(pix.to(dev), band_bytes=band_bytes)
    idat = _check_file(png, pix[0].numpy(), bands=bands)
    n = H * (3 * W + 1)
    assert n <= len(png) <= FIXED + bands * (12 + 5) + n
    assert set(_blocks(idat)) == {"stored"}


@pytest.mark.parametrize("backend", BACKENDS)
def test_stored_and_coded_bands_in_one_file(backend):
    dev = use_backend(backend)
    H, W = 64, 80
    pix = _photo(53, H, W)
    pix[:, H // 2:] = torch.randint(0, 256, (1, H // 2, W, 3), generator=torch.Generator().manual_seed(54), dtype=torch.uint8)
    png, = ops.png_encode(pix.to(dev), band_bytes=241 * 8)
    kinds = _blocks(_check_file(png, pix[0].numpy(), bands=8))
    assert kinds[:3] == ["coded"] * 3 and kinds[5:] == ["stored"] * 3
    assert len(png) <= FIXED + 8 * (12 + 5) + H * (3 * W + 1)


# ---- 6. size against Pillow ----
def _pillow_size(a):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a, "RGB").save(f, format="png")
    return f.getbuffer().nbytes


SIZE_CASES = [pytest.param(b, 96, 128, marks=m, id="%s-96x128" % b) for b, m in (("emu", ()), ("gpu", pytest.mark.gpu))] + \
             [pytest.param("gpu", 512, 512, marks=pytest.mark.gpu, id="gpu-512x512"), pytest.param("gpu", 1024, 1536, marks=pytest.mark.gpu, id="gpu-1024x1536")]


@pytest.mark.parametrize("backend,h,w", SIZE_CASES)
def test_size_against_pillow(backend, h, w):
    """Literal-only Huffman coding of Paeth residuals against Pillow's default save (zlib level 6 with LZ77, adaptive filter) on photograph-shaped
    images: the device file may be at most 1.05 x Pillow's.  Measured (device / Pillow): 96 x 128: 26 338 / 26 116 = 1.0085, 512 x 512:
    560 015 / 557 303 = 1.0049, 1024 x 1536: 3 360 614 / 3 344 650 = 1.0048 (profiles/png_bench.json); the fixed 139-byte block header per band is
    most of what the smallest size pays."""
    dev = use_backend(backend)
    pix = _photo(60 + h % 7, h, w)
    png, = ops.png_encode(pix.to(dev))
    _check_file(png, pix[0].numpy(), bands=_n_bands(h, w))
    ref = _pillow_size(pix[0].numpy())
    print("size against Pillow %d x %d: %d / %d = %.4f" % (h, w, len(png), ref, len(png) / ref))
    assert len(png) <= 1.05 * ref


# ---- 7. refusals (no device) ----
def test_refusals(monkeypatch):
    ok = torch.zeros((1, 4, 5, 3), dtype=torch.uint8)
    for bad in (ok.float(), ok[0], torch.zeros((1, 4, 5, 4), dtype=torch.uint8), torch.zeros((1, 4, 3, 5), dtype=torch.uint8).permute(0, 1, 3, 2),
                torch.zeros((1, 8, 5, 3), dtype=torch.uint8)[:, ::2], ok.numpy()):
        with pytest.raises(TypeError):
            ops.png_encode(bad)
    with pytest.raises(ValueError, match="empty"):
        ops.png_encode(torch.zeros((1, 0, 5, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="does not fit a band"):
        ops.png_encode(torch.zeros((1, 1, 21845, 3), dtype=torch.uint8))          # 3W + 1 = 65536
    for band_bytes in (15, 0, -1, 65536):                                       # a row of 5 pixels is 16 bytes
        with pytest.raises(ValueError, match="band_bytes"):
            ops.png_encode(ok, band_bytes=band_bytes)
    for band_bytes in (0, 65536):
        with pytest.raises(ValueError, match="band_bytes"):
            ops.deflate_bands(torch.zeros(8, dtype=torch.uint8), band_bytes=band_bytes)
    with pytest.raises(TypeError):
        ops.deflate_bands(torch.zeros((2, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.deflate_bands(torch.zeros(0, dtype=torch.uint8))

    assert uegan_amd.get_png_encoder() == "pillow" and uegan_amd.set_png_encoder is tester.set_png_encoder
    for name in ("Device", "gpu", "", None):
        with pytest.raises(ValueError, match="unknown PNG encoder"):
            tester.set_png_encoder(name)
    assert tester.get_png_encoder() == "pillow"
    with pytest.raises(ValueError, match="2 paths for 1 images"):
        tester.write_pngs(["a.png", "b.png"], ok)
    monkeypatch.setenv("UEGAN_PNG_ENCODER", "zlib")
    with pytest.raises(ValueError, match="UEGAN_PNG_ENCODER='zlib'"):
        runner.main(["--mode", "test", "--is_test_nima", "False"])
    assert tester.get_png_encoder() == "pillow"


# ---- 8. through the public paths ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_run_test_with_either_encoder(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    _tree(Path("pngsrc"), [(40, 52), (33, 47)])
    _, G = _generator(8, dev)
    res = {}
    try:
        for enc in tester.PNG_ENCODERS:
            tester.set_png_encoder(enc)
            assert tester.get_png_encoder() == enc
            loader = data.get_test_loader("pngsrc", 0, batch_size=2, num_workers=2, device=dev)
            try:
                res[enc] = tester.run_test(G, loader, save_dir="out_" + enc, tag="2.00", compare_dir="cmp_" + enc)
            finally:
                loader.close()
    finally:
        tester.set_png_encoder("pillow")
    assert res["device"] == res["pillow"] and len(res["device"]["psnr"]) == 2
    for kind in ("out_", "cmp_"):
        names = sorted(os.listdir(kind + "pillow"))
        assert len(names) == 2 and sorted(os.listdir(kind + "device")) == names
        for f in names:
            blob = (Path(kind + "device") / f).read_bytes()
            pixels = _png(Path(kind + "pillow") / f)
            _check_file(blob, pixels, bands=1)          # (... so the device's file is none of Pillow's: Pillow writes no 78 01 stream of one IDAT per band)
            assert blob[8 + 25 + 8:8 + 25 + 10] == b"\x78\x01"


@pytest.mark.parametrize("backend", BACKENDS)
def test_command_line_with_device_encoder(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    root = Path("data")
    root.mkdir()
    _make_tree(root, 3, [(40, 52), (36, 36), (61, 33)])
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    mdir = Path("results") / "UEGAN-FiveK" / "models"
    mdir.mkdir(parents=True)
    torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    argv = ["--mode", "test", "--test_img_dir", "data", "--test_img_size", "32", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "3", "--is_test_nima", "False"]
    monkeypatch.setenv("UEGAN_PNG_ENCODER", "device")
    try:
        got = runner.main(argv)
        assert tester.get_png_encoder() == "device"
    finally:
        tester.set_png_encoder("pillow")
    G = G.to(dev) if dev.type != "cpu" else G
    loader = data.get_test_loader("data", 32, 3, False, 2, device=dev)
    try:
        want = tester.run_test(G, loader, save_dir="want", tag="2.00", compare_dir="want_cmp")
    finally:
        loader.close()
    assert got["names"] == want["names"] and got["psnr"] == want["psnr"] and got["ssim"] == want["ssim"]
    out = Path("results") / "UEGAN-FiveK" / "test"
    for sub, ref, width in (("test_results", "want", 32), ("test_compare", "want_cmp", 64)):
        names = sorted(os.listdir(ref))
        assert len(names) == 3 and sorted(os.listdir(out / sub)) == names
        for f in names:
            pixels = _png(Path(ref) / f)
            assert pixels.shape == (32, width, 3)
            _check_file((out / sub / f).read_bytes(), pixels, bands=1)
