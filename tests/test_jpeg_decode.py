"""Baseline JPEG files decoded on the device: csrc/jpeg_decode.hip through codecs.jpeg_info / jpeg_decode / jpeg_decode_coeffs, the loaders with
decode="device", and the command line with UEGAN_INPUT_DECODER=device.

The oracles are independent of the code under test: test_jpeg._parse for the coefficients (a baseline reader in pure Python), Pillow (libjpeg) for
the pixels, and between them jpeg_decode_helpers, a numpy restatement of libjpeg's default path from coefficients to pixels, which test 1 pins
against Pillow before any kernel is compared with either.  The input files are written by Pillow (and by this project's own encoder) in the tests."""
import functools
import io
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import BACKENDS, ROOT, use_backend
from test_jpeg import _crafted, _parse
from test_native import _generator
import jpeg_decode_helpers as JH
from uegan_amd import _lib, codecs, data, ops, runner, tester
import uegan_amd

SENTINEL = 0xA5
FRAME = 64


# ---- 1. the numpy restatement equals Pillow (no device) ----
GRID_SIZES = [(1, 1), (8, 8), (17, 23), (33, 47), (40, 56), (64, 64), (96, 128), (15, 250)]
VARIANTS = [{}, {"optimize": True}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 3}]


@pytest.mark.parametrize("size", GRID_SIZES + [(5, 3), (6, 4), (9, 2)], ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pillow(size):
    """photo-like and noise content x 4:4:4, 4:2:2, 4:2:0 x quality 30, 75, 95, 100 x plain, optimize, restart rows, restart blocks, + a grayscale
    file.  Widths 2, 3 and 4 are added to the issue's grid: libjpeg replicates a chroma plane of at most two columns instead of interpolating."""
    h, w = size
    for kind, make in (("photo", JH.photo_like), ("noise", JH.noise)):
        pix = make(11 * h + w, h, w)
        for ss in JH.SUBSAMPLING:
            for quality in (30, 75, 95, 100):
                for kw in VARIANTS:
                    blob = JH.pillow_jpeg(pix, quality, ss, **kw)
                    assert np.array_equal(JH.decode(blob), JH.pillow_pixels(blob)), (kind, ss, quality, kw)
    blob = JH.pillow_jpeg(JH.photo_like(3, h, w)[..., 1].copy(), 85)
    assert np.array_equal(JH.decode(blob), JH.pillow_pixels(blob))


# ---- 2. what jpeg_info accepts and declines (no device) ----
def _segments(blob):
    """[(marker, start of the marker, end of the segment)] up to and with SOS"""
    out, pos = [], 2
    while True:
        m, n = blob[pos + 1], int.from_bytes(blob[pos + 2:pos + 4], "big")
        out.append((m, pos, pos + 2 + n))
        pos += 2 + n
        if m == 0xda:
            return out


def _patch(blob, marker, offset, value, nth=0):
    """the file with byte `offset` of the nth `marker` segment's payload replaced"""
    seg = [s for s in _segments(blob) if s[0] == marker][nth]
    b = bytearray(blob)
    b[seg[1] + 4 + offset] = value
    return bytes(b)


def _without(blob, marker):
    for m, a, e in _segments(blob):
        if m == marker:
            return blob[:a] + blob[e:]
    raise AssertionError("no marker %x" % marker)


def test_jpeg_info_accepts_and_declines():
    from PIL import Image
    pix = JH.photo_like(1, 40, 56)
    for ss, comps in (("4:4:4", (1, 1)), ("4:2:2", (2, 1)), ("4:2:0", (2, 2))):
        for kw in VARIANTS:
            blob = JH.pillow_jpeg(pix, 90, ss, **kw)
            info = codecs.jpeg_info(blob)
            j = _parse(blob)
            assert (info.height, info.width, info.subsampling, info.restart_interval) == (40, 56, ss, j.dri)
            assert info.components[0][1:3] == comps and [c[:4] for c in info.components] == j.comps
            assert blob[info.scan_offset - 3:info.scan_offset] == b"\x00\x3f\x00" and info.scan_offset + info.scan_length == len(blob)
            assert info.planes == [c.shape[:2] for c in j.coefs] and info.blocks == sum(c.shape[0] * c.shape[1] for c in j.coefs)
            assert [bytes(info.desc.quant[t]) for t in sorted(j.q)] == [bytes(j.q[t]) for t in sorted(j.q)]
            for tc, th, counts, syms in j.dht:
                tab = (info.desc.ac if tc else info.desc.dc)[th]
                assert list(tab.counts) == counts and list(tab.symbols)[:len(syms)] == syms
    gray = JH.pillow_jpeg(pix[..., 0].copy(), 90)
    assert codecs.jpeg_info(gray).subsampling == "gray" and len(codecs.jpeg_info(gray).components) == 1
    base = JH.pillow_jpeg(pix, 90, "4:2:0")
    # libjpeg's colour defaults: JFIF; else Adobe with transform 1; else neither marker and the ids 1, 2, 3
    bare = _without(base, 0xe0)
    assert codecs.jpeg_info(bare).subsampling == "4:2:0"
    adobe = lambda t: bare[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + bare[2:]      # noqa: E731
    assert codecs.jpeg_info(adobe(1)).subsampling == "4:2:0"
    f = io.BytesIO()
    Image.fromarray(pix, "RGB").save(f, format="JPEG", progressive=True)
    progressive = f.getvalue()
    f = io.BytesIO()
    Image.fromarray(np.dstack([pix, pix[..., :1]]), "CMYK").save(f, format="JPEG")
    cmyk = f.getvalue()
    declined = [(progressive, "progressive"), (cmyk, "four components"), (adobe(0), "Adobe colour transform 0"), (adobe(2), "Adobe colour transform 2"),
                (_patch(_patch(bare, 0xc0, 6, 82), 0xda, 1, 82), "component ids"),              # 'R' as the first id, no JFIF, no Adobe
                (_patch(base, 0xc0, 0, 12), "12-bit samples"), (_patch(base, 0xdb, 0, 0x10), "16-bit quantisation table"),
                (_patch(base, 0xc0, 7, 0x12), "sampling factors"), (_patch(base, 0xc0, 7, 0x41), "sampling factors"),
                (_patch(base, 0xc0, 10, 0x21), "sampling factors"),                             # chroma 2x1
                (_patch(base, 0xda, 7, 1), r"\(0, 63, 0\)"), (_patch(base, 0xda, 8, 5), r"\(0, 63, 0\)"), (_patch(base, 0xda, 9, 0x10), r"\(0, 63, 0\)"),
                (_patch(base, 0xda, 0, 1), "several scans"),                                   # a scan of one component: not interleaved
                (_patch(base, 0xda, 2, 0x30), "Huffman table"), (_patch(base, 0xc0, 8, 3), "quantisation table 3"),
                (b"\x89PNG\r\n\x1a\n" + bytes(40), "not a JPEG"), (base[:200], "truncated header"), (base[:2] + b"\xff\xd9", "SOS")]
    for m in (0xc1, 0xc3, 0xc9, 0xca):
        b = bytearray(base)
        b[[s for s in _segments(base) if s[0] == 0xc0][0][1] + 1] = m
        declined.append((bytes(b), "SOF%d" % (m - 0xc0)))
    big = bytearray(base)
    at = [s for s in _segments(base) if s[0] == 0xc0][0][1] + 5
    big[at:at + 4] = (8000).to_bytes(2, "big") + (8000).to_bytes(2, "big")
    declined.append((bytes(big), "pads to"))
    for blob, what in declined:
        with pytest.raises(codecs.JpegUnsupported, match=what):
            codecs.jpeg_info(blob)
    assert issubclass(codecs.JpegUnsupported, ValueError) and ops.jpeg_info is codecs.jpeg_info and ops.JpegUnsupported is codecs.JpegUnsupported


def test_decode_refusals(monkeypatch):
    """a declined file, a bad subseq_bits or max_rounds: before the library is reached"""
    use_backend("emu")

    def reached(*a, **k):
        raise AssertionError("a refusal must come before the library is reached")
    monkeypatch.setattr(_lib, "load", reached)
    ok = JH.pillow_jpeg(JH.photo_like(1, 8, 8), 90)
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(JH.photo_like(1, 8, 8), "RGB").save(f, format="JPEG", progressive=True)
    with pytest.raises(codecs.JpegUnsupported, match="progressive"):
        codecs.jpeg_decode([ok, f.getvalue()])
    for bits in (64, 100, 130, -1, 1 << 21, 1024.0, True):
        with pytest.raises(ValueError, match="subseq_bits"):
            codecs.jpeg_decode([ok], subseq_bits=bits)
    for rounds in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="max_rounds"):
            codecs.jpeg_decode([ok], max_rounds=rounds)
    with pytest.raises(TypeError):
        codecs.jpeg_decode(ok)


# ---- 3. + 4. coefficients equal _parse's, pixels equal Pillow's ----
SIZES = [(1, 1), (8, 8), (17, 23), (33, 47), (40, 300), (96, 128)]


@functools.lru_cache(maxsize=None)
def _files(size):
    """[(what, file, subseq_bits)]: grayscale, 4:4:4, 4:2:2, 4:2:0, each plain, with restart rows (also decoded with one thread per interval), with
    restart intervals of 3 MCUs (they end mid-row) and optimised; the plain file also from noise at quality 100 (the longest codes)"""
    h, w = size
    pix, nz = JH.photo_like(7 * h + w, h, w), JH.noise(h + w, h, w)
    out = []
    for ss in ("gray",) + tuple(JH.SUBSAMPLING):
        src, hard = (pix[..., 1].copy(), nz[..., 1].copy()) if ss == "gray" else (pix, nz)
        args = () if ss == "gray" else (ss,)
        out.append(("%s plain" % ss, JH.pillow_jpeg(src, 90, *args), None))
        out.append(("%s noise" % ss, JH.pillow_jpeg(hard, 100, *args), None))
        out.append(("%s rows" % ss, JH.pillow_jpeg(src, 90, *args, restart_marker_rows=1), None))
        out.append(("%s rows, one thread per interval" % ss, out[-1][1], 0))
        out.append(("%s blocks" % ss, JH.pillow_jpeg(src, 90, *args, restart_marker_blocks=3), None))
        out.append(("%s optimize" % ss, JH.pillow_jpeg(src, 90, *args, optimize=True), None))
    return out


@functools.lru_cache(maxsize=None)
def _parsed(blob):
    return _parse(blob)


@functools.lru_cache(maxsize=None)
def _reference_pixels(blob):
    return torch.from_numpy(JH.pillow_pixels(blob).copy())


def _check_coeffs(blob, dev, subseq_bits=None, max_rounds=None):
    j = _parsed(blob)
    planes, stats = codecs.jpeg_decode_coeffs(blob, dev, subseq_bits, max_rounds)
    assert len(planes) == len(j.coefs)
    for got, want in zip(planes, j.coefs):
        assert got.dtype == torch.int16 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert stats["intervals"] == len(j.rst) + 1 and stats["stream_bytes"] == len(j.unstuffed) and 1 <= stats["rounds"] <= stats["subsequences"]
    return planes, stats


def _decode_framed(blob, dev, subseq_bits=None, max_rounds=None):
    """through jpeg_decode_into, into a buffer framed by sentinel bytes -> (the pixels [h, w, 3], the frame is intact, the stats or the error)"""
    info = codecs.jpeg_info(blob)
    n = info.height * info.width * 3
    buf = torch.full((FRAME + n + FRAME,), SENTINEL, dtype=torch.uint8).to(dev)
    assert buf.data_ptr() % 16 == 0
    f = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    try:
        res = codecs.jpeg_decode_into(info, f, buf[FRAME:FRAME + n], subseq_bits, max_rounds)
    except codecs.JpegDecodeError as e:
        res = e
    host = buf.cpu()
    intact = bool((host[:FRAME] == SENTINEL).all()) and bool((host[FRAME + n:] == SENTINEL).all())
    return host[FRAME:FRAME + n].view(info.height, info.width, 3), intact, res


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_coefficients_equal_parse(backend, size):
    dev = use_backend(backend)
    for what, blob, bits in _files(size):
        try:
            _check_coeffs(blob, dev, bits)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_pixels_equal_pillow(backend, size):
    dev = use_backend(backend)
    for what, blob, bits in _files(size):
        got, intact, res = _decode_framed(blob, dev, bits)
        assert isinstance(res, dict), (what, res)
        assert intact, what
        assert torch.equal(got, _reference_pixels(blob)), what
    blobs = [b for _, b, bits in _files(size) if bits is None][:4]
    many = codecs.jpeg_decode(blobs, dev)
    assert len(many) == 4
    for t, blob in zip(many, blobs):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (1, size[0], size[1], 3) and torch.equal(t[0].cpu(), _reference_pixels(blob))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", ["4:4:4", "4:2:0"])
def test_own_files(backend, ss):
    """this project's encoder writes one restart interval per MCU row; standard and optimised tables.  The decoded coefficients are also the ones
    the encoder's first stage computed from the pixels."""
    dev = use_backend(backend)
    pix = torch.from_numpy(JH.photo_like(21, 72, 40))[None].to(dev)
    want = codecs.jpeg_coeffs(pix, 90, ss)
    for optimize in (False, True):
        blob, = codecs.jpeg_encode(pix, 90, ss, optimize=optimize)
        planes, _ = _check_coeffs(blob, dev)
        for got, w in zip(planes, want):
            assert torch.equal(got, w[0])
        got, intact, res = _decode_framed(blob, dev)
        assert isinstance(res, dict) and intact and torch.equal(got, _reference_pixels(blob))


# ---- 5. synchronisation regimes: 96 x 128, no restart markers, 128-bit sub-sequences ----
def _regime(kind):
    if kind == "photo":          # several hundred sub-sequences, so the rounds cross thread blocks of 256
        return JH.pillow_jpeg(JH.photo_like(5, 96, 128), 95, "4:4:4")
    if kind == "noise":          # blocks of several hundred bits: a block spans three or more sub-sequences
        return JH.pillow_jpeg(JH.noise(6, 96, 128), 100, "4:4:4")
    if kind == "flat":           # dozens of blocks per sub-sequence
        return JH.pillow_jpeg(np.full((96, 128, 3), 100, dtype=np.uint8), 75, "4:2:0")
    if kind == "flat, own tables":
        # optimize=True gives every table of a flat image one 1-bit code: behind the first block every block is the two bits 00 whatever its
        # component, so a decoder that starts at the wrong block of the MCU stays there for ever: no synchronisation before the truth arrives
        return JH.pillow_jpeg(np.full((96, 128, 3), 100, dtype=np.uint8), 75, "4:4:4", optimize=True)
    raise ValueError(kind)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["photo", "noise", "flat", "flat, own tables"])
def test_synchronisation_regimes(backend, kind):
    """Measured on the emulator (rounds of sub-sequences at 128 bits; at 1024): photo 20 of 807; 3 of 101.  noise 437 of 3132; 55 of 392.
    flat 2 of 13; 2 of 2 -- with the standard tables a decoder at the wrong block of the MCU reads luma blocks with chroma tables and wanders until
    it meets the true state, so this file does synchronise early.  flat, own tables 10 of 10: the case without early synchronisation."""
    dev = use_backend(backend)
    blob = _regime(kind)
    j = _parsed(blob)
    assert j.dri == 0
    fine, stats = _check_coeffs(blob, dev, 128, 1 << 20)
    coarse, stats1024 = _check_coeffs(blob, dev, 1024, 1 << 20)
    for a, b in zip(fine, coarse):
        assert torch.equal(a, b)
    n, rounds = stats["subsequences"], stats["rounds"]
    print("regime %s: %d rounds of %d sub-sequences at 128 bits, %d of %d at 1024" % (kind, rounds, n, stats1024["rounds"], stats1024["subsequences"]))
    assert n == -(-8 * len(j.unstuffed) // 128) and rounds <= n and stats1024["rounds"] <= stats1024["subsequences"]
    blocks = sum(c.shape[0] * c.shape[1] for c in j.coefs)
    if kind == "photo":
        assert n > 2 * 256 and rounds > 1
    elif kind == "noise":
        assert 8 * len(j.unstuffed) / blocks > 2 * 128          # the mean block is longer than two sub-sequences
        assert rounds > 4
        with pytest.raises(codecs.JpegDecodeError, match="not synchronised") as e:
            codecs.jpeg_decode([blob], dev, subseq_bits=128, max_rounds=4)
        assert e.value.status == codecs.JPEG_E_DESYNC
    elif kind == "flat":
        assert blocks / n > 12
    else:
        # round r makes sub-sequence r right and no later one (64 blocks per sub-sequence, 3 per MCU: the block phase at a boundary is never the
        # blind start's for two boundaries in a row), so the last change comes in round n - 1, or n - 2 where the last blind start happens to be right
        assert blocks / n > 24 and n - 1 <= rounds <= n
    got, intact, res = _decode_framed(blob, dev, 128, 1 << 20)
    assert isinstance(res, dict) and intact and torch.equal(got, _reference_pixels(blob))


# ---- 6. stuffing ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_stuffed_bytes(backend):
    """FF 00 pairs in the file; in the Pillow file of seed 0 (no restart markers) four of them end exactly at a 128-bit sub-sequence boundary of the
    plain stream: the FF is the last byte of a sub-sequence, the 00 that followed it in the file would have been the first of the next"""
    dev = use_backend(backend)
    own, = codecs.jpeg_encode(_crafted("stuffing").to(dev), 100, "4:4:4")
    pil = JH.pillow_jpeg(JH.noise(0, 32, 32), 100, "4:4:4")
    for blob in (own, pil):
        j = _parsed(blob)
        assert b"\xff" in j.unstuffed and blob.count(b"\xff\x00", codecs.jpeg_info(blob).scan_offset) >= j.unstuffed.count(b"\xff") > 0
        for bits in (128, 1024, 0):
            _check_coeffs(blob, dev, bits)
            got, intact, res = _decode_framed(blob, dev, bits)
            assert isinstance(res, dict) and intact and torch.equal(got, _reference_pixels(blob))
    at = [i for i, b in enumerate(_parsed(pil).unstuffed) if b == 0xff and i % 16 == 15]
    assert len(at) >= 1, at


# ---- 7. malformed streams: the emulator only (a defect shows as sentinel damage or a Python error on the CPU) ----
def _malformed(kind):
    pix = JH.photo_like(9, 40, 56)
    good = JH.pillow_jpeg(pix, 90, "4:2:0", restart_marker_rows=1)
    info = codecs.jpeg_info(good)
    if kind == "cut":
        return good[:info.scan_offset + info.scan_length // 2]
    if kind == "cut, no restart markers":
        good = JH.pillow_jpeg(JH.noise(9, 40, 56), 100, "4:4:4")
        info = codecs.jpeg_info(good)
        return good[:info.scan_offset + info.scan_length // 2]
    if kind == "random":
        rng = np.random.default_rng(4)
        return good[:info.scan_offset] + rng.integers(0, 256, size=info.scan_length, dtype=np.uint8).tobytes()
    if kind == "random, no markers":
        rng = np.random.default_rng(5)
        plain = JH.pillow_jpeg(pix, 90, "4:4:4")
        i = codecs.jpeg_info(plain)
        return plain[:i.scan_offset] + rng.integers(0, 255, size=i.scan_length, dtype=np.uint8).tobytes()
    if kind == "rst removed":
        at = good.index(b"\xff\xd1", info.scan_offset)
        return good[:at] + good[at + 2:]
    if kind == "rst out of sequence":
        at = good.index(b"\xff\xd1", info.scan_offset)
        return good[:at] + b"\xff\xd3" + good[at + 2:]
    if kind == "undefined code":
        # an optimised file's tables hold exactly the symbols that occur; the last AC luma symbol (the longest code) is taken out of its DHT
        opt = JH.pillow_jpeg(JH.noise(3, 40, 56), 95, "4:4:4", optimize=True)
        for m, a, e in _segments(opt):
            if m == 0xc4 and opt[a + 4] == 0x10:
                body = bytearray(opt[a + 4:e])
                last = max(i for i in range(16) if body[1 + i])
                body[1 + last] -= 1
                body = body[:-1]
                return opt[:a] + b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + bytes(body) + opt[e:]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["cut", "cut, no restart markers", "random", "random, no markers", "rst removed", "rst out of sequence", "undefined code"])
def test_malformed_streams(kind):
    dev = use_backend("emu")
    blob = _malformed(kind)
    for bits in (128, 1024, 0):
        _, intact, res = _decode_framed(blob, dev, bits)
        assert isinstance(res, codecs.JpegDecodeError) and res.status == codecs.JPEG_E_STREAM, (kind, bits, res)
        assert intact, (kind, bits)
        with pytest.raises(codecs.JpegDecodeError):
            codecs.jpeg_decode_coeffs(blob, dev, bits)
    with pytest.raises(codecs.JpegDecodeError):
        codecs.jpeg_decode([blob], dev)


# ---- 8. the loaders ----
def _jpeg_tree(root):
    """four pairs: 4:4:4, 4:2:0 with restart markers, 4:2:2 optimised, grayscale; one raw file is a PNG and one label file a progressive JPEG"""
    from PIL import Image
    for d in ("label", "raw"):
        (root / d).mkdir(parents=True)
    spec = [((40, 52), "4:4:4", {}), ((33, 47), "4:2:0", {"restart_marker_rows": 1}), ((64, 64), "4:2:2", {"optimize": True}), ((36, 36), "gray", {})]
    for i, ((h, w), ss, kw) in enumerate(spec):
        for d in ("label", "raw"):
            a = JH.photo_like(40 + i + 10 * (d == "raw"), h, w)
            path = root / d / ("im%02d.jpg" % i)
            if (d, i) == ("raw", 0):
                Image.fromarray(a, "RGB").save(root / d / "im00.png")
            elif (d, i) == ("label", 1):
                Image.fromarray(a, "RGB").save(path, format="JPEG", quality=90, progressive=True)
            elif ss == "gray":
                path.write_bytes(JH.pillow_jpeg(a[..., 1].copy(), 90))
            else:
                path.write_bytes(JH.pillow_jpeg(a, 90, ss, **kw))
    return [s[0] for s in spec]


@pytest.mark.parametrize("backend", BACKENDS)
def test_loaders_with_either_decoder(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    monkeypatch.chdir(tmp_path)
    sizes = _jpeg_tree(Path("src"))
    made = {"train": lambda dec: data.get_train_loader("src", 32, 16, batch_size=2, shuffle=True, num_workers=2, device=dev,
                                                       generator=torch.Generator().manual_seed(5), decode=dec),
            "test": lambda dec: data.get_test_loader("src", 64, batch_size=2, num_workers=2, device=dev, decode=dec),
            "native": lambda dec: data.get_test_loader("src", 0, batch_size=3, num_workers=2, device=dev, decode=dec)}
    for mode, make in made.items():
        got = {}
        for dec in ("host", "device"):
            loader = make(dec)
            try:
                assert loader.decode == dec
                passes = []
                for _ in range(2):
                    passes.append([(b.img_exp, b.img_raw, b.img_name) for b in loader])
                    assert loader.fallbacks == (2 if dec == "device" else 0), (mode, dec)
                assert loader.fallbacks_total == (4 if dec == "device" else 0)
                got[dec] = passes
            finally:
                loader.close()
        for ph, pd in zip(got["host"], got["device"]):
            assert len(ph) == len(pd) == 2
            for (he, hr, hn), (de, dr, dn) in zip(ph, pd):
                assert hn == dn
                if mode == "native":
                    assert len(he) == len(de) and all(torch.equal(a, b) for a, b in zip(list(he) + list(hr), list(de) + list(dr)))
                    assert all(t.data_ptr() % 16 == 0 for t in list(de) + list(dr))
                else:
                    assert torch.equal(he, de) and torch.equal(hr, dr)
        if mode == "native":
            assert sorted(tuple(t.shape[1:3]) for b in got["device"][0] for t in b[1]) == sorted(sizes)          # (a folder's listing order is the file system's)
    with pytest.raises(ValueError, match="unknown input decoder 'gpu'"):
        data.get_test_loader("src", 64, decode="gpu")
    with pytest.raises(ValueError, match="workers must be 'thread'"):
        data.get_test_loader("src", 64, decode="device", workers="process")


def test_input_decoder_selection(monkeypatch):
    use_backend("emu")
    assert data.get_input_decoder() == "host" and uegan_amd.set_input_decoder is data.set_input_decoder
    with pytest.raises(ValueError, match="unknown input decoder 'pillow'"):
        data.set_input_decoder("pillow")
    argv = ["--mode", "test", "--is_test_nima", "False"]
    for bad in ("gpu", "Device", ""):
        monkeypatch.setenv("UEGAN_INPUT_DECODER", bad)
        with pytest.raises(ValueError, match="UEGAN_INPUT_DECODER=%r" % bad):
            runner.main(argv)
        assert data.get_input_decoder() == "host"
    try:
        assert data.set_input_decoder("device") == "host"
        assert data.DeviceLoader(data.ReferenceDataset(os.path.join(ROOT, "tests", "golden")), 1, train=False).decode == "device"
    finally:
        data.set_input_decoder("host")


# ---- 9. end to end ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_run_test_with_either_decoder(backend, tmp_path, monkeypatch):
    """native-size inference on a tree of JPEG files: the same metrics and the same result files whoever decoded the inputs"""
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    for d in ("label", "raw"):
        Path("src", d).mkdir(parents=True)
    for i, ((h, w), ss, kw) in enumerate([((40, 52), "4:2:0", {}), ((33, 47), "4:4:4", {"restart_marker_rows": 1})]):
        for d in ("label", "raw"):
            (Path("src", d) / ("im%02d.jpg" % i)).write_bytes(JH.pillow_jpeg(JH.photo_like(60 + i + 10 * (d == "raw"), h, w), 92, ss, **kw))
    _, G = _generator(8, dev)
    res = {}
    for dec in data.INPUT_DECODERS:
        loader = data.get_test_loader("src", 0, batch_size=2, num_workers=2, device=dev, decode=dec)
        try:
            res[dec] = tester.run_test(G, loader, save_dir="out_" + dec, tag="2.00", compare_dir="cmp_" + dec)
            assert loader.fallbacks == 0
        finally:
            loader.close()
    assert res["device"] == res["host"] and len(res["host"]["psnr"]) == 2
    for kind in ("out_", "cmp_"):
        names = sorted(os.listdir(kind + "host"))
        assert len(names) == 2 and sorted(os.listdir(kind + "device")) == names
        for n in names:
            assert (Path(kind + "host") / n).read_bytes() == (Path(kind + "device") / n).read_bytes()


@pytest.mark.parametrize("backend", BACKENDS)
def test_command_line_with_device_decoder(backend, tmp_path, monkeypatch):
    """python -m uegan_amd --mode test --test_img_size 0 on a folder of baseline JPEG files: the same metrics file and result files with
    UEGAN_INPUT_DECODER=device as without it"""
    from uegan_amd import models
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    for d in ("exp", "raw"):
        Path("data", d).mkdir(parents=True)
    for i, ((h, w), ss) in enumerate([((40, 52), "4:2:0"), ((36, 36), "4:2:2")]):
        for d in ("exp", "raw"):
            (Path("data", d) / ("im%02d.jpg" % i)).write_bytes(JH.pillow_jpeg(JH.photo_like(80 + i + 10 * (d == "raw"), h, w), 92, ss))
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    for save_root in ("results", "results_device"):
        mdir = Path(save_root) / "UEGAN-FiveK" / "models"
        mdir.mkdir(parents=True)
        torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    argv = ["--mode", "test", "--test_img_dir", "data", "--test_img_size", "0", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "2", "--is_test_nima", "False"]
    for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_PNG_ENCODER", "UEGAN_INPUT_DECODER"):
        monkeypatch.delenv(k, raising=False)
    runner.main(argv)
    assert data.get_input_decoder() == "host"
    monkeypatch.setenv("UEGAN_INPUT_DECODER", "device")
    try:
        runner.main(argv + ["--save_root_dir", "results_device"])
        assert data.get_input_decoder() == "device"
    finally:
        data.set_input_decoder("host")
    out = []
    for save_root in ("results", "results_device"):
        base = Path(save_root) / "UEGAN-FiveK" / "test"
        m = json.loads((base / "test_metrics.json").read_text())
        m.pop("checkpoint")
        files = {str(p.relative_to(base)): p.read_bytes() for p in sorted(base.rglob("*.png"))}
        out.append((m, files))
    assert out[0] == out[1] and len(out[0][0]["names"]) == 2 and len(out[0][1]) == 4


# ---- 10. plumbing ----
def test_abi_symbols():
    src = open(os.path.join(ROOT, "include", "uegan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = {"uegan_jpeg_decode_workspace_bytes": 2, "uegan_jpeg_decode": 9, "uegan_jpeg_decode_coeffs": 8}
    for name, nargs in names.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "UEGAN_E_JPEG_DESYNC = -4" in src and "UEGAN_E_JPEG_STREAM = -5" in src
    assert (codecs.JPEG_E_DESYNC, codecs.JPEG_E_STREAM) == (-4, -5)
    use_backend("emu")
    assert all(hasattr(ops.lib(), name) for name in names)
    assert ops.lib().uegan_version() == 105
    info = codecs.jpeg_info(JH.pillow_jpeg(JH.photo_like(1, 40, 56), 90, "4:2:0"))
    import ctypes
    for bits in (0, 128, 1024):
        assert ops.lib().uegan_jpeg_decode_workspace_bytes(ctypes.byref(info.desc), bits) > 0
    for bits in (64, 130, -8):
        assert ops.lib().uegan_jpeg_decode_workspace_bytes(ctypes.byref(info.desc), bits) == 0
