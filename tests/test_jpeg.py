"""Baseline JPEG files encoded on the device: csrc/jpeg.hip through ops.jpeg_encode / jpeg_sizes / jpeg_coeffs / jpeg_qtables, tester.write_images with
set_image_format, and the command line with UEGAN_IMAGE_FORMAT=jpeg.

The oracles are independent of the code under test: Pillow's decoder (libjpeg), a baseline-JPEG reader in pure Python below (markers, Huffman
decoders built from the file's own DHT, stuffing, the RST sequence, per-block zigzag coefficients and the symbols that coded them), and an fp64
numpy restatement of stage 1 (colour conversion, edge replication, 4:2:0 means, DCT, quantisation) written from the standard."""
import io
import json
import os
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import BACKENDS, ROOT, use_backend
from test_data import _make_tree
from test_native import _generator, _photo, _pixels, _tree
from uegan_amd import _lib, data, models, ops, runner, tester
import uegan_amd

SS = {"4:4:4": 0, "4:2:0": 2}          # name -> Pillow's subsampling code
SENTINEL = 0xA5
HEADER = 629
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
EOB, ZRL = 0x00, 0xF0


# ---- a baseline JPEG reader ----
class Jpeg:
    """markers: [(marker, payload)] up to SOS; q: {id: 64 ints, zigzag}; comps: [(id, h, v, tq)]; huff: {(class, id): {(length, code): symbol}} with
    dht: [(class, id, counts, symbols)] in file order; dri; scan: SOS payload; rst: the restart indices met; coefs: per component int array
    [block rows, block cols, 64] (zigzag); symbols: per component, per block (scan order) [DC size, AC run/size symbols ...]; unstuffed: the entropy
    bytes of all intervals without stuffing and markers; end: the position behind EOI"""


def _parse(blob):
    j = Jpeg()
    assert blob[:2] == b"\xff\xd8"
    j.markers, j.q, j.huff, j.dht, j.dri = [], {}, {}, [], 0
    pos = 2
    while True:
        assert blob[pos] == 0xff, pos
        m = blob[pos + 1]
        n = int.from_bytes(blob[pos + 2:pos + 4], "big")
        body = blob[pos + 4:pos + 2 + n]
        j.markers.append((m, body))
        pos += 2 + n
        if m == 0xdb:
            at = 0
            while at < len(body):
                assert body[at] >> 4 == 0          # 8-bit precision
                j.q[body[at] & 15] = list(body[at + 1:at + 65])
                at += 65
        elif m == 0xc0:
            j.precision, j.H, j.W, nc = body[0], int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            j.comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nc)]
        elif m == 0xc4:
            at = 0
            while at < len(body):
                tc, th = body[at] >> 4, body[at] & 15
                counts = list(body[at + 1:at + 17])
                syms = list(body[at + 17:at + 17 + sum(counts)])
                at += 17 + sum(counts)
                j.dht.append((tc, th, counts, syms))
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = syms[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                j.huff[(tc, th)] = table
        elif m == 0xdd:
            j.dri = int.from_bytes(body, "big")
        elif m == 0xda:
            j.scan = body
            break
    # entropy data: intervals between RSTm, up to EOI
    intervals, cur, j.rst = [], bytearray(), []
    while True:
        b = blob[pos]
        if b != 0xff:
            cur.append(b)
            pos += 1
            continue
        nxt = blob[pos + 1]
        if nxt == 0:
            cur.append(0xff)
        elif 0xd0 <= nxt <= 0xd7:
            j.rst.append(nxt - 0xd0)
            intervals.append(bytes(cur))
            cur = bytearray()
        else:
            assert nxt == 0xd9, hex(nxt)
            intervals.append(bytes(cur))
            pos += 2
            break
        pos += 2
    j.end = pos
    j.unstuffed = b"".join(intervals)
    hmax, vmax = max(c[1] for c in j.comps), max(c[2] for c in j.comps)
    mcux, mcuy = -(-j.W // (8 * hmax)), -(-j.H // (8 * vmax))
    per = j.dri or mcux * mcuy
    assert len(intervals) == -(-mcux * mcuy // per)
    ns = j.scan[0]
    tabs = {j.scan[1 + 2 * i]: (j.scan[2 + 2 * i] >> 4, j.scan[2 + 2 * i] & 15) for i in range(ns)}
    assert ns == len(j.comps) and tuple(j.scan[1 + 2 * ns:]) == (0, 63, 0)
    j.coefs = [np.zeros((mcuy * v, mcux * h, 64), dtype=np.int64) for _, h, v, _ in j.comps]
    j.symbols = [[] for _ in j.comps]
    mcu = 0
    for data_ in intervals:
        bits = "".join(format(v, "08b") for v in data_)
        at = 0
        pred = [0] * len(j.comps)

        def sym(table):
            nonlocal at
            code = 0
            for length in range(1, 17):
                code = (code << 1) | int(bits[at + length - 1])
                if (length, code) in table:
                    at += length
                    return table[(length, code)]
            raise AssertionError("no code at bit %d" % at)

        def magnitude(size):
            nonlocal at
            if size == 0:
                return 0
            v = int(bits[at:at + size], 2)
            at += size
            return v if v >> (size - 1) else v - (1 << size) + 1

        for _ in range(min(per, mcux * mcuy - mcu)):
            my, mx = divmod(mcu, mcux)
            for ci, (cid, h, v, _) in enumerate(j.comps):
                td, ta = tabs[cid]
                for by in range(v):
                    for bx in range(h):
                        blk = j.coefs[ci][my * v + by, mx * h + bx]
                        s = sym(j.huff[(0, td)])
                        rec = [s]
                        pred[ci] += magnitude(s)
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = sym(j.huff[(1, ta)])
                            rec.append(rs)
                            if rs == EOB:
                                break
                            if rs == ZRL:
                                k += 16
                                continue
                            k += rs >> 4
                            assert k < 64
                            blk[k] = magnitude(rs & 15)
                            k += 1
                        assert k <= 64
                        j.symbols[ci].append(rec)
            mcu += 1
        assert len(bits) - at < 8 and set(bits[at:]) <= {"1"}, "an interval ends with at most 7 padding 1-bits"
    assert mcu == mcux * mcuy
    return j


# ---- stage 1 in fp64 ----
_n = np.arange(8)
DCT = 0.5 * np.cos((2 * _n[None, :] + 1) * _n[:, None] * np.pi / 16)          # DCT[k, n]
DCT[0] /= np.sqrt(2.0)
NATURAL_OF = np.array(ZIGZAG)                                                 # zigzag position -> natural index


def _planes(pixels, ss):
    """uint8 [H,W,3] -> the level-shifted Y, Cb, Cr planes in fp64, edges replicated to whole MCUs, chroma averaged 2 x 2 for 4:2:0"""
    H, W, _ = pixels.shape
    mcu = 16 if ss == "4:2:0" else 8
    Hp, Wp = -(-H // mcu) * mcu, -(-W // mcu) * mcu
    p = np.pad(pixels.astype(np.float64), ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb, cr = (b - y) / 1.772, (r - y) / 1.402
    if ss == "4:2:0":
        cb, cr = (x.reshape(Hp // 2, 2, Wp // 2, 2).mean(axis=(1, 3)) for x in (cb, cr))
    return [y - 128.0, cb, cr]


def _qnatural(qzz):
    q = np.zeros(64)
    q[NATURAL_OF] = np.asarray(qzz, dtype=np.float64)
    return q.reshape(8, 8)


def _ratios(pixels, quality, ss):
    """per component [block rows, block cols, 64] (zigzag): the fp64 coefficient / its table entry, before rounding"""
    q = ops.jpeg_qtables(quality)
    out = []
    for ci, plane in enumerate(_planes(pixels, ss)):
        h, w = plane.shape
        blocks = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        coef = DCT @ blocks @ DCT.T
        r = coef / _qnatural(q[:64] if ci == 0 else q[64:])
        out.append(r.reshape(h // 8, w // 8, 64)[..., NATURAL_OF])
    return out


def _half_away(r):
    return (np.sign(r) * np.floor(np.abs(r) + 0.5)).astype(np.int64)


def _reconstruct(coefs, q, H, W):
    """4:4:4: zigzag coefficients per component -> dequantise, inverse DCT, YCbCr -> RGB, round, clamp -> uint8 [H,W,3]"""
    planes = []
    for ci, c in enumerate(coefs):
        nat = np.zeros(c.shape, dtype=np.float64)
        nat[..., NATURAL_OF] = c
        f = nat.reshape(c.shape[0], c.shape[1], 8, 8) * _qnatural(q[0] if ci == 0 else q[1])
        x = DCT.T @ f @ DCT
        planes.append(x.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8)[:H, :W])
    y, cb, cr = planes[0] + 128.0, planes[1], planes[2]
    rgb = np.stack([y + 1.402 * cr, y - (0.114 * 1.772 * cb + 0.299 * 1.402 * cr) / 0.587, y + 1.772 * cb], axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


# ---- checks shared by the cases ----
def _pillow(blob):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with Image.open(io.BytesIO(blob)) as im:
            im.load()
            assert im.format == "JPEG" and im.mode == "RGB"
            return np.array(im), {k: list(v) for k, v in im.quantization.items()}


def _check_file(blob, H, W, quality, ss):
    """the layout of include/uegan_hip.h, marker by marker -> the parsed file"""
    pixels, _ = _pillow(blob)
    assert pixels.shape == (H, W, 3)
    j = _parse(blob)
    assert j.end == len(blob)
    q = ops.jpeg_qtables(quality)
    mcu = 16 if ss == "4:2:0" else 8
    mcux, mcuy = -(-W // mcu), -(-H // mcu)
    assert [m for m, _ in j.markers] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
    assert j.markers[0][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert j.markers[1][1] == bytes([0] + q[:64]) and j.markers[2][1] == bytes([1] + q[64:])
    assert (j.precision, j.H, j.W) == (8, H, W)
    assert j.comps == [(1, 2, 2, 0) if ss == "4:2:0" else (1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert [(tc, th) for tc, th, _, _ in j.dht] == [(0, 0), (1, 0), (0, 1), (1, 1)]
    assert j.dht == _standard_dht()
    assert j.dri == mcux
    assert j.scan == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert j.rst == [k % 8 for k in range(mcuy - 1)]
    assert sum(len(body) + 4 for _, body in j.markers) + 2 == HEADER
    return j


_dht = []


def _standard_dht():
    """the Annex K.3 tables as Pillow (libjpeg) writes them into a file that is not optimised"""
    if not _dht:
        from PIL import Image
        f = io.BytesIO()
        Image.new("RGB", (8, 8)).save(f, format="JPEG", optimize=False)
        _dht.extend(sorted(_parse(f.getvalue()).dht, key=lambda t: (t[1], t[0])))
        assert [len(t[3]) for t in _dht] == [12, 162, 12, 162]
    return _dht


def _encode(pix, dev, quality, ss):
    """through the one-call path into a sentinel-filled buffer, and through the two-step path: the same files; nothing behind a file is touched"""
    B, H, W, _ = pix.shape
    cap = ops.jpeg_capacity(H, W, ss)
    out = torch.full((B, cap + 32), SENTINEL, dtype=torch.uint8).to(dev)
    x = pix.to(dev)
    files = ops.jpeg_encode(x, quality, ss, out=out)
    host = out.cpu().numpy()
    for b, f in enumerate(files):
        assert HEADER < len(f) <= cap
        assert bytes(host[b, :len(f)]) == f and (host[b, len(f):] == SENTINEL).all()
    assert ops.jpeg_encode(x, quality, ss) == files
    assert ops.jpeg_sizes(x, quality, ss) == [len(f) for f in files]
    return files


def _check_lossless(j, pix_dev, b, quality, ss):
    """the coefficients decoded from the file are those of stage 1, exactly"""
    want = ops.jpeg_coeffs(pix_dev, quality, ss)
    for ci in range(3):
        assert np.array_equal(j.coefs[ci], want[ci][b].cpu().numpy().astype(np.int64)), ci
    return want


# ---- 1. + 2. structure and lossless entropy coding at the smallest shapes ----
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (1, 8, 8), (1, 16, 16), (1, 17, 33), (1, 72, 40), (2, 40, 52), (1, 144, 24)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", list(SS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_structure_and_lossless(backend, shape, ss):
    """(72, 40) at 4:4:4 and (144, 24) at 4:2:0 have 9 MCU rows: RST wraps past 7.  B = 2: other content per image, so other sizes."""
    dev = use_backend(backend)
    B, H, W = shape
    pix = _pixels(80 + H, B, H, W)
    if B == 2:
        pix[1] = _photo(81, H, W)[0]
    files = _encode(pix, dev, 90, ss)
    assert len(files) == B and all(isinstance(f, bytes) for f in files)
    for b in range(B):
        j = _check_file(files[b], H, W, 90, ss)
        _check_lossless(j, pix.to(dev), b, 90, ss)
    if B == 2:
        assert len(files[0]) != len(files[1])


# ---- 2. crafted streams, quality 100 ----
ZRL_AMPLITUDE = 400.0


def _zrl_block(amplitude):
    """An 8 x 8 RGB block whose Y plane is 128 + the inverse DCT of `amplitude` at zigzag index 63 alone.  Grey pixels would round every sample by up
    to half a level, which leaves coefficients of +-1 all over the block at quality 100; so each pixel takes the R, G, B within two levels of its
    grey value whose 0.299 R + 0.587 G + 0.114 B comes closest to the sample (within 0.02 levels).  Cb and Cr then are small and not zero."""
    f = np.zeros((8, 8))
    f[7, 7] = amplitude
    target = DCT.T @ f @ DCT + 128.0
    d = np.arange(-2, 3)
    offs = np.stack(np.meshgrid(d, d, d, indexing="ij"), axis=-1).reshape(-1, 3)
    lum = offs @ np.array([0.299, 0.587, 0.114])
    out = np.zeros((8, 8, 3), dtype=np.uint8)
    for y in range(8):
        for x in range(8):
            base = int(np.floor(target[y, x] + 0.5))
            out[y, x] = base + offs[np.argmin(np.abs(base + lum - target[y, x]))]
    return out


def _crafted(kind):
    if kind == "stuffing":
        return torch.randint(0, 256, (1, 32, 32, 3), generator=torch.Generator().manual_seed(90), dtype=torch.uint8)
    if kind == "largest":
        tiles = (np.add.outer(np.arange(4), np.arange(6)) % 2 * 255).astype(np.uint8)
        return torch.from_numpy(np.kron(tiles, np.ones((8, 8), dtype=np.uint8))[None, :, :, None].repeat(3, axis=3).copy())
    if kind == "zrl":
        return torch.from_numpy(_zrl_block(ZRL_AMPLITUDE)[None])
    if kind == "eob":
        return torch.tensor([100, 150, 200], dtype=torch.uint8).view(1, 1, 1, 3).expand(1, 16, 24, 3).contiguous()
    if kind == "full":
        return torch.randint(0, 256, (1, 8, 16, 3), generator=torch.Generator().manual_seed(91), dtype=torch.uint8)
    raise ValueError(kind)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["stuffing", "largest", "zrl", "eob", "full"])
def test_crafted_streams(backend, kind):
    dev = use_backend(backend)
    pix = _crafted(kind)
    _, H, W, _ = pix.shape
    for ss in SS:
        if kind == "zrl" and ss == "4:2:0":
            continue                                      # (one 8 x 8 block is a quarter of a 4:2:0 MCU: its replicated rest is another stream)
        f, = _encode(pix, dev, 100, ss)
        j = _check_file(f, H, W, 100, ss)
        _check_lossless(j, pix.to(dev), 0, 100, ss)
        blocks = [(ci, rec, blk) for ci in range(3) for rec, blk in zip(j.symbols[ci], _scan_blocks(j, ci))]
        if kind == "stuffing":
            assert b"\xff" in j.unstuffed and b"\xff\x00" in f[HEADER:]
            assert f[HEADER:].count(b"\xff\x00") == j.unstuffed.count(b"\xff")
        elif kind == "largest":
            assert max(rec[0] for _, rec, _ in blocks) == 11
        elif kind == "zrl":
            r = _ratios(pix[0].numpy(), 100, ss)[0][0, 0]
            assert np.abs(r[1:63]).max() < 0.25 and abs(r[63] - ZRL_AMPLITUDE) < 0.25          # (the fixture is what it claims to be)
            rec = j.symbols[0][0]
            assert rec[1:4] == [ZRL, ZRL, ZRL] and rec[-1] != EOB and len(rec) == 5 and j.coefs[0][0, 0, 63] != 0
        elif kind == "eob":
            assert all(rec[1:] == [EOB] for _, rec, _ in blocks)
        else:
            full = [rec for _, rec, blk in blocks if blk[63] != 0]
            assert full and all(rec[-1] != EOB for rec in full)
            assert all(rec[-1] == EOB for _, rec, blk in blocks if blk[63] == 0)


def _scan_blocks(j, ci):
    """component ci's blocks in the order the scan codes them (the order of Jpeg.symbols)"""
    _, h, v, _ = j.comps[ci]
    c = j.coefs[ci]
    rows, cols = c.shape[0] // v, c.shape[1] // h
    return [c[my * v + by, mx * h + bx] for my in range(rows) for mx in range(cols) for by in range(v) for bx in range(h)]


# ---- 3. arithmetic ----
@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_qtables_equal_pillows(quality):
    """Image.quantization of Pillow 12 is in natural order (Pillow undoes the zigzag of the DQT segment since 8.3); uegan_jpeg_qtables is in zigzag
    order, as the segment holds it"""
    from PIL import Image
    use_backend("emu")
    f = io.BytesIO()
    Image.new("RGB", (8, 8)).save(f, format="JPEG", quality=quality)
    _, q = _pillow(f.getvalue())
    segment = _parse(f.getvalue()).q
    assert [q[t][n] for t in (0, 1) for n in ZIGZAG] == ops.jpeg_qtables(quality) == segment[0] + segment[1]


ARITH = [(64, 96), (50, 75)]
TIE = 0.005


def _arith_pixels(h, w):
    return _photo(92 + h, h, w)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", list(SS))
@pytest.mark.parametrize("size", ARITH, ids=lambda s: "%dx%d" % s)
def test_coefficients_against_fp64(backend, size, ss):
    """Equal wherever the fp64 coef / q lies more than 0.005 from a rounding tie, one step at most inside that window; at most 3 % of the
    coefficients may lie inside it (a condition on the inputs).  Measured shares, fp64 alone, q 50 / 90 / 100: 64 x 96: 0.15 / 0.63 / 0.92 % at
    4:4:4, 0.21 / 0.58 / 1.01 % at 4:2:0; 50 x 75: 0.15 / 0.51 / 1.03 % and 0.18 / 0.51 / 0.91 %."""
    dev = use_backend(backend)
    pix = _arith_pixels(*size)
    for quality in (50, 90, 100):
        got = ops.jpeg_coeffs(pix.to(dev), quality, ss)
        inside = total = 0
        for ci, r in enumerate(_ratios(pix[0].numpy(), quality, ss)):
            g = got[ci][0].cpu().numpy().astype(np.int64)
            assert g.shape == r.shape
            frac = np.abs(r) - np.floor(np.abs(r))
            window = np.abs(frac - 0.5) <= TIE
            diff = np.abs(g - _half_away(r))
            assert (diff[~window] == 0).all() and (diff[window] <= 1).all(), (quality, ci, int(diff.max()))
            inside, total = inside + int(window.sum()), total + window.size
        print("coefficients %s %s q %d: %.2f %% inside the tie window" % (size, ss, quality, 100.0 * inside / total))
        assert inside <= 0.03 * total


_pillow_bound = {}


def _decode_bound():
    """Largest difference between Pillow's decode and the fp64 reconstruction from the same coefficients, on PILLOW-written 4:4:4 files of the
    inputs and qualities below (no device involved): what libjpeg's integer inverse DCT and fixed-point colour conversion cost.  Measured: 2 levels
    (Pillow 12.2); the test allows that + 1."""
    if not _pillow_bound:
        from PIL import Image
        worst = 0
        for h, w in ARITH:
            a = _arith_pixels(h, w)[0].numpy()
            for quality in (50, 90, 100):
                f = io.BytesIO()
                Image.fromarray(a, "RGB").save(f, format="JPEG", quality=quality, subsampling=0, optimize=False)
                j = _parse(f.getvalue())
                dec, _ = _pillow(f.getvalue())
                worst = max(worst, int(np.abs(dec.astype(int) - _reconstruct(j.coefs, j.q, h, w).astype(int)).max()))
        _pillow_bound["v"] = worst
    return _pillow_bound["v"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", ARITH, ids=lambda s: "%dx%d" % s)
def test_decoded_pixels(backend, size):
    dev = use_backend(backend)
    h, w = size
    pix = _arith_pixels(h, w)
    bound = _decode_bound() + 1
    for quality in (50, 90, 100):
        f, = ops.jpeg_encode(pix.to(dev), quality, "4:4:4")
        j = _parse(f)
        dec, _ = _pillow(f)
        worst = int(np.abs(dec.astype(int) - _reconstruct(j.coefs, j.q, h, w).astype(int)).max())
        print("decoded pixels %s q %d: %d levels (bound %d)" % (size, quality, worst, bound))
        assert worst <= bound


# ---- 4. size against Pillow ----
# device / Pillow at 96 x 128 as tools/bench_jpeg.py records it in profiles/jpeg_bench.json ("size_ratio_96x128"); the bound is that + 2 points
RECORDED_RATIO = {(90, "4:4:4"): 0.9949, (90, "4:2:0"): 0.9984, (95, "4:4:4"): 0.9953, (95, "4:2:0"): 0.9934}
SIZE_CASES = [pytest.param(b, 96, 128, marks=m, id="%s-96x128" % b) for b, m in (("emu", ()), ("gpu", pytest.mark.gpu))] + \
             [pytest.param("gpu", 512, 512, marks=pytest.mark.gpu, id="gpu-512x512"), pytest.param("gpu", 1024, 1536, marks=pytest.mark.gpu, id="gpu-1024x1536")]


def _size_pixels(h, w):
    return _photo(60 + h % 7, h, w)


def _pillow_size(a, quality, ss):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a, "RGB").save(f, format="JPEG", quality=quality, subsampling=SS[ss], optimize=False)
    return f.getbuffer().nbytes


@pytest.mark.parametrize("backend,h,w", SIZE_CASES)
def test_size_against_pillow(backend, h, w):
    """The same tables and the same coding as libjpeg's, so the device file exceeds Pillow's by the DRI segment, 2 (MCU rows - 1) marker bytes and the
    padding of each interval; the fp32 DCT rounds a few coefficients the other way than libjpeg's integer one, which moves the size either way."""
    dev = use_backend(backend)
    pix = _size_pixels(h, w)
    for quality in (90, 95):
        for ss in SS:
            f, = ops.jpeg_encode(pix.to(dev), quality, ss)
            dec, _ = _pillow(f)
            assert dec.shape == (h, w, 3)
            ref = _pillow_size(pix[0].numpy(), quality, ss)
            print("size against Pillow %d x %d q %d %s: %d / %d = %.4f" % (h, w, quality, ss, len(f), ref, len(f) / ref))
            assert len(f) <= (RECORDED_RATIO[(quality, ss)] + 0.02) * ref


# ---- 5. capacity ----
# 16 x 4096: one MCU row of 512 (4:4:4) or 256 (4:2:0) MCUs = 1536 blocks: 32 or 16 blocks of jpeg_coeffs_kernel (JPEG_MCUS = 16 MCUs each) and
# 12 pieces of jpeg_pack_kernel (PACK_PIECE = 128 blocks), whose window flushes are split over JPEG_THREADS = 128 threads' runs
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", list(SS))
@pytest.mark.parametrize("size", [(33, 47), (16, 4096)], ids=lambda s: "%dx%d" % s)
def test_capacity_on_noise(backend, size, ss):
    dev = use_backend(backend)
    h, w = size
    pix = torch.randint(0, 256, (1, h, w, 3), generator=torch.Generator().manual_seed(93), dtype=torch.uint8)
    f, = _encode(pix, dev, 100, ss)          # (checks size <= capacity and the sentinel behind the file)
    mcu = 16 if ss == "4:2:0" else 8
    mcuy, per_interval = -(-h // mcu), -(-w // mcu) * (6 if ss == "4:2:0" else 3)
    assert ops.jpeg_capacity(h, w, ss) == HEADER + mcuy * (2 * -(-per_interval * (11 + 11 + 63 * 26) // 8) + 2)
    j = _check_file(f, h, w, 100, ss)
    _check_lossless(j, pix.to(dev), 0, 100, ss)


# ---- 6. refusals (no device) and plumbing ----
def test_abi_symbols():
    src = open(os.path.join(ROOT, "include", "uegan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ["uegan_jpeg_qtables", "uegan_jpeg_capacity_bytes", "uegan_jpeg_workspace_bytes", "uegan_jpeg_encode", "uegan_jpeg_coeffs"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES, name
    use_backend("emu")
    assert all(hasattr(ops.lib(), name) for name in names)
    assert ops.lib().uegan_version() == 105


def test_refusals(monkeypatch):
    use_backend("emu")

    def reached(*a, **k):
        raise AssertionError("a refusal must come before the library is reached")
    monkeypatch.setattr(_lib, "load", reached)
    ok = torch.zeros((1, 4, 5, 3), dtype=torch.uint8)
    for fn in (ops.jpeg_encode, ops.jpeg_sizes, ops.jpeg_coeffs):
        for bad in (ok.float(), ok[0], torch.zeros((1, 4, 5, 4), dtype=torch.uint8), torch.zeros((1, 4, 3, 5), dtype=torch.uint8).permute(0, 1, 3, 2),
                    torch.zeros((1, 8, 5, 3), dtype=torch.uint8)[:, ::2], ok.numpy()):
            with pytest.raises(TypeError):
                fn(bad)
        for empty in (torch.zeros((0, 4, 5, 3), dtype=torch.uint8), torch.zeros((1, 0, 5, 3), dtype=torch.uint8)):
            with pytest.raises(ValueError, match="empty"):
                fn(empty)
        for quality in (0, 101, -1, 95.0, "95", None, True):
            with pytest.raises(ValueError, match="quality"):
                fn(ok, quality)
        for ss in ("4:2:2", "444", 0, None, "4:4:0"):
            with pytest.raises(ValueError, match="subsampling"):
                fn(ok, 95, ss)
    for quality in (0, 101, "95"):
        with pytest.raises(ValueError, match="quality"):
            ops.jpeg_qtables(quality)

    assert uegan_amd.get_image_format() == ("png", 95, "4:4:4") and uegan_amd.set_image_format is tester.set_image_format
    for name in ("JPEG", "jpg", "", None):
        with pytest.raises(ValueError, match="unknown image format"):
            tester.set_image_format(name)
    with pytest.raises(ValueError, match="quality"):
        tester.set_image_format("jpeg", quality=0)
    with pytest.raises(ValueError, match="subsampling"):
        tester.set_image_format("jpeg", subsampling="4:2:2")
    assert tester.get_image_format() == ("png", 95, "4:4:4")
    try:
        tester.set_image_format("jpeg", 80, "4:2:0")
        assert tester.get_image_format() == ("jpeg", 80, "4:2:0") and tester.image_path("a/b.png") == "a/b.jpg"
        with pytest.raises(ValueError, match="2 paths for 1 images"):
            tester.write_images(["a.png", "b.png"], ok)
    finally:
        tester.set_image_format("png")
    assert tester.image_path("a/b.png") == "a/b.png"
    argv = ["--mode", "test", "--is_test_nima", "False"]
    for env, match in (({"UEGAN_IMAGE_FORMAT": "jpg"}, "UEGAN_IMAGE_FORMAT='jpg'"), ({"UEGAN_JPEG_QUALITY": "90"}, "UEGAN_JPEG_QUALITY='90' needs UEGAN_IMAGE_FORMAT=jpeg"),
                       ({"UEGAN_IMAGE_FORMAT": "png", "UEGAN_JPEG_QUALITY": "90"}, "needs UEGAN_IMAGE_FORMAT=jpeg"),
                       ({"UEGAN_IMAGE_FORMAT": "jpeg", "UEGAN_JPEG_QUALITY": "0"}, "UEGAN_JPEG_QUALITY='0'"),
                       ({"UEGAN_IMAGE_FORMAT": "jpeg", "UEGAN_JPEG_QUALITY": "high"}, "UEGAN_JPEG_QUALITY='high'")):
        for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(ValueError, match=match):
            runner.main(argv)
        assert tester.get_image_format() == ("png", 95, "4:4:4")


@pytest.mark.parametrize("backend", BACKENDS)
def test_run_test_in_either_format(backend, tmp_path, monkeypatch):
    """the same names with .jpg, files of the source's size that Pillow opens, no .png beside them, and the same metrics: they are computed before
    the encoding"""
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    sizes = [(40, 52), (33, 47)]
    _tree(Path("src"), sizes)
    _, G = _generator(8, dev)
    res = {}
    try:
        for fmt in tester.IMAGE_FORMATS:
            tester.set_image_format(fmt, 90, "4:2:0")
            loader = data.get_test_loader("src", 0, batch_size=2, num_workers=2, device=dev)
            try:
                res[fmt] = tester.run_test(G, loader, save_dir="out_" + fmt, tag="2.00", compare_dir="cmp_" + fmt)
            finally:
                loader.close()
    finally:
        tester.set_image_format("png")
    assert res["jpeg"] == res["png"] and len(res["jpeg"]["psnr"]) == 2
    for kind, panels in (("out_", 1), ("cmp_", 2)):
        names = sorted(os.listdir(kind + "png"))
        assert len(names) == 2 and all(n.endswith(".png") for n in names)
        assert sorted(os.listdir(kind + "jpeg")) == [n[:-4] + ".jpg" for n in names]
        for n, (h, w) in zip(names, sizes):
            blob = (Path(kind + "jpeg") / (n[:-4] + ".jpg")).read_bytes()
            _check_file(blob, h, panels * w, 90, "4:2:0")


@pytest.mark.parametrize("backend", BACKENDS)
def test_command_line_with_jpeg(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    root = Path("data")
    root.mkdir()
    _make_tree(root, 2, [(40, 52), (36, 36)])
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    for save_root in ("results", "results_jpeg"):
        mdir = Path(save_root) / "UEGAN-FiveK" / "models"
        mdir.mkdir(parents=True)
        torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    argv = ["--mode", "test", "--test_img_dir", "data", "--test_img_size", "32", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "2", "--is_test_nima", "False"]
    for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_PNG_ENCODER"):
        monkeypatch.delenv(k, raising=False)
    runner.main(argv)                                                        # a default run: the names as before
    assert tester.get_image_format() == ("png", 95, "4:4:4")
    monkeypatch.setenv("UEGAN_IMAGE_FORMAT", "jpeg")
    monkeypatch.setenv("UEGAN_JPEG_QUALITY", "85")
    try:
        runner.main(argv + ["--save_root_dir", "results_jpeg"])
        assert tester.get_image_format() == ("jpeg", 85, "4:4:4")
    finally:
        tester.set_image_format("png")
    metrics = []
    for save_root in ("results", "results_jpeg"):
        m = json.loads((Path(save_root) / "UEGAN-FiveK" / "test" / "test_metrics.json").read_text())
        m.pop("checkpoint")
        metrics.append(m)
    assert metrics[0] == metrics[1] and len(metrics[0]["names"]) == 2
    tag = "2.00"
    for sub, suffix, width in (("test_results", "testFakeExp", 32), ("test_compare", "testRealRaw_testFakeExp", 64)):
        want = sorted("%s_%s_%s" % (name, tag, suffix) for name in metrics[0]["names"])
        assert sorted(os.listdir(Path("results") / "UEGAN-FiveK" / "test" / sub)) == [n + ".png" for n in want]
        assert sorted(os.listdir(Path("results_jpeg") / "UEGAN-FiveK" / "test" / sub)) == [n + ".jpg" for n in want]
        for n in want:
            _check_file((Path("results_jpeg") / "UEGAN-FiveK" / "test" / sub / (n + ".jpg")).read_bytes(), 32, width, 85, "4:4:4")
