"""Per-image Huffman tables for the device JPEG encoder (csrc/jpeg.hip: jpeg_stats_kernel, jpeg_build_kernel, the packer and the offsets in their
optimised mode) through ops.jpeg_encode / jpeg_sizes / jpeg_capacity(optimize=True), ops.jpeg_histogram, ops.jpeg_build_tables,
tester.set_image_format(optimize=) and the command line with UEGAN_JPEG_OPTIMIZE=1.

The oracle of the code construction is `k2` below: Annex K.2 as libjpeg's jpeg_gen_optimal_table states it, restated in Python and pinned to
libjpeg itself (the tables of Pillow's optimize=True files, case 1).  Files are read by test_jpeg.py's baseline reader, which decodes any DHT, and by
Pillow."""
import io
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import BACKENDS, ROOT, use_backend
from test_data import _make_tree
from test_jpeg import EOB, SENTINEL, SHAPES, SS, _check_lossless, _crafted, _parse, _pillow, _standard_dht
from test_native import _generator, _photo, _pixels, _tree
from uegan_amd import _lib, data, models, ops, runner, tester
import uegan_amd

HEADER_MAX = 629
STANDARD_NVALS = 348          # 12 + 162 + 12 + 162
TABLES = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (class, id) in the order of the histograms: DC luma, DC chroma, AC luma, AC chroma
FILE_ORDER = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ---- the rule, restated ----
def k2(freq_in):
    """256 counts -> (BITS [16], HUFFVAL) by jpeg_gen_optimal_table's rule, without its 32-level limit on the unlimited tree"""
    freq = [int(v) for v in freq_in] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * (max(max(codesize), 16) + 2)
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1
    vals = [s for length in range(1, len(bits)) for s in range(256) if codesize[s] == length]
    return bits[1:17], vals


def _canonical(bits, vals):
    """{symbol: (length, code)} of BITS / HUFFVAL"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (length, code)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _histograms(j):
    """the parsed file's symbols -> {(class, id): 256 counts}"""
    h = {t: [0] * 256 for t in TABLES}
    for ci, recs in enumerate(j.symbols):
        th = 0 if ci == 0 else 1
        for rec in recs:
            h[(0, th)][rec[0]] += 1
            for s in rec[1:]:
                h[(1, th)][s] += 1
    return h


# ---- 1. the restatement is libjpeg's (no device) ----
def _pillow_optimized(a, quality, ss):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a, "RGB").save(f, format="JPEG", quality=quality, subsampling=ss, optimize=True)
    return f.getvalue()


def test_restatement_is_libjpegs():
    cases = [(_photo(7, 96, 128)[0].numpy(), q, ss) for q in (30, 75, 95, 100) for ss in (0, 2)]
    cases += [(_pixels(3, 1, 40, 56)[0].numpy(), q, 0) for q in (50, 100)]
    cases += [(np.full((24, 24, 3), 77, np.uint8), 90, 0)]
    tables = 0
    for a, quality, ss in cases:
        j = _parse(_pillow_optimized(a, quality, ss))
        h = _histograms(j)
        assert len(j.dht) == 4
        for tc, th, counts, syms in j.dht:
            assert k2(h[(tc, th)]) == (counts, syms), (a.shape, quality, ss, tc, th)
            tables += 1
    assert tables == 44


# ---- 2. the construction kernel against the restatement ----
def _fibonacci(n):
    """n Fibonacci counts scattered over the index range: the unlimited tree is n - 1 levels deep"""
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    h = [0] * 256
    for i, v in enumerate(fib):
        h[i * 7 % 256] = v
    return h


def _crafted_histograms():
    g = np.random.default_rng(20)
    one, two, ac, big = [0] * 256, [0] * 256, [0] * 256, [0] * 256
    one[5] = 9
    two[3] = two[200] = 4
    for s in _standard_dht()[1][3]:
        ac[s] = 7                                   # the 162 AC symbols, all counts equal
    for i, v in enumerate((1 << 40, (1 << 33) + 5, 1 << 32, 3, (1 << 40) + 1, 1 << 20)):
        big[40 * i + 2] = v
    hs = [one, two, ac, [1] * 256, _fibonacci(24), _fibonacci(40), big, [0] * 255 + [3]]
    for r in range(8):
        used = g.random(256) < (0.05, 0.3, 0.7, 1.0)[r % 4]
        used[int(g.integers(256))] = True
        counts = np.where(used, np.floor(np.exp(g.random(256) * (3, 12)[r // 4])), 0).astype(np.int64)
        hs.append([int(v) for v in counts])
    return hs                                       # 16 histograms = n 4 sets of four tables


_k2_cache = {}


def _k2_of(h):
    key = tuple(h)
    if key not in _k2_cache:
        _k2_cache[key] = k2(h)
    return _k2_cache[key]


def _check_table(h, dht, codes):
    """a built table against the restatement, and the properties that hold whatever the restatement says"""
    dht, codes = [int(v) for v in dht], [int(v) for v in codes]
    bits, rest = dht[:16], dht[16:]
    nv = sum(bits)
    vals = rest[:nv]
    assert all(v == 0 for v in rest[nv:])
    assert (bits, vals) == _k2_of(h)
    assert sorted(vals) == [s for s in range(256) if h[s]]                          # exactly the symbols that occur, each once
    assert sum(c << (16 - length) for length, c in enumerate(bits, 1)) <= (1 << 16) - 1          # Kraft, with the all-ones code left free
    want = _canonical(bits, vals)
    for s in range(256):
        if s in want:
            length, code = want[s]
            assert 1 <= length <= 16 and codes[s] == (length << 16 | code), s
            assert code != (1 << length) - 1, "no code is all ones"
        else:
            assert codes[s] == 0, s


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_tables_against_restatement(backend):
    """one used symbol; two equal counts; the 162 AC symbols at equal counts (ties); all 256 at count 1; Fibonacci counts over 24 and 40 symbols
    (unlimited depths 23 and 39: the limiting loop runs); counts above 2^32; a single symbol at index 255; eight random histograms; all of them as
    one call of n = 4 sets with different content per table, and one set alone"""
    dev = use_backend(backend)
    hs = _crafted_histograms()
    assert _k2_of(hs[0]) == ([1] + [0] * 15, [5]) and _k2_of(hs[1]) == ([1, 1] + [0] * 14, [3, 200])          # (the reserved code shares level 2)
    assert _k2_of(hs[4])[0] == [0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 1, 0, 0, 0]
    assert max(i + 1 for i, c in enumerate(_k2_of(hs[5])[0]) if c) == 16
    hist = torch.tensor(hs, dtype=torch.int64).view(4, 4, 256)
    dht, codes = ops.jpeg_build_tables(hist.to(dev))
    assert dht.dtype == torch.uint8 and tuple(dht.shape) == (4, 4, 272) and codes.dtype == torch.int32 and tuple(codes.shape) == (4, 4, 256)
    dht, codes = dht.cpu().view(16, 272).tolist(), codes.cpu().view(16, 256).tolist()
    for i, h in enumerate(hs):
        _check_table(h, dht[i], codes[i])
    single = torch.tensor(hs[4:8], dtype=torch.int64).view(1, 4, 256)
    d1, c1 = ops.jpeg_build_tables(single.to(dev))
    assert d1.cpu().view(4, 272).tolist() == dht[4:8] and c1.cpu().view(4, 256).tolist() == codes[4:8]


@pytest.mark.parametrize("backend", BACKENDS)
def test_build_tables_five_sets(backend):
    """n = 5 in one call, every table of every set different: the grid's second axis and the strides of all three buffers"""
    dev = use_backend(backend)
    g = np.random.default_rng(21)
    hist = torch.from_numpy(np.where(g.random((5, 4, 256)) < 0.2, g.integers(1, 1000, (5, 4, 256)), 0).astype(np.int64))
    hist[:, :, 0] += 1
    dht, codes = ops.jpeg_build_tables(hist.to(dev))
    seen = set()
    for i in range(5):
        for t in range(4):
            _check_table(hist[i, t].tolist(), dht[i, t].cpu().tolist(), codes[i, t].cpu().tolist())
            seen.add(tuple(dht[i, t].cpu().tolist()))
    assert len(seen) == 20


# ---- 3. the statistics kernel ----
def _stats_pixels(shape):
    B, H, W = shape
    pix = _pixels(80 + H, B, H, W)
    if B == 2:
        pix[1] = _photo(81, H, W)[0]
    return pix


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape,ss", [((1, 1, 1), "4:2:0"), ((1, 17, 33), "4:2:0"), ((1, 144, 24), "4:2:0"), ((2, 40, 52), "4:2:0"), ((2, 40, 52), "4:4:4"),
                                      ((1, 16, 1040), "4:4:4")], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_histogram_equals_the_files_symbols(backend, shape, ss):
    """(144, 24) at 4:2:0: nine intervals add to one histogram.  B = 2: a histogram per image.  (16, 1040) at 4:4:4: 390 blocks in one interval,
    four pieces of the 128-thread walk, the last one partly empty."""
    dev = use_backend(backend)
    pix = _stats_pixels(shape).to(dev)
    got = ops.jpeg_histogram(pix, 90, ss)
    assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], 4, 256)
    files = ops.jpeg_encode(pix, 90, ss)
    for b, f in enumerate(files):
        h = _histograms(_parse(f))
        for t, key in enumerate(TABLES):
            assert got[b, t].cpu().tolist() == h[key], (b, key)
    if shape[0] == 2:
        assert not torch.equal(got[0], got[1])


# ---- 4. optimised files ----
def _encode_optimized(pix, dev, quality, ss):
    """test_jpeg._encode for the optimised mode: the one-call path into a sentinel-filled buffer and the two-step path give the same files"""
    B, H, W, _ = pix.shape
    cap = ops.jpeg_capacity(H, W, ss, optimize=True)
    out = torch.full((B, cap + 32), SENTINEL, dtype=torch.uint8).to(dev)
    x = pix.to(dev)
    files = ops.jpeg_encode(x, quality, ss, out=out, optimize=True)
    host = out.cpu().numpy()
    for b, f in enumerate(files):
        assert len(f) <= cap
        assert bytes(host[b, :len(f)]) == f and (host[b, len(f):] == SENTINEL).all()
    assert ops.jpeg_encode(x, quality, ss, optimize=True) == files
    assert ops.jpeg_sizes(x, quality, ss, optimize=True) == [len(f) for f in files]
    return files


def _check_optimized_file(blob, H, W, quality, ss):
    """the layout of the standard file, marker by marker, but for the DHT: each is the restatement applied to the file's own symbols"""
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
    assert [(tc, th) for tc, th, _, _ in j.dht] == FILE_ORDER
    h = _histograms(j)
    for tc, th, counts, syms in j.dht:
        assert (counts, syms) == k2(h[(tc, th)]), (tc, th)
    assert j.dri == mcux
    assert j.scan == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert j.rst == [k % 8 for k in range(mcuy - 1)]
    header = sum(len(body) + 4 for _, body in j.markers) + 2
    assert header == HEADER_MAX - STANDARD_NVALS + sum(len(syms) for _, _, _, syms in j.dht) <= HEADER_MAX
    return j


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", list(SS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_optimized_files(backend, shape, ss):
    dev = use_backend(backend)
    B, H, W = shape
    pix = _stats_pixels(shape)
    files = _encode_optimized(pix, dev, 90, ss)
    standard = ops.jpeg_encode(pix.to(dev), 90, ss)
    assert ops.jpeg_encode(pix.to(dev), 90, ss, optimize=False) == standard
    assert len(files) == B and all(isinstance(f, bytes) for f in files)
    tables = []
    for b in range(B):
        j = _check_optimized_file(files[b], H, W, 90, ss)
        _check_lossless(j, pix.to(dev), b, 90, ss)
        assert np.array_equal(_pillow(files[b])[0], _pillow(standard[b])[0])
        assert sorted(j.dht, key=lambda t: (t[1], t[0])) != _standard_dht()
        tables.append(j.dht)
    if B == 2:
        assert all(tables[0][t] != tables[1][t] for t in range(4))


# ---- 5. crafted streams, quality 100 ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["stuffing", "largest", "zrl", "eob", "full", "grey"])
def test_crafted_streams_optimized(backend, kind):
    """the streams of test_jpeg.py::test_crafted_streams stay lossless under their own tables.  "eob" (one colour): both AC tables hold EOB alone,
    a single 1-bit code; "grey" (every sample 128, so every coefficient is 0): all four tables hold one symbol."""
    dev = use_backend(backend)
    pix = torch.full((1, 24, 24, 3), 128, dtype=torch.uint8) if kind == "grey" else _crafted(kind)
    _, H, W, _ = pix.shape
    for ss in SS:
        if kind == "zrl" and ss == "4:2:0":
            continue
        f, = _encode_optimized(pix, dev, 100, ss)
        j = _check_optimized_file(f, H, W, 100, ss)
        _check_lossless(j, pix.to(dev), 0, 100, ss)
        by_table = {(tc, th): (counts, syms) for tc, th, counts, syms in j.dht}
        if kind in ("eob", "grey"):
            assert by_table[(1, 0)] == by_table[(1, 1)] == ([1] + [0] * 15, [EOB])
        if kind == "grey":
            assert by_table[(0, 0)] == by_table[(0, 1)] == ([1] + [0] * 15, [0])
            mcu, nblk = (8, 3) if ss == "4:4:4" else (16, 6)
            n = -(-W // mcu) * nblk                 # an interval: n blocks of 1 + 1 bits, padded to bytes, and its marker
            assert len(f) == HEADER_MAX - STANDARD_NVALS + 4 + -(-H // mcu) * (-(-2 * n // 8) + 2)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("ss", list(SS))
def test_noise_optimized(backend, ss):
    """64 x 1040 noise at quality 100: intervals of 390 (4:4:4: four pieces) or 390 (4:2:0: 65 MCUs of 6) blocks under tables built from near-flat
    statistics.  Longest code met in these files: 16 bits at 4:4:4 (AC luma) and 16 bits at 4:2:0; lengths of 16 produced by the limiting loop
    are case 2's subject (Fibonacci counts), not this one's."""
    dev = use_backend(backend)
    pix = torch.randint(0, 256, (1, 64, 1040, 3), generator=torch.Generator().manual_seed(93), dtype=torch.uint8)
    f, = _encode_optimized(pix, dev, 100, ss)
    j = _check_optimized_file(f, 64, 1040, 100, ss)
    _check_lossless(j, pix.to(dev), 0, 100, ss)
    print("noise 64 x 1040 %s: longest code %d bits" % (ss, max(i + 1 for _, _, counts, _ in j.dht for i, c in enumerate(counts) if c)))
    assert len(f) < len(ops.jpeg_encode(pix.to(dev), 100, ss)[0])


# ---- 6. size ----
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", [(96, 128), (256, 384)], ids=lambda s: "%dx%d" % s)
def test_optimized_is_smaller(backend, size):
    """Pillow's own optimised / standard pair differs by 5 - 15 % on these inputs, far more than the layout's 2 bytes per MCU row and padding"""
    dev = use_backend(backend)
    h, w = size
    pix = _photo(60 + h % 7, h, w).to(dev)
    for quality in (75, 95):
        for ss in SS:
            std, = ops.jpeg_sizes(pix, quality, ss)
            opt, = ops.jpeg_sizes(pix, quality, ss, optimize=True)
            print("optimised / standard %d x %d q %d %s: %d / %d = %.4f" % (h, w, quality, ss, opt, std, opt / std))
            assert opt < std


# ---- 7. interface ----
NEW_SYMBOLS = ["uegan_jpeg_encode_ex", "uegan_jpeg_workspace_bytes_ex", "uegan_jpeg_capacity_bytes_ex", "uegan_jpeg_histogram", "uegan_jpeg_build_tables"]


def test_abi_symbols():
    src = open(os.path.join(ROOT, "include", "uegan_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES, name
    use_backend("emu")
    assert all(hasattr(ops.lib(), name) for name in NEW_SYMBOLS)
    assert ops.lib().uegan_version() == 105
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):          # the device libraries, as build() leaves them
        blob = open(path, "rb").read()
        assert all(name.encode() in blob for name in NEW_SYMBOLS), path


def test_flags_and_capacity():
    """flags 0 is the standard entry; bit 0 widens the per-block bound from 1660 to 1665 bits; any other bit is refused"""
    use_backend("emu")
    lib = ops.lib()
    for h, w, ss in ((33, 47, 0), (16, 4096, 2), (1, 1, 0)):
        assert lib.uegan_jpeg_capacity_bytes_ex(h, w, ss, 0) == lib.uegan_jpeg_capacity_bytes(h, w, ss) > 0
        assert lib.uegan_jpeg_workspace_bytes_ex(2, h, w, ss, 0) == lib.uegan_jpeg_workspace_bytes(2, h, w, ss) > 0
        mcu = 16 if ss else 8
        mcuy, per_interval = -(-h // mcu), -(-w // mcu) * (6 if ss else 3)
        assert lib.uegan_jpeg_capacity_bytes_ex(h, w, ss, 1) == HEADER_MAX + mcuy * (2 * -(-per_interval * (16 + 11 + 63 * 26) // 8) + 2)
        assert lib.uegan_jpeg_workspace_bytes_ex(2, h, w, ss, 1) > lib.uegan_jpeg_workspace_bytes(2, h, w, ss)
        for flags in (2, 3, 4, -1, 1 << 16):
            assert lib.uegan_jpeg_capacity_bytes_ex(h, w, ss, flags) == 0 and lib.uegan_jpeg_workspace_bytes_ex(2, h, w, ss, flags) == 0
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    sizes, ws = torch.zeros(1, dtype=torch.int64), torch.zeros(1 << 16, dtype=torch.uint8)
    for flags in (2, 3, -1):
        with pytest.raises(RuntimeError, match="flags %d holds an unknown bit" % flags):
            _lib.check(lib.uegan_jpeg_encode_ex(x.data_ptr(), 1, 8, 8, 90, 0, flags, None, 0, sizes.data_ptr(), ws.data_ptr(), None))


def test_refusals(monkeypatch):
    use_backend("emu")

    def reached(*a, **k):
        raise AssertionError("a refusal must come before the library is reached")
    monkeypatch.setattr(_lib, "load", reached)
    ok = torch.zeros((1, 4, 5, 3), dtype=torch.uint8)
    for bad in (1, 0, None, "1", 1.0):
        for fn in (ops.jpeg_encode, ops.jpeg_sizes):
            with pytest.raises(ValueError, match="optimize"):
                fn(ok, 95, "4:4:4", optimize=bad)
        with pytest.raises(ValueError, match="optimize"):
            ops.jpeg_capacity(4, 5, "4:4:4", optimize=bad)
        with pytest.raises(ValueError, match="optimize"):
            tester.set_image_format("jpeg", optimize=bad)
    for bad in (torch.zeros((1, 4, 256), dtype=torch.int32), torch.zeros((4, 256), dtype=torch.int64), torch.zeros((1, 4, 255), dtype=torch.int64), [[0] * 256] * 4):
        with pytest.raises(TypeError):
            ops.jpeg_build_tables(bad)
    with pytest.raises(ValueError, match="optimize"):
        tester.set_image_format("png", optimize=True)
    assert tester.get_image_format() == ("png", 95, "4:4:4") and tester.get_jpeg_optimize() is False
    assert uegan_amd.get_jpeg_optimize is tester.get_jpeg_optimize
    try:
        tester.set_image_format("jpeg", 80, "4:2:0", optimize=True)
        assert tester.get_image_format() == ("jpeg", 80, "4:2:0") and len(tester.get_image_format()) == 3 and tester.get_jpeg_optimize() is True
        tester.set_image_format("jpeg", 80, "4:2:0")
        assert tester.get_jpeg_optimize() is False
        tester.set_image_format("jpeg", optimize=True)
        tester.set_image_format("png")
        assert tester.get_image_format() == ("png", 95, "4:4:4") and tester.get_jpeg_optimize() is False
    finally:
        tester.set_image_format("png")
    argv = ["--mode", "test", "--is_test_nima", "False"]
    for env, match in (({"UEGAN_JPEG_OPTIMIZE": "1"}, "UEGAN_JPEG_OPTIMIZE='1' needs UEGAN_IMAGE_FORMAT=jpeg"),
                       ({"UEGAN_IMAGE_FORMAT": "png", "UEGAN_JPEG_OPTIMIZE": "1"}, "needs UEGAN_IMAGE_FORMAT=jpeg"),
                       ({"UEGAN_IMAGE_FORMAT": "jpeg", "UEGAN_JPEG_OPTIMIZE": "2"}, "UEGAN_JPEG_OPTIMIZE='2'"),
                       ({"UEGAN_IMAGE_FORMAT": "jpeg", "UEGAN_JPEG_OPTIMIZE": "true"}, "UEGAN_JPEG_OPTIMIZE='true'"),
                       ({"UEGAN_IMAGE_FORMAT": "jpeg", "UEGAN_JPEG_OPTIMIZE": ""}, "UEGAN_JPEG_OPTIMIZE=''"),
                       ({"UEGAN_JPEG_OPTIMIZE": "yes"}, "UEGAN_JPEG_OPTIMIZE='yes'")):
        for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_JPEG_OPTIMIZE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(ValueError, match=match):
            runner.main(argv)
        assert tester.get_image_format() == ("png", 95, "4:4:4") and tester.get_jpeg_optimize() is False


@pytest.mark.parametrize("backend", BACKENDS)
def test_run_test_optimized(backend, tmp_path, monkeypatch):
    """the same names, the same metrics (they are computed before the encoding) and the same decoded pixels as the standard-table run; own tables"""
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    sizes = [(40, 52), (33, 47)]
    _tree(Path("src"), sizes)
    _, G = _generator(8, dev)
    res = {}
    try:
        for optimize in (False, True):
            tester.set_image_format("jpeg", 90, "4:2:0", optimize=optimize)
            loader = data.get_test_loader("src", 0, batch_size=2, num_workers=2, device=dev)
            try:
                res[optimize] = tester.run_test(G, loader, save_dir="out_%d" % optimize, tag="2.00", compare_dir="cmp_%d" % optimize)
            finally:
                loader.close()
    finally:
        tester.set_image_format("png")
    assert res[True] == res[False] and len(res[True]["psnr"]) == 2
    for kind, panels in (("out_", 1), ("cmp_", 2)):
        names = sorted(os.listdir(kind + "0"))
        assert len(names) == 2 and all(n.endswith(".jpg") for n in names) and sorted(os.listdir(kind + "1")) == names
        for n, (h, w) in zip(names, sizes):
            blob, std = (Path(kind + "1") / n).read_bytes(), (Path(kind + "0") / n).read_bytes()
            j = _check_optimized_file(blob, h, panels * w, 90, "4:2:0")
            assert sorted(j.dht, key=lambda t: (t[1], t[0])) != _standard_dht() and len(blob) < len(std)
            assert np.array_equal(_pillow(blob)[0], _pillow(std)[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_command_line_optimized(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    root = Path("data")
    root.mkdir()
    _make_tree(root, 2, [(40, 52), (36, 36)])
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    for save_root in ("results_std", "results_opt"):
        mdir = Path(save_root) / "UEGAN-FiveK" / "models"
        mdir.mkdir(parents=True)
        torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    argv = ["--mode", "test", "--test_img_dir", "data", "--test_img_size", "32", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "2", "--is_test_nima", "False"]
    for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_JPEG_OPTIMIZE", "UEGAN_PNG_ENCODER"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("UEGAN_IMAGE_FORMAT", "jpeg")
    monkeypatch.setenv("UEGAN_JPEG_QUALITY", "85")
    try:
        monkeypatch.setenv("UEGAN_JPEG_OPTIMIZE", "0")
        runner.main(argv + ["--save_root_dir", "results_std"])
        assert tester.get_image_format() == ("jpeg", 85, "4:4:4") and tester.get_jpeg_optimize() is False
        monkeypatch.setenv("UEGAN_JPEG_OPTIMIZE", "1")
        runner.main(argv + ["--save_root_dir", "results_opt"])
        assert tester.get_image_format() == ("jpeg", 85, "4:4:4") and tester.get_jpeg_optimize() is True
    finally:
        tester.set_image_format("png")
    metrics = []
    for save_root in ("results_std", "results_opt"):
        m = json.loads((Path(save_root) / "UEGAN-FiveK" / "test" / "test_metrics.json").read_text())
        m.pop("checkpoint")
        metrics.append(m)
    assert metrics[0] == metrics[1] and len(metrics[0]["names"]) == 2
    for sub, suffix, width in (("test_results", "testFakeExp", 32), ("test_compare", "testRealRaw_testFakeExp", 64)):
        want = sorted("%s_2.00_%s.jpg" % (name, suffix) for name in metrics[0]["names"])
        assert sorted(os.listdir(Path("results_opt") / "UEGAN-FiveK" / "test" / sub)) == want
        for n in want:
            blob = (Path("results_opt") / "UEGAN-FiveK" / "test" / sub / n).read_bytes()
            std = (Path("results_std") / "UEGAN-FiveK" / "test" / sub / n).read_bytes()
            j = _check_optimized_file(blob, 32, width, 85, "4:4:4")
            assert sorted(j.dht, key=lambda t: (t[1], t[0])) != _standard_dht()
            assert np.array_equal(_pillow(blob)[0], _pillow(std)[0])
