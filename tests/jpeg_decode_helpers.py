"""libjpeg's default decode path from coefficients to pixels, restated in numpy: dequantisation, the integer "islow" inverse DCT, "fancy" chroma
up-sampling and the fixed-point YCbCr -> RGB conversion.  Written from the arithmetic (jidctint.c, jdsample.c, jdcolor.c), independent of the
device code; tests/test_jpeg_decode.py pins it against Pillow before any kernel is compared with either."""
import io

import numpy as np

from test_jpeg import NATURAL_OF, _parse


def idct_islow(blocks):
    """int64 [..., 8, 8] dequantised coefficients (natural order) -> int64 [..., 8, 8] samples before the level shift and the clamp: columns first
    with (x + 2^10) >> 11, then rows with (x + 2^17) >> 18"""
    def pass_(x, shift):          # along axis -2
        x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i, :] for i in range(8))
        z1 = (x2 + x6) * 4433
        tmp2 = z1 - x6 * 15137
        tmp3 = z1 + x2 * 6270
        tmp0 = (x0 + x4) << 13
        tmp1 = (x0 - x4) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = x7, x5, x3, x1
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        half = 1 << (shift - 1)
        rows = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
        return np.stack([(r + half) >> shift for r in rows], axis=-2)
    ws = pass_(blocks.astype(np.int64), 11)
    return np.swapaxes(pass_(np.swapaxes(ws, -1, -2), 18), -1, -2)


def component_plane(coefs, q_zigzag):
    """[block rows, block cols, 64] zigzag coefficients, the 64 table entries in zigzag order -> uint8 samples [8 rows, 8 cols]"""
    rows, cols, _ = coefs.shape
    nat = np.zeros((rows, cols, 64), dtype=np.int64)
    nat[..., NATURAL_OF] = coefs.astype(np.int64) * np.asarray(q_zigzag, dtype=np.int64)
    x = np.clip(idct_islow(nat.reshape(rows, cols, 8, 8)) + 128, 0, 255)
    return x.transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def _shift(p, d, axis):
    """p moved by d along axis, the edge sample repeated"""
    idx = np.clip(np.arange(p.shape[axis]) + d, 0, p.shape[axis] - 1)
    return np.take(p, idx, axis=axis)


def upsample_h2v1(p):
    if p.shape[1] <= 2:           # (jdsample.c takes the fancy routine only for downsampled_width > 2)
        return np.repeat(p, 2, axis=1)
    out = np.zeros((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * p + _shift(p, -1, 1) + 1) >> 2
    out[:, 1::2] = (3 * p + _shift(p, 1, 1) + 2) >> 2
    return out


def upsample_h2v2(p):
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    out = np.zeros((2 * p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    for v, d in ((0, -1), (1, 1)):
        s = 3 * p + _shift(p, d, 0)
        out[v::2, 0::2] = (3 * s + _shift(s, -1, 1) + 8) >> 4
        out[v::2, 1::2] = (3 * s + _shift(s, 1, 1) + 7) >> 4
    return out


def pixels_from_coefs(coefs, quant, comps, H, W):
    """per component zigzag coefficients over whole MCUs, {table id: 64 entries, zigzag}, [(id, h, v, tq)], the image's size -> uint8 [H, W, 3]"""
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    full = []
    for c, (_, h, v, tq) in zip(coefs, comps):
        p = component_plane(c, quant[tq])[:-(-H * v // vmax), :-(-W * h // hmax)].astype(np.int64)
        if (h, v) == (hmax, vmax):
            pass
        elif (hmax, vmax) == (2 * h, v):
            p = upsample_h2v1(p)
        elif (hmax, vmax) == (2 * h, 2 * v):
            p = upsample_h2v2(p)
        else:
            raise ValueError("sampling %s" % (comps,))
        full.append(p[:H, :W])
    if len(full) == 1:
        return np.repeat(full[0][..., None], 3, axis=2).astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(blob):
    """a baseline JPEG file -> uint8 [H, W, 3], by test_jpeg._parse and the arithmetic above"""
    j = _parse(blob)
    return pixels_from_coefs(j.coefs, j.q, j.comps, j.H, j.W)


# ---- files ----
def photo_like(seed, h, w):
    """smooth structure + a little noise, uint8 [h, w, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.02, 0.35), rng.uniform(0.02, 0.35), rng.uniform(0, 6.28)
            img[..., c] += rng.uniform(20, 60) * np.sin(fy * yy + fx * xx + ph)
    img += 128 + rng.normal(0, 6, size=img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pillow_jpeg(pixels, quality=90, subsampling="4:4:4", **kw):
    """uint8 [h, w, 3] (or [h, w] for a grayscale file) -> the bytes of Pillow's file"""
    from PIL import Image
    f = io.BytesIO()
    if pixels.ndim == 2:
        Image.fromarray(pixels, "L").save(f, format="JPEG", quality=quality, **kw)
    else:
        Image.fromarray(pixels, "RGB").save(f, format="JPEG", quality=quality, subsampling=SUBSAMPLING[subsampling], **kw)
    return f.getvalue()


def pillow_pixels(blob):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.asarray(im.convert("RGB"))
