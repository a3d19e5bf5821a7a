"""Result files written on the device: PNG (csrc/png.hip) and baseline JPEG (csrc/jpeg.hip).  Not autograd and not on the training path:
uint8 images in, complete files as bytes out."""
import ctypes as C

import torch

from . import _lib as L
from .ops.core import _chk, _stream, lib


# --------------------------------------------------------------------------------------------------------------------
# PNG files on the device (csrc/png.hip)
# --------------------------------------------------------------------------------------------------------------------
PNG_MAX_BAND = 65535          # the default and largest band: what one stored deflate block holds


def _png_band(band_bytes, least, what):
    bb = PNG_MAX_BAND if band_bytes is None else int(band_bytes)
    if not least <= bb <= PNG_MAX_BAND:
        raise ValueError("%s: band_bytes %d is not in [%d, %d]" % (what, bb, least, PNG_MAX_BAND))
    return bb


def _fetch_files(out, stride, sizes):
    """one read of the sizes (a device tensor, or the list already read), one D2H copy of the used bytes -> list[bytes]"""
    sizes = [int(v) for v in (sizes.tolist() if torch.is_tensor(sizes) else sizes)]
    used = out[:sizes[0]] if len(sizes) == 1 else torch.cat([out[i * stride:i * stride + n] for i, n in enumerate(sizes)])
    host = used.cpu().numpy().tobytes()
    ends = [0]
    for n in sizes:
        ends.append(ends[-1] + n)
    return [host[ends[i]:ends[i + 1]] for i in range(len(sizes))]


def png_encode(images_u8, band_bytes=None):
    """uint8 [B,H,W,3] on the device -> B complete 8-bit RGB PNG files as bytes, every per-byte step on the device (uegan_png_encode): Paeth filter,
    one dynamic-Huffman deflate block per band of whole rows (at most band_bytes filtered bytes, default 65535), chunk CRCs, Adler-32.  The host
    reads the B sizes and copies the used bytes.  Refused before any launch: anything but a contiguous uint8 [B,H,W,3] tensor (TypeError), an
    empty image, a row that does not fit a band (3W + 1 > 65535), band_bytes outside [3W + 1, 65535] (ValueError)."""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
        raise TypeError("png_encode expects a contiguous uint8 [B,H,W,3] tensor")
    B, H, W, _ = images_u8.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("png_encode: empty image stack %s" % (tuple(images_u8.shape),))
    row = 3 * W + 1
    if row > PNG_MAX_BAND:
        raise ValueError("png_encode: a filtered row of %d pixels (%d bytes) does not fit a band of %d bytes" % (W, row, PNG_MAX_BAND))
    bb = _png_band(band_bytes, row, "png_encode")
    _chk(images_u8)
    dev = images_u8.device
    stride = (lib().uegan_png_capacity_bytes(H, W, bb) + 15) // 16 * 16
    out = torch.empty((B * stride,), dtype=torch.uint8, device=dev)
    sizes = torch.empty((B,), dtype=torch.int64, device=dev)
    ws = torch.empty((lib().uegan_png_workspace_bytes(B, H, W, bb),), dtype=torch.uint8, device=dev)
    L.check(lib().uegan_png_encode(images_u8.data_ptr(), B, H, W, bb, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), _stream()))
    return _fetch_files(out, stride, sizes)


def deflate_bands(data_u8, band_bytes=None):
    """the band coder of png_encode on a 1-D uint8 tensor, without filter and PNG framing: a bare zlib stream of one dynamic-Huffman (or stored) block
    per band_bytes bytes (uegan_deflate_bands) -> bytes; band_bytes in [1, 65535]"""
    if not torch.is_tensor(data_u8) or data_u8.dtype != torch.uint8 or data_u8.dim() != 1 or not data_u8.is_contiguous():
        raise TypeError("deflate_bands expects a contiguous 1-D uint8 tensor")
    n = data_u8.numel()
    if n < 1:
        raise ValueError("deflate_bands: no data")
    bb = _png_band(band_bytes, 1, "deflate_bands")
    _chk(data_u8)
    dev = data_u8.device
    cap = lib().uegan_png_capacity_bytes(n, 0, bb)
    out = torch.empty((cap,), dtype=torch.uint8, device=dev)
    size = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = torch.empty((lib().uegan_png_workspace_bytes(1, n, 0, bb),), dtype=torch.uint8, device=dev)
    L.check(lib().uegan_deflate_bands(data_u8.data_ptr(), n, bb, out.data_ptr(), size.data_ptr(), ws.data_ptr(), _stream()))
    return _fetch_files(out, cap, size)[0]


# --------------------------------------------------------------------------------------------------------------------
# Baseline JPEG files on the device (csrc/jpeg.hip)
# --------------------------------------------------------------------------------------------------------------------
JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:0": 2}          # name -> the code of the C ABI (Pillow's)
JPEG_MAX_SIDE = 65535                                 # the SOF0 fields; it also keeps the restart interval of one MCU row inside DRI's 16 bits


def _jpeg_args(images_u8, quality, subsampling, what):
    """the refusals shared by the three entry points, all before any launch -> (B, H, W, quality, subsampling code)"""
    if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
        raise TypeError("%s expects a contiguous uint8 [B,H,W,3] tensor" % what)
    B, H, W, _ = images_u8.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty image stack %s" % (what, tuple(images_u8.shape)))
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("%s: quality %r is not an integer in [1, 100]" % (what, quality))
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("%s: subsampling %r is not one of %s" % (what, subsampling, ", ".join(JPEG_SUBSAMPLINGS)))
    if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
        raise ValueError("%s: %d x %d exceeds %d (SOF0's 16-bit fields, and DRI's for a restart interval of one MCU row)" % (what, H, W, JPEG_MAX_SIDE))
    return B, H, W, quality, JPEG_SUBSAMPLINGS[subsampling]


def jpeg_qtables(quality):
    """the 128 quantisation table entries of `quality` (Annex K.1 / K.2 by libjpeg's rule), zigzag order, luma then chroma (host only)"""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("jpeg_qtables: quality %r is not an integer in [1, 100]" % (quality,))
    buf = (C.c_uint8 * 128)()
    L.check(lib().uegan_jpeg_qtables(quality, buf))
    return list(buf)


def _jpeg_flags(optimize, what):
    """optimize -> the flags of the _ex entry points (bit 0: the image's own Huffman tables); only a bool is taken"""
    if not isinstance(optimize, bool):
        raise ValueError("%s: optimize %r is not a bool" % (what, optimize))
    return 1 if optimize else 0


def jpeg_capacity(H, W, subsampling="4:4:4", optimize=False):
    """bytes no file of this shape can exceed (uegan_jpeg_capacity_bytes: every code at its longest, every byte stuffed; optimize: an own DC table
    may hold a 16-bit code where the standard ones stop at 11, so the bound is a little larger)"""
    flags = _jpeg_flags(optimize, "jpeg_capacity")
    return int(lib().uegan_jpeg_capacity_bytes_ex(H, W, JPEG_SUBSAMPLINGS[subsampling], flags))


def jpeg_coeffs(images_u8, quality=95, subsampling="4:4:4"):
    """stage 1 of jpeg_encode alone (uegan_jpeg_coeffs): the quantised DCT coefficients as [Y, Cb, Cr], each an int16 device tensor
    [B, block rows, block cols, 64] in zigzag order (4:2:0: Y has twice the rows and columns of Cb / Cr)"""
    B, H, W, q, ss = _jpeg_args(images_u8, quality, subsampling, "jpeg_coeffs")
    _chk(images_u8)
    mcu = 16 if ss else 8
    my, mx = -(-H // mcu), -(-W // mcu)
    shapes = [(2 * my, 2 * mx) if ss else (my, mx), (my, mx), (my, mx)]
    per = sum(r * c for r, c in shapes)
    flat = torch.empty((B, per, 64), dtype=torch.int16, device=images_u8.device)
    L.check(lib().uegan_jpeg_coeffs(images_u8.data_ptr(), B, H, W, q, ss, flat.data_ptr(), _stream()))
    planes, at = [], 0
    for r, c in shapes:
        planes.append(flat[:, at:at + r * c].reshape(B, r, c, 64))
        at += r * c
    return planes


def jpeg_histogram(images_u8, quality=95, subsampling="4:4:4"):
    """the statistics pass of the optimised mode alone (uegan_jpeg_coeffs, then uegan_jpeg_histogram): how often the entropy coder emits each symbol
    of each table for these images -> int64 device tensor [B, 4, 256], tables in the order DC luma, DC chroma, AC luma, AC chroma"""
    B, H, W, q, ss = _jpeg_args(images_u8, quality, subsampling, "jpeg_histogram")
    _chk(images_u8)
    flat = torch.cat([p.reshape(B, -1) for p in jpeg_coeffs(images_u8, quality, subsampling)], dim=1).contiguous()
    hist = torch.empty((B, 4, 256), dtype=torch.int64, device=images_u8.device)
    L.check(lib().uegan_jpeg_histogram(flat.data_ptr(), B, H, W, ss, hist.data_ptr(), _stream()))
    return hist


def jpeg_build_tables(hist):
    """the code construction of the optimised mode alone (uegan_jpeg_build_tables: Annex K.2 as libjpeg's jpeg_gen_optimal_table) on any counts.
    hist: int64 [n, 4, 256] on the device, counts >= 0 -> (dht uint8 [n, 4, 272]: per table the 16 BITS counts, then HUFFVAL, zero-filled;
    codes int32 [n, 4, 256]: per symbol length << 16 | code, 0 for a symbol that does not occur)"""
    if not torch.is_tensor(hist) or hist.dtype != torch.int64 or hist.dim() != 3 or tuple(hist.shape[1:]) != (4, 256) or not hist.is_contiguous():
        raise TypeError("jpeg_build_tables expects a contiguous int64 [n, 4, 256] tensor")
    n = hist.shape[0]
    if not 1 <= n <= 65535:
        raise ValueError("jpeg_build_tables: %d histogram sets (1..65535)" % n)
    _chk(hist)
    dht = torch.empty((n, 4, 272), dtype=torch.uint8, device=hist.device)
    codes = torch.empty((n, 4, 256), dtype=torch.int32, device=hist.device)
    L.check(lib().uegan_jpeg_build_tables(hist.data_ptr(), n, dht.data_ptr(), codes.data_ptr(), _stream()))
    return dht, codes


def _jpeg_sizing(images_u8, B, H, W, q, ss, flags=0):
    """the sizing step -> (sizes tensor, workspace): coefficients, code lengths and offsets stay in the workspace"""
    dev = images_u8.device
    sizes = torch.empty((B,), dtype=torch.int64, device=dev)
    ws = torch.empty((lib().uegan_jpeg_workspace_bytes_ex(B, H, W, ss, flags),), dtype=torch.uint8, device=dev)
    L.check(lib().uegan_jpeg_encode_ex(images_u8.data_ptr(), B, H, W, q, ss, flags, None, 0, sizes.data_ptr(), ws.data_ptr(), _stream()))
    return sizes, ws


def jpeg_sizes(images_u8, quality=95, subsampling="4:4:4", optimize=False):
    """the exact sizes of the files jpeg_encode would return, without writing them (the sizing step of uegan_jpeg_encode) -> list of B ints"""
    B, H, W, q, ss = _jpeg_args(images_u8, quality, subsampling, "jpeg_sizes")
    flags = _jpeg_flags(optimize, "jpeg_sizes")
    _chk(images_u8)
    return [int(v) for v in _jpeg_sizing(images_u8, B, H, W, q, ss, flags)[0].tolist()]


def jpeg_encode(images_u8, quality=95, subsampling="4:4:4", out=None, optimize=False):
    """uint8 [B,H,W,3] on the device -> B complete baseline JPEG files as bytes (uegan_jpeg_encode: JFIF YCbCr, fp32 DCT, the Annex K tables, one
    restart interval per MCU row), every per-pixel and per-bit step on the device.  The capacity bound of a shape is far above what a photograph
    takes, so the call is split: the sizing step leaves the exact file sizes on the device, the host reads them, allocates exactly that and runs
    the writing step; then one D2H copy of the files.  out: a uint8 device tensor [B, stride] with stride >= jpeg_capacity(H, W, subsampling) to
    encode into in ONE call instead (the files are returned all the same; bytes of `out` behind a file are left as they were).
    Refused before any launch: anything but a contiguous uint8 [B,H,W,3] tensor (TypeError); an empty batch, a quality outside 1..100, a subsampling
    other than "4:4:4" / "4:2:0", a side above 65535, an optimize that is not a bool (ValueError).
    optimize=True (uegan_jpeg_encode_ex, flags bit 0): every file carries its own four Huffman tables, built on the device from that image's symbol
    counts the way libjpeg's optimize does -- the same coefficients and decoded pixels in a smaller file; `out` then needs
    jpeg_capacity(H, W, subsampling, optimize=True).  False: the Annex K.3 tables, every byte as before."""
    B, H, W, q, ss = _jpeg_args(images_u8, quality, subsampling, "jpeg_encode")
    flags = _jpeg_flags(optimize, "jpeg_encode")
    dev = images_u8.device
    if out is not None:
        cap = lib().uegan_jpeg_capacity_bytes_ex(H, W, ss, flags)
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < cap or not out.is_contiguous() \
                or out.device != dev:
            raise TypeError("jpeg_encode: out must be a contiguous uint8 [%d, >= %d] tensor on the images' device" % (B, cap))
        _chk(images_u8, out)
        stride = out.shape[1]
        sizes = torch.empty((B,), dtype=torch.int64, device=dev)
        ws = torch.empty((lib().uegan_jpeg_workspace_bytes_ex(B, H, W, ss, flags),), dtype=torch.uint8, device=dev)
        L.check(lib().uegan_jpeg_encode_ex(images_u8.data_ptr(), B, H, W, q, ss, flags, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), _stream()))
        return _fetch_files(out.view(-1), stride, sizes)
    _chk(images_u8)
    sizes, ws = _jpeg_sizing(images_u8, B, H, W, q, ss, flags)
    known = [int(v) for v in sizes.tolist()]
    stride = max((max(known) + 15) // 16 * 16, 640)          # (the C entry asks for room for the longest header, whatever this one's length)
    buf = torch.empty((B * stride,), dtype=torch.uint8, device=dev)
    L.check(lib().uegan_jpeg_encode_ex(None, B, H, W, q, ss, flags, buf.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), _stream()))
    return _fetch_files(buf, stride, known)
