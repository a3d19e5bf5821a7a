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


# --------------------------------------------------------------------------------------------------------------------
# Baseline JPEG files read on the device (csrc/jpeg_decode.hip)
# --------------------------------------------------------------------------------------------------------------------
JPEG_SUBSEQ_BITS = 1024          # the default sub-sequence of the entropy decoder; 0: one thread per restart interval
JPEG_MAX_ROUNDS = 512            # the default bound of the synchronisation rounds
JPEG_E_DESYNC, JPEG_E_STREAM = -4, -5


class JpegUnsupported(ValueError):
    """a file the device decoder declines by its header, before any launch (the caller decodes it with Pillow)"""


class JpegDecodeError(RuntimeError):
    """uegan_jpeg_decode returned a status; .status: JPEG_E_DESYNC (not synchronised within max_rounds) or JPEG_E_STREAM (the stream contradicts the header)"""

    def __init__(self, status, message):
        RuntimeError.__init__(self, "jpeg_decode: status %d: %s" % (status, message))
        self.status = status


class JpegInfo:
    """What jpeg_info read: height, width, components [(id, h, v, tq, td, ta)], subsampling ("gray", "4:4:4", "4:2:2", "4:2:0"), restart_interval,
    scan_offset / scan_length (the bytes behind SOS), mcux / mcuy, planes [(block rows, block cols)] per component, blocks (their sum), intervals,
    desc (the uegan_jpeg_desc of the C ABI)"""


_SOF_NAMES = {0xc1: "extended sequential (SOF1)", 0xc2: "progressive (SOF2)", 0xc3: "lossless (SOF3)", 0xc5: "differential (SOF5)", 0xc6: "differential (SOF6)",
              0xc7: "differential (SOF7)", 0xc9: "arithmetic coding (SOF9)", 0xca: "arithmetic coding (SOF10)", 0xcb: "arithmetic coding (SOF11)",
              0xcd: "arithmetic coding (SOF13)", 0xce: "arithmetic coding (SOF14)", 0xcf: "arithmetic coding (SOF15)"}


def jpeg_info(blob):
    """Parse a JPEG file's header up to SOS (host only; nothing behind SOS is read) -> JpegInfo.  JpegUnsupported names what the device decoder
    declines: anything but SOF0 with 8-bit samples and tables, one interleaved scan over all components (0, 63, 0), one component or three in
    4:4:4 / 4:2:2 / 4:2:0 that libjpeg reads as YCbCr (JFIF, or Adobe transform 1, or neither and ids 1, 2, 3), sides 1..65535 and a padded area of
    at most data.NATIVE_TILED_MAX_PIXELS.  A file that is no JPEG at all is declined the same way."""
    n = len(blob)
    if n < 4 or blob[0] != 0xff or blob[1] != 0xd8:
        raise JpegUnsupported("not a JPEG file")
    pos = 2
    quant, huff, sof, dri, jfif, adobe = {}, {}, None, 0, False, None
    while True:
        while pos < n and blob[pos] != 0xff:          # (libjpeg skips garbage before a marker with a warning)
            pos += 1
        while pos < n and blob[pos] == 0xff:
            pos += 1
        if pos >= n:
            raise JpegUnsupported("no scan (SOS) in the file")
        m = blob[pos]
        pos += 1
        if m == 0xd8 or m == 0x01 or 0xd0 <= m <= 0xd7:
            continue
        if m == 0xd9:
            raise JpegUnsupported("no scan (SOS) in the file")
        if pos + 2 > n:
            raise JpegUnsupported("truncated header")
        ln = blob[pos] << 8 | blob[pos + 1]
        body = bytes(blob[pos + 2:pos + ln])
        if ln < 2 or pos + ln > n:
            raise JpegUnsupported("truncated header")
        pos += ln
        if m in _SOF_NAMES:
            raise JpegUnsupported(_SOF_NAMES[m])
        if m == 0xcc:
            raise JpegUnsupported("arithmetic coding (DAC)")
        if m == 0xc0:
            if sof is not None:
                raise JpegUnsupported("two frame headers")
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                raise JpegUnsupported("truncated header")
            sof = (body[0], body[1] << 8 | body[2], body[3] << 8 | body[4], [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])])
        elif m == 0xdb:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    raise JpegUnsupported("16-bit quantisation table")
                if (body[at] & 15) > 3 or at + 65 > len(body):
                    raise JpegUnsupported("bad quantisation table")
                quant[body[at] & 15] = body[at + 1:at + 65]
                at += 65
        elif m == 0xc4:
            at = 0
            while at < len(body):
                tc, th = body[at] >> 4, body[at] & 15
                counts = body[at + 1:at + 17]
                if tc > 1 or th > 3 or len(counts) < 16 or sum(counts) > 256 or at + 17 + sum(counts) > len(body):
                    raise JpegUnsupported("bad Huffman table")
                code = 0
                for c in counts:          # (libjpeg refuses an oversubscribed table too)
                    code = (code + c) << 1
                    if code > 1 << 17:
                        break
                space = 0
                for length, c in enumerate(counts, 1):
                    space += c << (16 - length)
                if space > 1 << 16:
                    raise JpegUnsupported("bad Huffman table")
                huff[(tc, th)] = (counts, body[at + 17:at + 17 + sum(counts)])
                at += 17 + sum(counts)
        elif m == 0xdd:
            if len(body) < 2:
                raise JpegUnsupported("truncated header")
            dri = body[0] << 8 | body[1]
        elif m == 0xe0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xee and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xda:
            scan = body
            break
    if sof is None:
        raise JpegUnsupported("a scan before the frame header")
    precision, H, W, comps = sof
    if precision != 8:
        raise JpegUnsupported("%d-bit samples" % precision)
    if H < 1 or W < 1:
        raise JpegUnsupported("a side of 0 (DNL)")
    nc = len(comps)
    if nc == 4:
        raise JpegUnsupported("four components (CMYK / YCCK)")
    if nc not in (1, 3):
        raise JpegUnsupported("%d components" % nc)
    if len(scan) < 1 or scan[0] != nc or len(scan) != 4 + 2 * nc:
        raise JpegUnsupported("several scans (not one interleaved scan over all components)")
    if tuple(scan[1 + 2 * nc:]) != (0, 63, 0):
        raise JpegUnsupported("a scan that is not (Ss, Se, Ah/Al) = (0, 63, 0)")
    if [scan[1 + 2 * i] for i in range(nc)] != [c[0] for c in comps]:
        raise JpegUnsupported("scan components in another order than the frame's")
    tabs = [(scan[2 + 2 * i] >> 4, scan[2 + 2 * i] & 15) for i in range(nc)]
    if nc == 3:
        if not jfif:
            if adobe is not None and adobe != 1:
                raise JpegUnsupported("Adobe colour transform %d" % adobe)
            if adobe is None and [c[0] for c in comps] != [1, 2, 3]:
                raise JpegUnsupported("component ids %s without JFIF or Adobe marker" % [c[0] for c in comps])
        samp = [(c[1], c[2]) for c in comps]
        names = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}
        if samp[0] not in names or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise JpegUnsupported("sampling factors %s" % "".join("%dx%d " % s for s in samp).strip())
        subsampling = names[samp[0]]
        hmax, vmax = samp[0]
    else:
        comps = [(comps[0][0], 1, 1, comps[0][3])]          # (a scan of one component is not interleaved: its sampling factors mean nothing)
        subsampling, hmax, vmax = "gray", 1, 1
    for (cid, h, v, tq), (td, ta) in zip(comps, tabs):
        if tq > 3 or tq not in quant:
            raise JpegUnsupported("quantisation table %d is not defined" % tq)
        if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
            raise JpegUnsupported("Huffman table %d / %d is not defined" % (td, ta))
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    from . import data
    if mcux * mcuy * 64 * hmax * vmax > data.NATIVE_TILED_MAX_PIXELS:
        raise JpegUnsupported("%d x %d pads to %d pixels, above %d" % (H, W, mcux * mcuy * 64 * hmax * vmax, data.NATIVE_TILED_MAX_PIXELS))
    if n - pos < 1 or n - pos > 1 << 28:
        raise JpegUnsupported("%d bytes behind SOS" % (n - pos))
    info = JpegInfo()
    info.height, info.width, info.subsampling, info.restart_interval = H, W, subsampling, dri
    info.components = [(cid, h, v, tq, td, ta) for (cid, h, v, tq), (td, ta) in zip(comps, tabs)]
    info.scan_offset, info.scan_length, info.mcux, info.mcuy = pos, n - pos, mcux, mcuy
    info.planes = [(mcuy * v, mcux * h) for _, h, v, _ in comps]
    info.blocks = sum(r * c for r, c in info.planes)
    info.intervals = -(-mcux * mcuy // dri) if dri else 1
    d = L.JpegDesc()
    d.H, d.W, d.ncomp, d.restart_interval, d.scan_offset, d.scan_length = H, W, nc, dri, pos, n - pos
    for i, (cid, h, v, tq, td, ta) in enumerate(info.components):
        d.h[i], d.v[i], d.tq[i], d.td[i], d.ta[i] = h, v, tq, td, ta
    for t, q in quant.items():
        C.memmove(d.quant[t], bytes(q), 64)
    for (tc, th), (counts, syms) in huff.items():
        tab = (d.ac if tc else d.dc)[th]
        C.memmove(tab.counts, bytes(counts), 16)
        C.memmove(tab.symbols, bytes(syms), len(syms))
    info.desc = d
    return info


def _jpeg_decode_args(subseq_bits, max_rounds):
    s = JPEG_SUBSEQ_BITS if subseq_bits is None else subseq_bits
    r = JPEG_MAX_ROUNDS if max_rounds is None else max_rounds
    if isinstance(s, bool) or not isinstance(s, int) or (s != 0 and (s < 128 or s % 32 or s > 1 << 20)):
        raise ValueError("jpeg_decode: subseq_bits %r is not 0 (one thread per restart interval) or a multiple of 32 in [128, 2^20]" % (subseq_bits,))
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError("jpeg_decode: max_rounds %r is not an integer >= 1" % (max_rounds,))
    return s, r


def _jpeg_status(rc):
    if rc == 0:
        return
    msg = lib().uegan_last_error()
    msg = msg.decode() if msg else "?"
    if rc in (JPEG_E_DESYNC, JPEG_E_STREAM):
        raise JpegDecodeError(rc, msg)
    raise RuntimeError("libuegan_hip error %d: %s" % (rc, msg))


def jpeg_decode_into(info, file_u8, out_u8, subseq_bits=None, max_rounds=None, stream=None, timings=False):
    """The launches of jpeg_decode for one file: file_u8 a 1-D uint8 device tensor holding the file jpeg_info read, out_u8 a contiguous uint8 device
    tensor of height * width * 3 elements whose first byte is 16-byte aligned.  -> {"rounds", "subsequences", "intervals", "stream_bytes"} and,
    with timings=True, "stage_ms": [unstuff, rounds, write pass, pixels] by HIP events.  stream: a raw stream handle (default: the current one).
    JpegDecodeError for a status: out_u8 then holds nothing of use."""
    s, r = _jpeg_decode_args(subseq_bits, max_rounds)
    if not torch.is_tensor(file_u8) or file_u8.dtype != torch.uint8 or file_u8.dim() != 1 or not file_u8.is_contiguous() or \
            file_u8.numel() < info.scan_offset + info.scan_length:
        raise TypeError("jpeg_decode_into: the file must be a contiguous 1-D uint8 tensor of at least %d bytes" % (info.scan_offset + info.scan_length))
    if not torch.is_tensor(out_u8) or out_u8.dtype != torch.uint8 or not out_u8.is_contiguous() or out_u8.numel() != info.height * info.width * 3 or \
            out_u8.data_ptr() % 16 or out_u8.device != file_u8.device:
        raise TypeError("jpeg_decode_into: out must be a contiguous 16-byte aligned uint8 tensor of %d x %d x 3 on the file's device" % (info.height, info.width))
    _chk(file_u8, out_u8)
    ws = torch.empty((lib().uegan_jpeg_decode_workspace_bytes(C.byref(info.desc), s),), dtype=torch.uint8, device=file_u8.device)
    stats = (C.c_int32 * 4)()
    ms = (C.c_float * 4)() if timings else None
    L.n_calls += 1
    _jpeg_status(lib().uegan_jpeg_decode(file_u8.data_ptr(), C.byref(info.desc), s, r, out_u8.data_ptr(), stats, ms, ws.data_ptr(),
                                         _stream() if stream is None else stream))
    res = {"rounds": stats[0], "subsequences": stats[1], "intervals": stats[2], "stream_bytes": stats[3]}
    if timings:
        res["stage_ms"] = list(ms)
    return res


def _jpeg_upload(blob, device):
    host = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    return host if L.is_emulated() else host.to(torch.device("cuda") if device is None else device)


def jpeg_decode(blobs, device=None, subseq_bits=None, max_rounds=None):
    """Baseline JPEG files (bytes) -> a list of uint8 [1, h, w, 3] device tensors, byte for byte Pillow's Image.open(f).convert("RGB")
    (uegan_jpeg_decode: unstuffing, entropy decoding, libjpeg's integer inverse DCT, fancy up-sampling and colour conversion on the device; the host
    parses the header and copies the file up).  subseq_bits: the entropy decoder's sub-sequence (default 1024; 0: one thread per restart interval);
    max_rounds: the bound of its synchronisation rounds.  JpegUnsupported: a file is declined by its header, before any launch (jpeg_info lists
    what is accepted).  JpegDecodeError: the device returned a status (not synchronised within max_rounds, or a stream that contradicts its header)."""
    if isinstance(blobs, (bytes, bytearray, memoryview)):
        raise TypeError("jpeg_decode expects a list of files (bytes)")
    _jpeg_decode_args(subseq_bits, max_rounds)
    infos = [jpeg_info(b) for b in blobs]          # every refusal comes before the first launch
    out = []
    for blob, info in zip(blobs, infos):
        f = _jpeg_upload(blob, device)
        px = torch.empty((1, info.height, info.width, 3), dtype=torch.uint8, device=f.device)
        jpeg_decode_into(info, f, px, subseq_bits, max_rounds)
        out.append(px)
    return out


def jpeg_decode_coeffs(blob, device=None, subseq_bits=None, max_rounds=None):
    """the unstuffing and entropy stages of jpeg_decode alone (uegan_jpeg_decode_coeffs) -> (planes, stats): per component an int16 device tensor
    [block rows, block cols, 64] in zigzag order over whole MCUs, DC values summed; stats as jpeg_decode_into's"""
    s, r = _jpeg_decode_args(subseq_bits, max_rounds)
    info = jpeg_info(blob)
    f = _jpeg_upload(blob, device)
    _chk(f)
    flat = torch.empty((info.blocks, 64), dtype=torch.int16, device=f.device)
    ws = torch.empty((lib().uegan_jpeg_decode_workspace_bytes(C.byref(info.desc), s),), dtype=torch.uint8, device=f.device)
    stats = (C.c_int32 * 4)()
    L.n_calls += 1
    _jpeg_status(lib().uegan_jpeg_decode_coeffs(f.data_ptr(), C.byref(info.desc), s, r, flat.data_ptr(), stats, ws.data_ptr(), _stream()))
    planes, at = [], 0
    for rows, cols in info.planes:
        planes.append(flat[at:at + rows * cols].reshape(rows, cols, 64))
        at += rows * cols
    return planes, {"rounds": stats[0], "subsequences": stats[1], "intervals": stats[2], "stream_bytes": stats[3]}
