"""Inference path (tester.py:58-71) and the evaluation metrics of the inference configuration, on the device.

    enhance(G, x)                     tester.py:58-67: `G.eval()`, `torch.no_grad()`, one `G(x)` per image
    GraphedGenerator(G, shape)        the same forward captured once into a hipGraph and replayed (batch-1 inference is
                                      ~60 dependent launches: launch latency, not arithmetic, sets its time)
    enhance_native(G, pixels_u8)      an image at its OWN size: crop(G(reflect_extend(normalise(pixels)))), uint8 in, uint8 out; tile=T: the same,
                                      evaluated tile by tile for images above data.NATIVE_MAX_PIXELS
    enhance_tiled(G, x, core)         G(x) for an fp32 image too large for one forward: two passes over tiles, exact
    montage_place_u8(dst, images, ..) the quantised window of 1..4 images written into a larger uint8 image in place
    montage_u8(a, b, ...)             `to_uint8_image(torch.cat([a, b, ...], 3))` in one launch: the side-by-side sample / compare images
                                      (trainer.py:182-183,244-245, tester.py:73-74); window=(H, W): of the images' top-left H x W corner
    to_uint8_image(x)                 what tester.py:70-71 writes to a PNG: denorm (utils.py:128-130) + torchvision save_image's
                                      mul(255).add(0.5).clamp(0,255).to(uint8), NHWC
    calculate_psnr / calculate_ssim   metrics/CalcPSNR.py:85-92 and metrics/CalcSSIM.py:63 (skimage defaults) with the 4-pixel
                                      border crop both scripts apply (:24,56), computed by libuegan_hip.so kernels
    mean_metric(values)               the TRUE mean; the reference's directory averages divide by N-1 (CalcPSNR.py:77, CalcSSIM.py:75)
    write_pngs(paths, images_u8)      the 8-bit images as PNG files, by the encoder set_png_encoder selects: "pillow" (the default: Image.save on the
                                      host) or "device" (codecs.png_encode: filter, deflate and CRCs in libuegan_hip.so, the host only writes)
    write_images(paths, images_u8)    ... by the format set_image_format selects: "png" (write_pngs, the default) or "jpeg" (codecs.jpeg_encode: baseline
                                      JPEG on the device, files named .jpg; set_image_format(optimize=True): with the image's own Huffman
                                      tables); returns the paths written
    run_test(G, loader, ...)          the loop of Tester.test (tester.py:40-105): enhance every batch of a test loader, write the
                                      PNGs `save_image` would write, PSNR / SSIM against the labels on the device, and the NIMA
                                      score of the enhanced images (uegan_amd/nima.py) when a scorer is passed
"""
import math

import torch

from . import _lib as L
from . import codecs, data, ops
from .ops.core import _chk, _p, _ptr_table, _stream, lib

CROP_BORDER = 4          # CalcPSNR.py:24 / CalcSSIM.py:24


def denorm(x):
    """utils.py:128-130"""
    out = (x + 1) / 2.0
    return out.clamp_(0, 1)


@torch.no_grad()
def enhance(G, x):
    """tester.py:58-67 inner loop body: eval-mode generator forward."""
    G.eval()
    return G(x)


class GraphedGenerator:
    """`enhance` for a fixed input shape as one hipGraph launch: the eval-mode forward is captured once on a side stream
    (torch.cuda.CUDAGraph = hipGraph on ROCm; every kernel of the forward is enqueued on the capturing stream by the C ABI and
    nothing in it allocates or synchronises) and replayed per image.  Weights are read at replay time, but their PACKED copies
    are made at capture time: re-capture (`.capture()`) after the weights change."""

    def __init__(self, G, shape, device=None):
        self.G = G
        dev = device if device is not None else next(G.parameters()).device
        self.x = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.graph = None
        self.y = None
        self.capture()

    @torch.no_grad()
    def capture(self):
        self.G.eval()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                       # warm-up: packs the weights, fills the allocator pool
                self.G(self.x)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.y = self.G(self.x)

    @torch.no_grad()
    def __call__(self, x):
        self.x.copy_(x)
        self.graph.replay()
        return self.y


def to_uint8_image(x, window=None):
    """[-1,1] NCHW fp32 -> uint8 NHWC as tester.py:70-71 + torchvision.utils.save_image produce it (uegan_quantize_u8).
    window=(H, W): of x[:, :, :H, :W] only, without the copy (uegan_montage_crop_u8 with one image)."""
    if window is not None:
        return montage_u8(x, window=window)
    x = x.detach().contiguous()
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError("to_uint8_image expects a float32 [B,C,H,W] tensor")
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
    _chk(x, y)
    L.check(lib().uegan_quantize_u8(x.data_ptr(), y.data_ptr(), B, C, H, W, _stream()))
    return y


# the launcher's constants (csrc/metrics.hip: MONTAGE_MAX_BLOCKS, MONTAGE_THREADS, MONTAGE_VEC): above MAX_BLOCKS * THREADS work items
# (4 pixels each on the vector path, 1 on the scalar path) the kernels loop by grid stride -- tests/test_montage.py crosses both thresholds
MONTAGE_MAX_BLOCKS, MONTAGE_THREADS, MONTAGE_VEC = 1024, 256, 4
MONTAGE_MAX_IMAGES = 4


def montage_u8(*images, window=None):
    """1..4 float32 [B,C,H,W] images of equal shape -> uint8 [B,H,n*W,C], image k in columns [k*W, (k+1)*W): bit for bit
    `to_uint8_image(torch.cat(images, 3))`, i.e. what `save_image(torch.cat([denorm(a), denorm(b), ...], 3))` writes for the sample and
    compare montages (trainer.py:182-183,244-245, tester.py:73-74), in one launch that reads every source once (uegan_montage_u8).
    window=(H, W): the same of every image's top-left corner, `to_uint8_image(torch.cat([x[:, :, :H, :W] for x in images], 3))`, read in
    place (uegan_montage_crop_u8); a window that does not fit the images raises ValueError."""
    n = len(images)
    if not 1 <= n <= MONTAGE_MAX_IMAGES:
        raise ValueError("montage_u8 takes 1..%d images (got %d)" % (MONTAGE_MAX_IMAGES, n))
    for x in images:
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4:
            raise TypeError("montage_u8 expects float32 [B,C,H,W] tensors")
        if x.shape != images[0].shape or x.device != images[0].device:
            raise ValueError("montage_u8: the images must have one shape and one device (got %s and %s)" % (tuple(images[0].shape), tuple(x.shape)))
    xs = [x.detach().contiguous() for x in images]
    B, C, H, W = xs[0].shape
    if window is not None:
        Hs, Ws = H, W
        H, W = (int(v) for v in window)
        if not (1 <= H <= Hs and 1 <= W <= Ws):
            raise ValueError("montage_u8: the %d x %d window does not fit the %d x %d images" % (H, W, Hs, Ws))
    y = torch.empty((B, H, n * W, C), dtype=torch.uint8, device=xs[0].device)
    _chk(y, *xs)
    if window is not None:
        L.check(lib().uegan_montage_crop_u8(_ptr_table(xs), n, y.data_ptr(), B, C, Hs, Ws, H, W, _stream()))
    else:
        L.check(lib().uegan_montage_u8(_ptr_table(xs), n, y.data_ptr(), B, C, H, W, _stream()))
    return y


def montage_place_u8(dst, images, src_window, dst_origin, panel=None):
    """Quantise the window (sy, sx, h, w) of 1..4 float32 [B,C,Hs,Ws] images straight into the uint8 [B,Hd,Wd,C] image `dst`: image k to rows
    [dy, dy + h) and columns [dx + k*panel, dx + k*panel + w), (dy, dx) = dst_origin, panel = the montage's panel width (default w).  Bit for bit
    `dst[:, dy:dy+h, dx+k*panel:dx+k*panel+w] = to_uint8_image(x_k[:, :, sy:sy+h, sx:sx+w])`; no other byte of dst is written
    (uegan_montage_place_u8).  ValueError before any launch for a window or a destination that does not fit."""
    n = len(images)
    if not 1 <= n <= MONTAGE_MAX_IMAGES:
        raise ValueError("montage_place_u8 takes 1..%d images (got %d)" % (MONTAGE_MAX_IMAGES, n))
    for x in images:
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4:
            raise TypeError("montage_place_u8 expects float32 [B,C,H,W] tensors")
        if x.shape != images[0].shape or x.device != images[0].device:
            raise ValueError("montage_place_u8: the images must have one shape and one device (got %s and %s)" % (tuple(images[0].shape), tuple(x.shape)))
    B, C, Hs, Ws = images[0].shape
    if not torch.is_tensor(dst) or dst.dtype != torch.uint8 or dst.dim() != 4 or dst.shape[0] != B or dst.shape[3] != C or not dst.is_contiguous():
        raise TypeError("montage_place_u8 writes into a contiguous uint8 [B,Hd,Wd,C] image of the sources' batch and channels")
    sy, sx, h, w = (int(v) for v in src_window)
    dy, dx = (int(v) for v in dst_origin)
    panel = w if panel is None else int(panel)
    Hd, Wd = dst.shape[1:3]
    if not (sy >= 0 and sx >= 0 and h >= 1 and w >= 1 and sy + h <= Hs and sx + w <= Ws):
        raise ValueError("montage_place_u8: the %d x %d window at (%d, %d) does not fit the %d x %d images" % (h, w, sy, sx, Hs, Ws))
    if not (dy >= 0 and dx >= 0 and panel >= w and dy + h <= Hd and dx + (n - 1) * panel + w <= Wd):
        raise ValueError("montage_place_u8: %d panels of %d x %d (pitch %d) at (%d, %d) do not fit the %d x %d destination" % (n, h, w, panel, dy, dx, Hd, Wd))
    xs = [x.detach().contiguous() for x in images]
    _chk(dst, *xs)
    L.check(lib().uegan_montage_place_u8(_ptr_table(xs), n, dst.data_ptr(), B, C, Hs, Ws, sy, sx, h, w, Hd, Wd, dy, dx, panel, _stream()))
    return dst


def _tiled_moments(G, hp, wp, core, tile_of):
    """pass 1 of the tiled forward: the attention modules' whole-image moments, from the encoder run over every tile (halo NATIVE_TILE_HALO_ENC);
    tile_of(ty0, ty1, tx0, tx1) -> that tile of the padded image as fp32 NCHW"""
    acc = None
    for cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1 in data.native_tiles(hp, wp, core, data.NATIVE_TILE_HALO_ENC):
        xt = tile_of(ty0, ty1, tx0, tx1)
        if acc is None:
            acc = G.tile_moments_new(xt.shape[0], xt.device)
        G.tile_moments(xt, (cy0 - ty0, cy1 - ty0, cx0 - tx0, cx1 - tx0), acc)
    return [ops.moments_finish(a, (hp >> k) * (wp >> k)) for k, a in enumerate(acc)]


def _check_tiled(G, core, hp, wp):
    """the refusals of the tiled forward, all before any launch -> (models.Tile, core)"""
    from . import models
    if G.training or torch.is_grad_enabled():
        raise RuntimeError("the tiled forward is inference only: G.eval() and torch.no_grad()")
    core = data.check_native_tile(core)
    for tile in data.native_tiles(hp, wp, core, data.NATIVE_TILE_HALO):      # (the largest tiles: pass 1's have the smaller halo)
        data.check_native_size(tile[5] - tile[4], tile[7] - tile[6])
    return models.Tile, core


def enhance_tiled(G, x, core):
    """`enhance(G, x)` evaluated tile by tile: x fp32 [B,3,Hp,Wp] with sides that are multiples of 16 -> G(x), fp32, for an image too large for one
    forward.  Not an approximation: pass 1 runs the encoder over tiles (halo 32) and accumulates the attention modules' moments over
    the whole image (Generator.tile_moments); pass 2 runs the whole network per tile (halo 80, the generator's receptive-field radius 67 on the
    stride-16 grid) with those moments and the image's own up-sampling phase (Generator.forward(tile=)) and keeps each tile's core.  `core`: the
    tiles' core side, a multiple of 16, at least 32; tiles in row-major order.  G in eval mode, under torch.no_grad() (RuntimeError otherwise);
    ValueError before any launch for a bad core or size."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != 3 or x.shape[2] % 16 or x.shape[3] % 16:
        raise ValueError("enhance_tiled expects float32 [B,3,Hp,Wp] with Hp, Wp multiples of 16")
    hp, wp = data.check_native_tiled_size(x.shape[2], x.shape[3])
    Tile, core = _check_tiled(G, core, hp, wp)

    def tile_of(ty0, ty1, tx0, tx1):
        return x[:, :, ty0:ty1, tx0:tx1].contiguous()
    moments = _tiled_moments(G, hp, wp, core, tile_of)
    out = torch.empty_like(x)
    for cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1 in data.native_tiles(hp, wp, core, data.NATIVE_TILE_HALO):
        fake = G(tile_of(ty0, ty1, tx0, tx1), tile=Tile(ty0, tx0, hp, wp, moments))
        out[:, :, cy0:cy1, cx0:cx1] = fake[:, :, cy0 - ty0:cy1 - ty0, cx0 - tx0:cx1 - tx0]
    return out


def _enhance_native_tiled(G, pixels_u8, compare, core):
    if not torch.is_tensor(pixels_u8) or pixels_u8.dtype != torch.uint8 or pixels_u8.dim() != 4 or pixels_u8.shape[3] != 3 or not pixels_u8.is_contiguous():
        raise ValueError("native_input expects a contiguous uint8 [B, h, w, 3] tensor")
    B, h, w, _ = pixels_u8.shape
    hp, wp = data.check_native_tiled_size(h, w)
    G.eval()
    Tile, core = _check_tiled(G, core, hp, wp)

    def tile_of(ty0, ty1, tx0, tx1):
        # (tile origins are multiples of 16: only the last row / column of tiles is ragged, and native_input's extension of those is the image's)
        return data.native_input(pixels_u8[:, ty0:min(ty1, h), tx0:min(tx1, w)].contiguous())
    moments = _tiled_moments(G, hp, wp, core, tile_of)
    q = torch.empty((B, h, w, 3), dtype=torch.uint8, device=pixels_u8.device)
    pair = torch.empty((B, h, 2 * w, 3), dtype=torch.uint8, device=pixels_u8.device) if compare else None
    for cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1 in data.native_tiles(hp, wp, core, data.NATIVE_TILE_HALO):
        xt = tile_of(ty0, ty1, tx0, tx1)
        fake = G(xt, tile=Tile(ty0, tx0, hp, wp, moments))
        win = (cy0 - ty0, cx0 - tx0, min(cy1, h) - cy0, min(cx1, w) - cx0)
        montage_place_u8(q, [fake], win, (cy0, cx0))
        if compare:
            montage_place_u8(pair, [xt, fake], win, (cy0, cx0), panel=w)
    return (q, pair) if compare else q


def enhance_native(G, pixels_u8, compare=False, tile=None):
    """An image at its own size: uint8 [B,h,w,3] on the device (decoded RGB, both sides >= 32) -> the enhanced uint8 [B,h,w,3]; compare=True:
    also the raw | enhanced montage uint8 [B,h,2w,3] (tester.py:73-74).  The mode is DEFINED as

        crop(G(reflect_extend(normalise(pixels))))

    normalise = ToTensor + Normalize(0.5, 0.5); reflect_extend = reflection at the bottom and right up to the next multiples of 16 (the
    generator's four stride-2 stages), both in one pass (data.native_input); crop = the top-left h x w window, cut during the 8-bit
    quantisation (uegan_montage_crop_u8).  Bit for bit `to_uint8_image(enhance(G, F.pad(data.input_transform(pixels, (h, w)), (0, wp - w, 0,
    hp - h), mode="reflect")))[:, :h, :w]` in every storage mode.  One consequence: the attention modules' global moments are taken over the
    extended image, so they include its up-to-15 reflected rows and columns (masked moments are not implemented).  The forward is eager
    (there is no hipGraph per padded shape).  ValueError before any launch: a side below 32, a padded area above data.NATIVE_MAX_PIXELS
    per image, anything but a contiguous uint8 [B,h,w,3] tensor.

    tile=T (a multiple of 16, at least 32): the same definition evaluated tile by tile, for images above that cap (up to
    data.NATIVE_TILED_MAX_PIXELS): two passes over uint8 tiles of core T -- see enhance_tiled, of which this is bit for bit
    `to_uint8_image(enhance_tiled(G, data.native_input(pixels), T), window=(h, w))` without ever holding the image in fp32: every tile is cut from
    the bytes, and its core is quantised straight into the full-size result (montage_place_u8).  Nothing synchronises with the host between tiles."""
    if tile is not None:
        with torch.no_grad():
            return _enhance_native_tiled(G, pixels_u8, compare, tile)
    x = data.native_input(pixels_u8)
    h, w = pixels_u8.shape[1:3]
    fake = enhance(G, x)
    q = to_uint8_image(fake, window=(h, w))
    if not compare:
        return q
    return q, montage_u8(x, fake, window=(h, w))


PNG_ENCODERS = ("pillow", "device")
_png_encoder = "pillow"


def set_png_encoder(name):
    """who encodes the PNG files write_pngs writes: "pillow" (the default; files as before) or "device" (codecs.png_encode: same pixels, another
    deflate stream).  Anything else: ValueError."""
    global _png_encoder
    if name not in PNG_ENCODERS:
        raise ValueError("unknown PNG encoder %r (one of %s)" % (name, ", ".join(PNG_ENCODERS)))
    _png_encoder = name


def get_png_encoder():
    return _png_encoder


def write_pngs(paths, images_u8):
    """images_u8: uint8 [B,H,W,3] on the device; image i goes to paths[i] as an 8-bit RGB PNG (what save_image writes), encoded by the selected
    encoder.  Both encoders' files decode to the same pixels."""
    paths = list(paths)
    if len(paths) != images_u8.shape[0]:
        raise ValueError("write_pngs: %d paths for %d images" % (len(paths), images_u8.shape[0]))
    if _png_encoder == "device":
        for path, blob in zip(paths, codecs.png_encode(images_u8.contiguous())):
            with open(path, "wb") as f:
                f.write(blob)
        return
    from PIL import Image
    host = images_u8.cpu().numpy()
    for i, path in enumerate(paths):
        Image.fromarray(host[i], "RGB").save(path)


IMAGE_FORMATS = ("png", "jpeg")
_image_format = ("png", 95, "4:4:4")
_jpeg_optimize = False


def set_image_format(name, quality=95, subsampling="4:4:4", optimize=False):
    """the container write_images writes: "png" (the default: write_pngs, every file name and byte as before) or "jpeg" (codecs.jpeg_encode with this
    quality, 1..100, and subsampling, "4:4:4" or "4:2:0": baseline JPEG files named .jpg, always encoded on the device -- there is no Pillow arm,
    and the PNG encoder selection does not matter to it).  optimize (a bool; "jpeg" only): every file carries its own Huffman tables, built on the
    device from its symbol counts, instead of the standard ones: the same pixels in a smaller file.  Anything else: ValueError, and the selection
    stays."""
    global _image_format, _jpeg_optimize
    if name not in IMAGE_FORMATS:
        raise ValueError("unknown image format %r (one of %s)" % (name, ", ".join(IMAGE_FORMATS)))
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("JPEG quality %r is not an integer in [1, 100]" % (quality,))
    if subsampling not in codecs.JPEG_SUBSAMPLINGS:
        raise ValueError("JPEG subsampling %r is not one of %s" % (subsampling, ", ".join(codecs.JPEG_SUBSAMPLINGS)))
    if not isinstance(optimize, bool):
        raise ValueError("JPEG optimize %r is not a bool" % (optimize,))
    if optimize and name != "jpeg":
        raise ValueError("optimize=True needs the \"jpeg\" format, not %r" % (name,))
    _image_format = (name, quality, subsampling)
    _jpeg_optimize = optimize


def get_image_format():
    """(name, quality, subsampling) as set_image_format took them; quality and subsampling only matter to the "jpeg" format"""
    return _image_format


def get_jpeg_optimize():
    """whether write_images asks the "jpeg" format for per-image Huffman tables (set_image_format's optimize; False after any other selection)"""
    return _jpeg_optimize


def image_path(path):
    """the name write_images gives the file asked for as `path`: the same for "png"; for "jpeg" a .png suffix becomes .jpg"""
    if _image_format[0] == "jpeg" and path.endswith(".png"):
        return path[:-4] + ".jpg"
    return path


def write_images(paths, images_u8):
    """write_pngs by the selected format (set_image_format): image i goes to image_path(paths[i]).  Returns the paths actually written."""
    paths = list(paths)
    name, quality, subsampling = _image_format
    if name == "png":
        write_pngs(paths, images_u8)
        return paths
    if len(paths) != images_u8.shape[0]:
        raise ValueError("write_images: %d paths for %d images" % (len(paths), images_u8.shape[0]))
    written = [image_path(p) for p in paths]
    for path, blob in zip(written, codecs.jpeg_encode(images_u8.contiguous(), quality, subsampling, optimize=_jpeg_optimize)):
        with open(path, "wb") as f:
            f.write(blob)
    return written


def _as_stack(img):
    if img.dtype != torch.uint8:
        raise TypeError("metrics take uint8 HWC / BHWC images (to_uint8_image)")
    return (img.unsqueeze(0) if img.dim() == 3 else img).contiguous()


def _metrics(img1, img2, crop_border, want_sq, want_ssim):
    a, b = _as_stack(img1), _as_stack(img2)
    if a.shape != b.shape:
        raise ValueError("Input images must have the same dimensions.")
    B, H, W, C = a.shape
    sq = torch.empty((B,), dtype=torch.float64, device=a.device) if want_sq else None
    ss = torch.empty((B,), dtype=torch.float64, device=a.device) if want_ssim else None
    _chk(a, b)
    L.check(lib().uegan_image_metrics_u8(a.data_ptr(), b.data_ptr(), _p(sq), _p(ss), B, H, W, C, crop_border, _stream()))
    h, w = H - 2 * crop_border, W - 2 * crop_border
    return sq, ss, h * w * C, (h - 6) * (w - 6) * C


def calculate_psnr(img1, img2, crop_border=CROP_BORDER):
    """metrics/CalcPSNR.py:85-92 on uint8 HWC images (or a BHWC stack -> list) after the border crop of :24,56."""
    sq, _, n, _ = _metrics(img1, img2, crop_border, True, False)
    out = []
    for v in sq.tolist():
        mse = v / n
        out.append(float("inf") if mse == 0 else 10 * math.log10(255.0 ** 2 / mse))
    return out[0] if img1.dim() == 3 else out


def calculate_ssim(img1, img2, crop_border=CROP_BORDER):
    """metrics/CalcSSIM.py:63: skimage structural_similarity(multichannel=True, data_range=255) with its defaults (7x7 uniform
    window, K1 0.01, K2 0.03, sample covariance) on the border-cropped uint8 images."""
    _, ss, _, n = _metrics(img1, img2, crop_border, False, True)
    out = [v / n for v in ss.tolist()]
    return out[0] if img1.dim() == 3 else out


def mean_metric(values):
    """True mean over a test set.  (The reference's directory loops return total / i with i = N - 1: CalcPSNR.py:77, CalcSSIM.py:75.)"""
    values = list(values)
    return sum(values) / len(values)


def run_test(G, loader, save_dir=None, tag="0.00", metrics=True, nima=None, suffix="testFakeExp", compare_dir=None,
             compare_suffix="testRealRaw_testFakeExp", native_tile=None):
    """Tester.test (tester.py:40-105) over a `uegan_amd.data` test loader: `G.eval()` forward per batch (:64-67), the enhanced image of
    every sample as `<name>_<tag>_<suffix>.png` in `save_dir` (:69-71: the 8-bit image torchvision's save_image writes; None: no
    files), and -- what calc_psnr / calc_ssim then compute from those files against the label images (:96-103) -- PSNR and SSIM of
    each enhanced image against `img_exp`, here straight from the device tensors.  Returns {"names", "psnr", "ssim", "mean_psnr",
    "mean_ssim"} (true means).

    Native mode (a `data.get_test_loader(root, 0)` loader, whose batches hold the decoded files as uint8 lists): every sample goes through
    `enhance_native` at its own size, the PNGs have the size of their source, the result gains "sizes" ([h, w] per image), and PSNR / SSIM
    compare against the label FILE's own pixels -- what calc_psnr / calc_ssim read; a label of another size than its raw image raises
    ValueError naming both files (CalcPSNR.py:87 raises on it too).  The restriction below is that of the resizing mode only.  A sample whose
    padded area exceeds data.NATIVE_MAX_PIXELS is enhanced tile by tile (`enhance_native(tile=data.NATIVE_TILE)`); native_tile=T: every sample is,
    with core T.

    Restriction: the label here is the loader's `img_exp` -- the label FILE resized to the test size by the loader's transform
    (data_loader.py:95-99) and re-quantised to 8 bits -- whereas calc_psnr / calc_ssim read the ORIGINAL files of test_label_dir.  The
    numbers agree with the reference's when the label files already have the test size (the reference itself needs equal shapes:
    CalcPSNR.py:87 raises otherwise); for labels of another size decode them yourself and call calculate_psnr / calculate_ssim.

    compare_dir: also write the raw image and the enhanced one side by side (tester.py:73-74; `montage_u8`) as
    `<name>_<tag>_<compare_suffix>.png` there.  Validation passes suffix="valFakeExp", compare_suffix="valRealRaw_valFakeExp" (trainer.py:242,245).

    nima: a `uegan_amd.nima.NIMA` module -> also "nima" / "nima_std" (per image) and "mean_nima" (true mean): what calc_nima (tester.py:91-94,
    on by default in the reference: config.py:80) computes from the saved files, here from the same 8-bit images on the device.  It needs no
    label: with metrics=False the loader's `img_exp` is never touched (the unpaired setting).

    The files go through `write_images`: with set_image_format("jpeg", ...) they are baseline JPEGs named `.jpg` instead of `.png`.  NIMA, PSNR and
    SSIM are computed from the device's 8-bit tensor BEFORE it is encoded, whatever the format: with JPEG the numbers describe the enhanced
    pixels, not the lossy file, and equal those of a PNG run."""
    rec = _TestRecord(metrics, nima, save_dir, compare_dir, tag, suffix, compare_suffix)
    for batch in loader:
        if isinstance(batch.img_raw, (list, tuple)):      # native mode: the samples one by one, since their sizes may differ
            if metrics:                                   # (before any launch)
                for i, (raw, lab) in enumerate(zip(batch.img_raw, batch.img_exp)):
                    if lab.shape != raw.shape:
                        raise ValueError("Input images must have the same dimensions: label %s, raw %s are %d x %d and %d x %d"
                                         % (batch.paths[i] + (lab.shape[1], lab.shape[2], raw.shape[1], raw.shape[2])))
            for i, name in enumerate(batch.img_name):
                raw = batch.img_raw[i]
                hp, wp = data.padded_size(raw.shape[1], raw.shape[2])
                core = native_tile if native_tile is not None else (data.NATIVE_TILE if hp * wp > data.NATIVE_MAX_PIXELS else None)
                res = enhance_native(G, raw, compare=compare_dir is not None, tile=core)
                q, pair = res if compare_dir is not None else (res, None)
                rec.add([name], q, pair, batch.img_exp[i] if metrics else None)
                rec.sizes.append([int(raw.shape[1]), int(raw.shape[2])])
            continue
        fake = enhance(G, batch.img_raw)
        q = to_uint8_image(fake)
        pair = montage_u8(batch.img_raw, fake) if compare_dir is not None else None
        rec.add(list(batch.img_name), q, pair, to_uint8_image(batch.img_exp) if metrics else None)
    return rec.result()


class _TestRecord:
    """what run_test does with the 8-bit images of one batch, whichever mode produced them: PSNR / SSIM against the 8-bit labels, NIMA, the PNGs"""

    def __init__(self, metrics, nima, save_dir, compare_dir, tag, suffix, compare_suffix):
        import os
        self.metrics, self.nima, self.tag = metrics, nima, tag
        self.dirs = ((save_dir, suffix), (compare_dir, compare_suffix))
        self.names, self.psnr, self.ssim, self.nima_mean, self.nima_std, self.sizes = [], [], [], [], [], []
        for d, _ in self.dirs:
            if d is not None:
                os.makedirs(d, exist_ok=True)

    def add(self, names, q, pair, ref):
        """q: enhanced uint8 [B,H,W,3]; pair: the raw | enhanced montage or None; ref: the labels as uint8 [B,H,W,3] or None"""
        import os
        if ref is not None:
            self.psnr += calculate_psnr(q, ref)
            self.ssim += calculate_ssim(q, ref)
        if self.nima is not None:
            from . import nima as nima_mod
            m, d = nima_mod.score(self.nima, q)
            self.nima_mean += m
            self.nima_std += d
        self.names += names
        for (d, suffix), images in zip(self.dirs, (q, pair)):
            if d is not None and images is not None:
                write_images([os.path.join(d, "%s_%s_%s.png" % (name, self.tag, suffix)) for name in names], images)

    def result(self):
        out = {"names": self.names, "psnr": self.psnr, "ssim": self.ssim}
        if self.sizes:
            out["sizes"] = self.sizes
        if self.metrics and self.names:
            out["mean_psnr"], out["mean_ssim"] = mean_metric(self.psnr), mean_metric(self.ssim)
        if self.nima is not None:
            out["nima"], out["nima_std"] = self.nima_mean, self.nima_std
            if self.names:
                out["mean_nima"] = mean_metric(self.nima_mean)
        return out
