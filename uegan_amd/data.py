"""Input pipeline with the transform ON THE DEVICE: the reference's data_loader.py restated so that the host
only decodes files and copies raw bytes, and everything torchvision does per pixel runs in uegan_input_transform.

  reference (data_loader.py)                               here
  ---------------------------------------------------     ------------------------------------------------------------------
  ReferenceDataset / DefaultDataset  (:21-71)               same names: file listing + pairing only (no transform argument)
  transforms.RandomCrop(img_size)    (:75)                  the crop window is what gets copied: host memcpy of its rows into a
                                                            pinned batch buffer, one H2D copy per batch on a side stream
  Resize / flips / ToTensor / Normalize (:76-81, :97-100)   uegan_input_transform (csrc/input.hip), bit-exact with Pillow's resampler
  DataLoader(pin_memory=True) + InputFetcher (:85-90,       DeviceLoader: decode threads -> pinned ring -> side-stream H2D + transform,
      :113-133: `.to(device)` on the training stream)       `prefetch` batches ahead; the training stream only waits on an event

  (nothing: every epoch decodes every file again)           cache="device" (opt-in): the decoded files stay in device memory from their first touch
                                                            on (_ResidentStore) and uegan_input_transform_windows cuts the crops out of them in place

Random draws follow torchvision's call order per image (RandomCrop.get_params: randint for the top row, randint for the left
column -- none when the image already has the crop size; then one torch.rand(1) < 0.5 per flip), img_exp before img_raw as
ReferenceDataset.__getitem__ transforms them (:63-65), and torch.randperm for the shuffle.  With DataLoader worker processes the
reference's own streams are per-worker and not reproducible, so this order is a convention, not a parity claim (torchvision is not
in this image: unpinned); the PIXEL arithmetic is pinned against Pillow itself (tests/test_data.py).
"""
import collections
import concurrent.futures
import math
import os
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .ops.core import _p, lib

_EXTS = ("png", "jpg", "jpeg", "JPG")
PRECISION_BITS = 32 - 8 - 2           # Pillow, src/libImaging/Resample.c (8-bit channels)
MAX_IMAGES_PER_CALL = 64


# --------------------------------------------------------------------------------------------------------------------
# Pillow's coefficient tables (Resample.c: precompute_coeffs + normalize_coeffs_8bpc) for the BILINEAR (triangle) filter
# --------------------------------------------------------------------------------------------------------------------
def _triangle(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def resample_table(in_size, out_size):
    """int32 [out_size, 2 + k]: per output index (first input index, tap count, k fixed-point coefficients), and k.
    Python floats are C doubles and the operations are in Pillow's order, so the integers are Pillow's."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale                      # bilinear: filter support 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    tab = np.zeros((out_size, 2 + ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)           # C (int) cast: truncation
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        k = [_triangle((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        tab[xx, 0], tab[xx, 1] = xmin, n
        for x, w in enumerate(k):
            tab[xx, 2 + x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
    return tab, ksize


_TABLES = {}


def _device_table(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _TABLES:
        tab, k = resample_table(in_size, out_size)
        _TABLES[key] = (torch.from_numpy(tab).to(device), k)
    return _TABLES[key]


def input_transform(pixels, out_size, flips=None, out=None, stream=None):
    """pixels: uint8 [B, h, w, 3] on the device (decoded RGB crop windows) -> fp32 [B, 3, out_h, out_w] in [-1, 1]:
    Resize(out_size) + flips (bit 0 horizontal, bit 1 vertical, per image) + ToTensor + Normalize(0.5, 0.5)."""
    if pixels.dtype != torch.uint8 or pixels.dim() != 4 or pixels.shape[3] != 3 or not pixels.is_contiguous():
        raise ValueError("input_transform expects a contiguous uint8 [B, h, w, 3] tensor")
    B, h, w, _ = pixels.shape
    oh, ow = (out_size, out_size) if isinstance(out_size, int) else out_size
    dev = pixels.device
    htab, hk = _device_table(w, ow, dev)
    vtab, vk = _device_table(h, oh, dev)
    if out is None:
        out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev)
    if stream is None and not L.is_emulated():
        stream = torch.cuda.current_stream().cuda_stream
    for b0 in range(0, B, MAX_IMAGES_PER_CALL):
        nb = min(MAX_IMAGES_PER_CALL, B - b0)
        tmp = torch.empty((nb, h, ow, 3), dtype=torch.uint8, device=dev)
        fl = None
        if flips is not None:
            fl = (L.C.c_int32 * nb)(*[int(f) for f in flips[b0:b0 + nb]])
        L.check(lib().uegan_input_transform(_p(pixels[b0:]), nb, h, w, oh, ow, _p(htab), hk, _p(vtab), vk, fl, _p(tmp), _p(out[b0:]), stream))
    return out


def input_transform_windows(images, windows, win, out_size, flips=None, out=None, stream=None):
    """input_transform of crop windows that are read IN PLACE out of images resident on the device (uegan_input_transform_windows): images is a list
    of uint8 [H_i, W_i, 3] device tensors -- sizes may differ, and a tensor may be a view with a row pitch (`big[:, 3:36]`): only its pixels have to
    be contiguous; windows the list of (top, left), one per image; win the window's (h, w) or one int for both.  -> fp32 [B, 3, out_h, out_w], bit for
    bit `input_transform(torch.stack([im[t:t + h, l:l + w] for ...]), out_size, flips)`.  A window that leaves its image is refused by the launcher
    (RuntimeError) before anything of its call is launched."""
    wh, ww = (win, win) if isinstance(win, int) else win
    oh, ow = (out_size, out_size) if isinstance(out_size, int) else out_size
    B = len(images)
    if B < 1 or len(windows) != B or (flips is not None and len(flips) != B):
        raise ValueError("input_transform_windows expects one (top, left) per image (and one flip code, if any), at least one image")
    dev = images[0].device
    for im in images:
        if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.device != dev or im.numel() == 0 or \
                im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) % 3 or im.stride(0) < 3 * im.shape[1]:
            raise ValueError("input_transform_windows expects uint8 [H, W, 3] tensors on one device whose pixels are contiguous (rows may have a pitch)")
    if not L.is_emulated() and not dev.type == "cuda":
        raise RuntimeError("uegan_amd ops need CUDA/HIP tensors (there is no CPU path)")
    htab, hk = _device_table(ww, ow, dev)
    vtab, vk = _device_table(wh, oh, dev)
    if out is None:
        out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev)
    if stream is None and not L.is_emulated():
        stream = torch.cuda.current_stream().cuda_stream
    for b0 in range(0, B, MAX_IMAGES_PER_CALL):
        nb = min(MAX_IMAGES_PER_CALL, B - b0)
        tmp = torch.empty((nb, wh, ow, 3), dtype=torch.uint8, device=dev)
        desc = (L.Window * nb)()
        for i in range(nb):
            im, (top, left) = images[b0 + i], windows[b0 + i]
            desc[i] = L.Window(im.data_ptr(), im.stride(0) // 3, int(top), int(left), int(flips[b0 + i]) if flips is not None else 0, im.shape[0], im.shape[1])
        L.check(lib().uegan_input_transform_windows(desc, nb, wh, ww, oh, ow, _p(htab), hk, _p(vtab), vk, _p(tmp), _p(out[b0:]), stream))
    return out


# --------------------------------------------------------------------------------------------------------------------
# native size: no resize, the image extended by reflection to the multiples of 16 the generator needs
# --------------------------------------------------------------------------------------------------------------------
NATIVE_MULTIPLE = 16                  # Generator.forward: four stride-2 stages
NATIVE_MIN_SIDE = 32
# per-image cap of the padded area.  8 * 1024^2 is the per-launch element count the suite has run the generator at (8 x 3 x 1024^2): a statement
# of what has been exercised, not a measured limit
NATIVE_MAX_PIXELS = 8 * 1024 * 1024
# Above the cap an image is enhanced tile by tile (tester.enhance_native(tile=)): cores of NATIVE_TILE pixels a side, each run with a
# halo -- the receptive-field radius of the network behind the point where the tiles are joined, rounded up to the stride-16 grid: 67 -> 80 input
# pixels for the whole generator (pass 2), 18 -> 32 for the encoder (pass 1, which collects the attention modules' whole-image moments).
NATIVE_TILE = 1024
NATIVE_TILE_HALO = 80
NATIVE_TILE_HALO_ENC = 32
# the largest image tools/bench_tiled.py has run on the GPU (4096 x 6144, profiles/tiled_bench.json): as above, what has been exercised
NATIVE_TILED_MAX_PIXELS = 4096 * 6144
# the launcher's constants (csrc/input.hip: NATIVE_MAX_BLOCKS, NATIVE_THREADS, NATIVE_VEC): above MAX_BLOCKS * THREADS groups of VEC output
# pixels the kernel loops by grid stride -- tests/test_native.py crosses the threshold on both read paths
NATIVE_MAX_BLOCKS, NATIVE_THREADS, NATIVE_VEC = 2048, 256, 4


def padded_size(h, w):
    """(hp, wp): the next multiples of 16 of an h x w image, the size the generator runs at in native mode"""
    m = NATIVE_MULTIPLE
    return (int(h) + m - 1) // m * m, (int(w) + m - 1) // m * m


def check_native_size(h, w):
    """raise ValueError unless an h x w image can be enhanced at its own size: both sides >= 32, padded area <= NATIVE_MAX_PIXELS.  Returns (hp, wp)."""
    if h < NATIVE_MIN_SIDE or w < NATIVE_MIN_SIDE:
        raise ValueError("native-size inference needs both sides >= %d (got %d x %d)" % (NATIVE_MIN_SIDE, h, w))
    hp, wp = padded_size(h, w)
    if hp * wp > NATIVE_MAX_PIXELS:
        raise ValueError("native-size inference: %d x %d pads to %d x %d = %d pixels, above the %d this package has been exercised at"
                         % (h, w, hp, wp, hp * wp, NATIVE_MAX_PIXELS))
    return hp, wp


def check_native_tile(core):
    """raise ValueError unless `core` is a usable tile core: a multiple of 16, at least 32"""
    if int(core) != core or core % NATIVE_MULTIPLE or core < NATIVE_MIN_SIDE:
        raise ValueError("tiled native-size inference needs a tile core that is a multiple of %d and at least %d (got %r)"
                         % (NATIVE_MULTIPLE, NATIVE_MIN_SIDE, core))
    return int(core)


def check_native_tiled_size(h, w):
    """check_native_size for an image that is enhanced tile by tile: both sides >= 32, padded area <= NATIVE_TILED_MAX_PIXELS.  Returns (hp, wp)."""
    if h < NATIVE_MIN_SIDE or w < NATIVE_MIN_SIDE:
        raise ValueError("native-size inference needs both sides >= %d (got %d x %d)" % (NATIVE_MIN_SIDE, h, w))
    hp, wp = padded_size(h, w)
    if hp * wp > NATIVE_TILED_MAX_PIXELS:
        raise ValueError("tiled native-size inference: %d x %d pads to %d x %d = %d pixels, above the %d this package has been exercised at"
                         % (h, w, hp, wp, hp * wp, NATIVE_TILED_MAX_PIXELS))
    return hp, wp


def native_tiles(hp, wp, core, halo):
    """the tiles of an hp x wp image (multiples of 16) in row-major order: (cy0, cy1, cx0, cx1, ty0, ty1, tx0, tx1) -- the core, which the tile
    accounts for, and the tile itself: the core extended by `halo` and clipped to the image, so that a tile edge at the image's border IS the
    image's edge and the convolutions' own reflection there is the right one"""
    out = []
    for cy0 in range(0, hp, core):
        cy1 = min(cy0 + core, hp)
        for cx0 in range(0, wp, core):
            cx1 = min(cx0 + core, wp)
            out.append((cy0, cy1, cx0, cx1, max(cy0 - halo, 0), min(cy1 + halo, hp), max(cx0 - halo, 0), min(cx1 + halo, wp)))
    return out


def native_input(pixels):
    """pixels: uint8 [B, h, w, 3] on the device (decoded RGB images) -> fp32 [B, 3, hp, wp] in [-1, 1], (hp, wp) = padded_size(h, w):
    ToTensor + Normalize(0.5, 0.5) and the reflection extension at the bottom and right in one pass (uegan_native_input) -- bit for bit
    `F.pad(input_transform(pixels, (h, w)), (0, wp - w, 0, hp - h), mode="reflect")`; the image itself is out[:, :, :h, :w]."""
    if not torch.is_tensor(pixels) or pixels.dtype != torch.uint8 or pixels.dim() != 4 or pixels.shape[3] != 3 or not pixels.is_contiguous():
        raise ValueError("native_input expects a contiguous uint8 [B, h, w, 3] tensor")
    B, h, w, _ = pixels.shape
    hp, wp = check_native_size(h, w)
    if B < 1:
        raise ValueError("native_input: empty batch")
    if not L.is_emulated() and not pixels.is_cuda:
        raise RuntimeError("uegan_amd ops need CUDA/HIP tensors (there is no CPU path)")
    out = torch.empty((B, 3, hp, wp), dtype=torch.float32, device=pixels.device)
    stream = None if L.is_emulated() else torch.cuda.current_stream().cuda_stream
    L.check(lib().uegan_native_input(_p(pixels), B, h, w, hp, wp, _p(out), stream))
    return out


# --------------------------------------------------------------------------------------------------------------------
# datasets: file listing only
# --------------------------------------------------------------------------------------------------------------------
def listdir(dname):
    """every image file below dname (data_loader.py:14-17: recursive, extension groups in this order)"""
    out = []
    for ext in _EXTS:
        out.extend(Path(dname).rglob("*." + ext))
    return out


class DefaultDataset:
    """sorted image files of one folder (data_loader.py:21-36)"""

    def __init__(self, root):
        self.samples = sorted(listdir(root))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        return self.samples[index]


class ReferenceDataset:
    """pairs (file of the first sub-folder, file of the second) in listing order (data_loader.py:39-71); the sample name is the
    second file's path up to its first '.', after its last '/' (:58-60)"""

    def __init__(self, root):
        firsts, seconds = [], []
        for idx, domain in enumerate(sorted(os.listdir(root))):
            files = listdir(os.path.join(root, domain))
            if idx == 0:
                firsts += files
            elif idx == 1:
                seconds += files
        self.samples = list(zip(firsts, seconds))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        a, b = self.samples[index]
        stem = str(b).split(".", 1)[0]
        return a, b, stem.rsplit("/", 1)[1]


# --------------------------------------------------------------------------------------------------------------------
# the loader
# --------------------------------------------------------------------------------------------------------------------
def draw_train_params(h, w, crop, generator=None):
    """(top, left, flip bits) in torchvision's draw order for RandomCrop -> RandomHorizontalFlip -> RandomVerticalFlip"""
    if h < crop or w < crop:
        raise ValueError("Required crop size (%d, %d) is larger than input image size (%d, %d)" % (crop, crop, h, w))
    if h == crop and w == crop:
        top = left = 0
    else:
        top = int(torch.randint(0, h - crop + 1, size=(1,), generator=generator).item())
        left = int(torch.randint(0, w - crop + 1, size=(1,), generator=generator).item())
    bits = 0
    if float(torch.rand(1, generator=generator)) < 0.5:
        bits |= 1
    if float(torch.rand(1, generator=generator)) < 0.5:
        bits |= 2
    return top, left, bits


Batch = collections.namedtuple("Batch", ["img_exp", "img_raw", "img_name"])
# a batch of the native mode (get_test_loader(img_size=0)): img_exp / img_raw are LISTS of uint8 [1,h,w,3] device tensors, one per sample (the
# decoded files, nothing resized; sizes may differ within a batch), paths the (label file, raw file) pair of each sample
NativeBatch = collections.namedtuple("NativeBatch", ["img_exp", "img_raw", "img_name", "paths"])


class _Slot:
    """one batch in flight: a pinned byte buffer (thread workers) or a shared-memory segment registered with the HIP runtime
    (process workers), its device mirror, the decode futures and the 'ready' event"""

    def __init__(self):
        self.host = None
        self.dev = None
        self.shm = None
        self.registered = False
        self.futures = []
        self.items = None
        self.ready = None
        self.out = None
        self.copied = None

    def ensure(self, nbytes, device, pinned, shared, mirror=True):
        """mirror=False: no device copy of the buffer (the native mode uploads every batch into a buffer of its own)"""
        if self.host is not None and self.host.numel() >= nbytes:
            return
        if shared:
            from multiprocessing import shared_memory
            self.release()
            self.shm = shared_memory.SharedMemory(create=True, size=max(nbytes, 1 << 20))
            self.host = torch.frombuffer(self.shm.buf, dtype=torch.uint8)
            if pinned:       # page-lock the segment so that the H2D copy is a DMA straight out of what the workers wrote
                self.registered = int(torch.cuda.cudart().cudaHostRegister(self.host.data_ptr(), self.host.numel(), 0)) == 0
        else:
            self.host = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=pinned)
        self.dev = torch.empty((self.host.numel(),), dtype=torch.uint8, device=device) if mirror else None

    def release(self):
        if self.shm is not None:
            if self.registered:
                torch.cuda.cudart().cudaHostUnregister(self.host.data_ptr())
                self.registered = False
            self.host = None
            try:
                self.shm.close()
                self.shm.unlink()
            except (BufferError, FileNotFoundError):
                pass
            self.shm = None


_ATTACHED = {}


def _shm_view(name, off, h, w):
    """worker process: numpy view of one window inside the named shared-memory segment (segments stay attached per process)"""
    from multiprocessing import shared_memory
    if name not in _ATTACHED:
        if len(_ATTACHED) > 16:
            for old in list(_ATTACHED.values()):
                old.close()
            _ATTACHED.clear()
        _ATTACHED[name] = shared_memory.SharedMemory(name=name)
    return np.ndarray((h, w, 3), dtype=np.uint8, buffer=_ATTACHED[name].buf, offset=off)


def _worker_decode(name, off, path, top, left, h, w, whole):
    dst = _shm_view(name, off, h, w)
    if whole:
        _decode_whole(path, dst)
    else:
        _decode_window(path, top, left, h, w, dst)
    return None


def _decode_window(path, top, left, h, w, dst):
    from PIL import Image
    with Image.open(path) as im:
        im.load()                                            # the decoder runs without the GIL
        win = im.crop((left, top, left + w, top + h))        # only the window goes through the mode conversion and the copies
        if win.mode != "RGB":
            win = win.convert("RGB")
        dst[...] = np.asarray(win)


def _decode_whole(path, dst):
    from PIL import Image
    with Image.open(path) as im:
        dst[...] = np.asarray(im.convert("RGB"))


# who decodes the input files: "host" (Pillow in the workers, the pixels copied up) or "device" (the workers read the files' bytes and parse their
# headers; codecs.jpeg_decode_into decodes baseline JPEG files on the loader's side stream; any other file takes the Pillow route, one by one)
INPUT_DECODERS = ("host", "device")
_input_decoder = "host"


def set_input_decoder(name):
    """the decoder of the loaders created from now on without a `decode` of their own: "host" (default) or "device"; returns the previous one"""
    global _input_decoder
    if name not in INPUT_DECODERS:
        raise ValueError("unknown input decoder %r (one of %s)" % (name, ", ".join(INPUT_DECODERS)))
    prev, _input_decoder = _input_decoder, name
    return prev


def get_input_decoder():
    return _input_decoder


# where the decoded files live between their touches: "none" (nowhere: every touch decodes the file again) or "device" (the whole decoded image stays
# in device memory from its first touch on, and a batch is cut out of the resident images by uegan_input_transform_windows: _ResidentStore)
DATASET_CACHES = ("none", "device")
DATASET_CACHE_DEFAULT_BYTES = 16 << 30      # per loader.  A setting, not a measurement: FiveK as the reference ships it decodes to about 11 GB
_dataset_cache = "none"
_dataset_cache_bytes = DATASET_CACHE_DEFAULT_BYTES


def _cache_budget(gigabytes):
    try:
        ok = not isinstance(gigabytes, bool) and math.isfinite(float(gigabytes)) and float(gigabytes) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("dataset cache budget %r: expected a positive number of gigabytes" % (gigabytes,))
    return int(float(gigabytes) * (1 << 30))


def set_dataset_cache(name, gigabytes=None):
    """the dataset cache of the loaders created from now on without a `cache` of their own: "none" (default) or "device", and the budget of "device"
    per loader in GiB (default 16); returns the previous name"""
    global _dataset_cache, _dataset_cache_bytes
    if name not in DATASET_CACHES:
        raise ValueError("unknown dataset cache %r (one of %s)" % (name, ", ".join(DATASET_CACHES)))
    if gigabytes is not None and name != "device":
        raise ValueError("a dataset cache budget (%r GiB) needs the dataset cache 'device'" % (gigabytes,))
    budget = DATASET_CACHE_DEFAULT_BYTES if gigabytes is None else _cache_budget(gigabytes)
    prev, _dataset_cache, _dataset_cache_bytes = _dataset_cache, name, budget
    return prev


def get_dataset_cache():
    return _dataset_cache


class _Entry:
    """one resident image: `pixels` a uint8 [H, W, 3] view into a chunk of the store; `filled` once its decode or copy has been enqueued on the
    loader's side stream, `pending` the pass (DeviceLoader.__iter__) whose earlier batch will do that"""
    __slots__ = ("pixels", "filled", "pending")

    def __init__(self, pixels):
        self.pixels, self.filled, self.pending = pixels, False, -1


class _ResidentStore:
    """Decoded images kept in device memory, keyed by path: whole RGB images as uint8 [H][W][3], bump-allocated at 16-byte boundaries out of large
    chunks.  No eviction: an epoch is a permutation, every file is used once per epoch, so a least-recently-used policy would evict each entry just
    before its reuse; a static resident set hits for exactly its share of the files.  The first image that does not fit the budget is declined and so
    is every later one.  The budget bounds the chunks' bytes; nothing is freed before close()."""
    CHUNK_BYTES = 256 << 20

    def __init__(self, budget, device, side):
        self.budget, self.device, self.side = int(budget), device, side
        self.chunks, self.cursor, self.reserved, self.used, self.full = [], 0, 0, 0, False
        self.entries = {}

    def _chunk(self, nbytes):
        if self.side is None:
            return torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        with torch.cuda.stream(self.side):      # the chunk belongs to the stream that writes and reads it
            return torch.empty((nbytes,), dtype=torch.uint8, device=self.device)

    def allocate(self, key, h, w):
        """-> the new _Entry of an h x w image, or None: declined (from then on every allocation is)"""
        n = (h * w * 3 + 15) // 16 * 16
        if not self.full and (not self.chunks or self.cursor + n > self.chunks[-1].numel()):
            room = self.budget - self.reserved
            if n > room:
                self.full = True
            else:
                self.chunks.append(self._chunk(max(n, min(self.CHUNK_BYTES, room))))
                self.reserved += self.chunks[-1].numel()
                self.cursor = 0
        if self.full:
            return None
        entry = _Entry(self.chunks[-1][self.cursor:self.cursor + h * w * 3].view(h, w, 3))
        self.cursor += n
        self.used += n
        self.entries[key] = entry
        return entry

    def close(self):
        if self.chunks and self.side is not None:
            torch.cuda.synchronize(self.device)      # a consumer may still read a NativeBatch view on its own stream
        self.chunks, self.entries, self.full = [], {}, True


def _read_file(path, size, dst, h, w):
    """worker of the device decoder: the file's bytes into the slot, its header parsed -> codecs.JpegInfo, or None for a file the device decoder
    declines (no JPEG, not baseline, ...: codecs.jpeg_info) or that changed since it was listed"""
    from . import codecs
    with open(path, "rb") as f:
        if f.readinto(dst) != size or f.read(1):
            return None
    try:
        info = codecs.jpeg_info(memoryview(dst))
    except codecs.JpegUnsupported:
        return None
    return info if (info.height, info.width) == (h, w) else None


_SIZES = {}


def _image_size(path):
    """(h, w) from the file header, remembered per path (the files of a dataset come round every epoch)"""
    key = str(path)
    if key not in _SIZES:
        from PIL import Image
        with Image.open(path) as im:          # header only
            _SIZES[key] = (im.size[1], im.size[0])
    return _SIZES[key]


class DeviceLoader:
    """Iterates Batch(img_exp, img_raw, img_name): fp32 [B,3,S,S] tensors on `device`, exactly the tensors the reference's
    DataLoader + InputFetcher deliver (data_loader.py:113-133), produced `prefetch` batches ahead of the consumer.

    train=True : RandomCrop(img_size) -> Resize(resize_size) -> flips      (get_train_loader, :72-90)
    train=False: Resize(img_size) of the whole image                        (get_test_loader, :93-110)
    train=False, img_size=0: the native mode -- nothing is resized and nothing transformed; it iterates NativeBatch, the decoded bytes of every
                 file as a uint8 [1,h,w,3] device tensor (tester.enhance_native / run_test take them from there)"""

    def __init__(self, dataset, batch_size, img_size=512, resize_size=256, train=True, shuffle=True, drop_last=True, num_workers=8,
                 device=None, prefetch=2, generator=None, shard=None, shard_seed=0, workers="thread", decode=None, cache=None, cache_bytes=None):
        """shard = (rank, world_size): this process iterates samples rank, rank + world, ... of the (shuffled) order -- one
        loader per GPU process.  The permutation of epoch e is then drawn from its own generator seeded
        shard_seed + e (the same on every rank, like DistributedSampler.set_epoch); crops and flips stay per-rank draws.
        workers: "thread" (decode in threads of this process: enough up to ~600 img/s, then the interpreter lock shared with the
        training loop caps it) or "process" (spawned decode processes writing into shared-memory segments that are page-locked
        for the H2D copy -- what DataLoader(num_workers=N) does, minus the transform and the pickling of tensors; as with any
        spawned pool, the launching script needs its `if __name__ == "__main__":` guard).
        decode: "host" (Pillow in the workers), "device" (baseline JPEG files are decoded on the device from their bytes, bit-exact with Pillow, so the
        tensors are the same; every other file takes the Pillow route and is counted in `fallbacks`, per pass, and `fallbacks_total`), or None: what
        set_input_decoder() chose.  "device" reads the files in threads.
        cache: "none" (every touch of a file decodes it again), "device", or None: what set_dataset_cache() chose.  "device" keeps the whole decoded
        image of every file in device memory from its first touch on (_ResidentStore; cache_bytes: the budget in bytes, default 16 GiB or what
        set_dataset_cache() set; no eviction: what does not fit is declined and decoded on every touch as with "none").  From the second touch on a
        batch is made with no file access, no host decode and no host-to-device pixel copy: uegan_input_transform_windows reads the crop windows in
        place.  The draws are consumed in the same order, so a seeded loader yields the tensors and names of cache="none", bit for bit.  The price:
        a file that changes on disk after it was cached is served from the store until close().  In the native mode the NativeBatch tensors of
        resident files are views into the store: read-only, alive as long as the loader.  Counters: cache_hits / cache_misses / cache_declined
        (touches, since the loader was made), cache_entries, cache_bytes_used."""
        self.cache = _dataset_cache if cache is None else cache
        if self.cache not in DATASET_CACHES:
            raise ValueError("unknown dataset cache %r (one of %s)" % (self.cache, ", ".join(DATASET_CACHES)))
        if cache_bytes is not None and (self.cache != "device" or isinstance(cache_bytes, bool) or int(cache_bytes) != cache_bytes or cache_bytes < 0):
            raise ValueError("cache_bytes=%r: expected a byte count, with cache='device'" % (cache_bytes,))
        self.cache_hits = self.cache_misses = self.cache_declined = 0
        self.decode = _input_decoder if decode is None else decode
        if self.decode not in INPUT_DECODERS:
            raise ValueError("unknown input decoder %r (one of %s)" % (self.decode, ", ".join(INPUT_DECODERS)))
        if self.decode == "device" and workers == "process":
            raise ValueError("decode='device' reads the files in threads: workers must be 'thread'")
        self.fallbacks = self.fallbacks_total = 0
        self.dataset, self.batch_size, self.img_size, self.resize_size = dataset, batch_size, img_size, resize_size
        self.train, self.shuffle, self.drop_last = train, shuffle, drop_last
        self.native = not train and img_size == 0
        self.generator = generator
        self.shard, self.shard_seed, self.epoch = shard, shard_seed, 0
        self.emulated = L.is_emulated()
        self.device = torch.device("cpu") if self.emulated else torch.device(device if device is not None else "cuda")
        self.prefetch = max(1, prefetch)
        if workers not in ("thread", "process"):
            raise ValueError("workers must be 'thread' or 'process'")
        self.shared = workers == "process"
        if self.shared:
            import multiprocessing
            self.pool = concurrent.futures.ProcessPoolExecutor(max_workers=max(1, num_workers), mp_context=multiprocessing.get_context("spawn"))
        else:
            self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, num_workers))
        self.side = None if self.emulated else torch.cuda.Stream(device=self.device)
        self.slots = [_Slot() for _ in range(self.prefetch + 1)]
        self.store = None
        if self.cache == "device":
            self.store = _ResidentStore(_dataset_cache_bytes if cache_bytes is None else cache_bytes, self.device, self.side)
        self._pass, self._file_sizes = 0, {}

    @property
    def cache_entries(self):
        return len(self.store.entries) if self.store is not None else 0

    @property
    def cache_bytes_used(self):
        return self.store.used if self.store is not None else 0

    def _n(self):
        n = len(self.dataset)
        if self.shard is not None:            # every rank's shard has the same length (DistributedSampler's padding): see _order
            world = self.shard[1]
            n = (n + world - 1) // world
        return n

    def set_epoch(self, epoch):
        """the permutation of epoch e is seeded with shard_seed + e on every rank (DistributedSampler.set_epoch).  Without a call the
        loader counts its own iterations -- which stays in step across ranks because every rank's shard has the same number of batches."""
        self.epoch = int(epoch)

    def close(self):
        """stop the decode workers and free the shared-memory segments"""
        self.pool.shutdown(wait=True, cancel_futures=True)
        for sl in self.slots:
            if sl.copied is not None:
                sl.copied.synchronize()
            sl.release()
        if self.store is not None:
            self.store.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = self._n()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self):
        n = len(self.dataset)
        if self.shard is None:
            return torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        rank, world = self.shard
        g = torch.Generator().manual_seed(self.shard_seed + self.epoch)
        self.epoch += 1
        order = torch.randperm(n, generator=g).tolist() if self.shuffle else list(range(n))
        # equal shards: pad by wrap-around to a multiple of `world` (like DistributedSampler with drop_last=False).  Unequal shards
        # would give the ranks different batch counts -- a `for batch in loader: train_step(...)` loop then deadlocks in the gradient
        # all-reduce, and with InputFetcher the short rank restarts early and its epoch counter (the permutation seed) drifts.
        total = (n + world - 1) // world * world
        order = (order * (total // max(n, 1) + 1))[:total] if n else order
        return order[rank::world]

    # -- stage 1: host decode into the pinned buffer (threads) -------------------------------------------------------
    def _submit(self, slot, indices):
        if self.store is not None:
            return self._submit_cached(slot, indices)
        if self.decode == "device":
            return self._submit_files(slot, indices)
        return self._submit_pixels(slot, indices)

    def _wait_slot(self, slot):
        """the wait for the slot's earlier use"""
        for f in getattr(slot, "futures", None) or []:      # decodes left pending by an abandoned iterator still write into this slot
            try:
                f.result()
            except Exception:
                pass
        slot.futures = []
        if slot.copied is not None:
            slot.copied.synchronize()            # the previous H2D copy out of this pinned buffer has finished
            slot.copied = None

    def _draw(self, slot, indices, align):
        """the wait for the slot's earlier use, the items and the plan of a batch: per file (path, top, left, h, w, flip bits, offset of its pixels)"""
        self._wait_slot(slot)
        items = [self.dataset[i] for i in indices]
        plan, off = [], 0
        for a, b, name in items:
            for path in (a, b):
                h, w = _image_size(path)
                if align:
                    off = (off + 15) // 16 * 16
                if self.train:
                    top, left, bits = draw_train_params(h, w, self.img_size, self.generator)
                    plan.append((path, top, left, self.img_size, self.img_size, bits, off))
                    off += self.img_size * self.img_size * 3
                else:
                    plan.append((path, 0, 0, h, w, 0, off))
                    off += h * w * 3
        return items, plan, off

    def _submit_files(self, slot, indices):
        """decode="device": the slot holds the pixel regions of _submit_pixels (16-byte aligned; a file of the Pillow route is decoded into its own)
        and, behind them, every file's bytes; a worker reads the file and parses its header"""
        items, plan, off = self._draw(slot, indices, True)
        pixel_bytes = off = (off + 15) // 16 * 16
        files = []
        for path, *_ in plan:
            size = os.path.getsize(path)
            files.append((off, size))
            off += (size + 15) // 16 * 16
        slot.ensure(off, self.device, pinned=not self.emulated, shared=False, mirror=not self.native)
        host = slot.host.numpy()
        for (path, _, _, _, _, _, _), (fo, size) in zip(plan, files):
            h, w = _image_size(path)
            slot.futures.append(self.pool.submit(_read_file, path, size, host[fo:fo + size], h, w))
        slot.items, slot.plan, slot.nbytes, slot.out = items, plan, off, None
        slot.files, slot.pixel_bytes = files, pixel_bytes

    def _submit_cached(self, slot, indices):
        """cache="device": the draws of _draw in its order, and per file what the store says -- "hit" (resident, or made resident by an earlier batch
        of this pass: uploads of a caching loader run in batch order), "miss" (a new entry: the WHOLE file is decoded, by the route of `decode`,
        straight into the entry or through the slot) or "declined" (no room: today's route; with decode="host" in train mode that is the window
        alone).  A hit takes nothing of the slot and starts no worker; the others get a 16-byte aligned pixel region and, with decode="device", a
        region for the file's bytes behind all of them.  slot.plan holds the image's own (h, w); slot.how (kind, entry, region h, region w)."""
        self._wait_slot(slot)
        items = [self.dataset[i] for i in indices]
        files_too = self.decode == "device"
        plan, how, off = [], [], 0
        for a, b, name in items:
            for path in (a, b):
                h, w = _image_size(path)
                top, left, bits = draw_train_params(h, w, self.img_size, self.generator) if self.train else (0, 0, 0)
                key = str(path)
                entry = self.store.entries.get(key)
                if entry is not None and (entry.filled or entry.pending == self._pass):
                    kind, rh, rw = "hit", 0, 0
                    self.cache_hits += 1
                else:      # (an entry left unfilled by an abandoned pass is filled again)
                    entry = entry if entry is not None else self.store.allocate(key, h, w)
                    if entry is None:
                        kind, (rh, rw) = "declined", (h, w) if files_too or not self.train else (self.img_size, self.img_size)
                        self.cache_declined += 1
                    else:
                        kind, rh, rw, entry.pending = "miss", h, w, self._pass
                        self.cache_misses += 1
                off = (off + 15) // 16 * 16
                plan.append((path, top, left, h, w, bits, off))
                how.append((kind, entry, rh, rw))
                off += rh * rw * 3
        pixel_bytes = off = (off + 15) // 16 * 16
        files = {}
        if files_too:
            for i, (path, *_) in enumerate(plan):
                if how[i][0] != "hit":
                    key = str(path)
                    if key not in self._file_sizes:
                        self._file_sizes[key] = os.path.getsize(path)
                    files[i] = (off, self._file_sizes[key])
                    off += (files[i][1] + 15) // 16 * 16
        slot.ensure(max(off, 16), self.device, pinned=not self.emulated, shared=self.shared, mirror=files_too or not self.native)
        host = slot.host.numpy()
        slot.reads = {}
        for i, ((path, top, left, h, w, _, o), (kind, _, rh, rw)) in enumerate(zip(plan, how)):
            if kind == "hit":
                continue
            whole = kind == "miss" or not self.train
            if files_too:
                fo, size = files[i]
                slot.reads[i] = self.pool.submit(_read_file, path, size, host[fo:fo + size], h, w)
                slot.futures.append(slot.reads[i])
            elif self.shared:
                slot.futures.append(self.pool.submit(_worker_decode, slot.shm.name, o, str(path), top, left, rh, rw, whole))
            else:
                dst = host[o:o + rh * rw * 3].reshape(rh, rw, 3)
                slot.futures.append(self.pool.submit(_decode_whole, path, dst) if whole else self.pool.submit(_decode_window, path, top, left, rh, rw, dst))
        slot.items, slot.plan, slot.how, slot.nbytes, slot.out = items, plan, how, off, None
        slot.files, slot.pixel_bytes = files, pixel_bytes

    def _upload_cached(self, slot, stream_handle):
        """cache="device", on the side stream: fill the entries of this batch's misses (decode="host": one copy out of the slot each; "device": the
        files' bytes go up in one copy, uegan_jpeg_decode writes into the entry, a file it declines is decoded by Pillow here and copied), bring up
        what was declined as today, then cut the batch out of the resident images -- one uegan_input_transform_windows call per 64 windows in train
        mode, per run of equally sized images in test mode; the native mode hands out the images themselves.  A batch of hits is that call alone."""
        from . import codecs
        files_too = self.decode == "device"
        if files_too and slot.nbytes > slot.pixel_bytes:
            slot.dev[slot.pixel_bytes:slot.nbytes].copy_(slot.host[slot.pixel_bytes:slot.nbytes], non_blocking=True)
        images, origins, transient = [], [], []
        for i, ((path, top, left, h, w, _, o), (kind, entry, rh, rw)) in enumerate(zip(slot.plan, slot.how)):
            if kind == "hit":
                images.append(entry.pixels)
                origins.append((top, left))
                continue
            n = rh * rw * 3
            if files_too:
                target = entry.pixels if kind == "miss" else torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
                info, decoded = slot.reads[i].result(), False
                if info is not None:
                    try:
                        fo, size = slot.files[i]
                        codecs.jpeg_decode_into(info, slot.dev[fo:fo + size], target, stream=stream_handle)
                        decoded = True
                    except codecs.JpegDecodeError:
                        pass
                if not decoded:
                    self.fallbacks += 1
                    self.fallbacks_total += 1
                    _decode_whole(path, slot.host.numpy()[o:o + n].reshape(h, w, 3))
                    target.view(-1).copy_(slot.host[o:o + n], non_blocking=True)
            elif kind == "miss" or self.native:      # (a declined native image is a buffer of its own: slot.dev would be overwritten by the next batch)
                target = entry.pixels if kind == "miss" else torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
                target.view(-1).copy_(slot.host[o:o + n], non_blocking=True)
            else:
                slot.dev[o:o + n].copy_(slot.host[o:o + n], non_blocking=True)
                target = slot.dev[o:o + n].view(rh, rw, 3)
                if self.train:
                    top = left = 0                   # (the worker decoded the window alone)
            if kind == "miss":
                entry.filled = True
            else:
                transient.append(target)
            images.append(target)
            origins.append((top, left))
        slot.transient = transient
        if self.native:
            return [im.view(1, im.shape[0], im.shape[1], 3) for im in images]
        S = self.resize_size if self.train else self.img_size
        out = torch.empty((len(images), 3, S, S), dtype=torch.float32, device=self.device)
        if self.train:
            input_transform_windows(images, origins, self.img_size, S, [p[5] for p in slot.plan], out=out, stream=stream_handle)
            return out
        i = 0
        while i < len(images):
            j = i + 1
            while j < len(images) and images[j].shape == images[i].shape:
                j += 1
            input_transform_windows(images[i:j], origins[i:j], tuple(images[i].shape[:2]), S, None, out=out[i:j], stream=stream_handle)
            i = j
        return out

    def _submit_pixels(self, slot, indices):
        self._wait_slot(slot)
        items = [self.dataset[i] for i in indices]
        plan, off = [], 0
        for a, b, name in items:
            for path in (a, b):
                h, w = _image_size(path)
                if self.train:
                    top, left, bits = draw_train_params(h, w, self.img_size, self.generator)
                    plan.append((path, top, left, self.img_size, self.img_size, bits, off))
                    off += self.img_size * self.img_size * 3
                else:
                    if self.native:
                        off = (off + 15) // 16 * 16      # every image starts 16-byte aligned: uegan_native_input reads whole dwords then
                    plan.append((path, 0, 0, h, w, 0, off))
                    off += h * w * 3
        slot.ensure(off, self.device, pinned=not self.emulated, shared=self.shared, mirror=not self.native)
        host = slot.host.numpy()
        slot.futures = []
        for path, top, left, h, w, bits, o in plan:
            if self.shared:
                slot.futures.append(self.pool.submit(_worker_decode, slot.shm.name, o, str(path), top, left, h, w, not self.train))
                continue
            dst = host[o:o + h * w * 3].reshape(h, w, 3)
            if self.train:
                slot.futures.append(self.pool.submit(_decode_window, path, top, left, h, w, dst))
            else:
                slot.futures.append(self.pool.submit(_decode_whole, path, dst))
        slot.items, slot.plan, slot.nbytes, slot.out = items, plan, off, None

    # -- stage 2: one H2D copy + the transform kernels, on the side stream -------------------------------------------
    def _upload_files(self, slot, stream_handle):
        """decode="device": the files' bytes go up in one copy and are decoded on this stream into the pixel regions the transforms read (train: the
        whole image into a buffer of its own, the crop window copied out of it).  A file without a header the device takes, or whose decode returns
        a status, is decoded by Pillow here and its pixels copied up alone.  -> the device buffer that holds the pixel regions"""
        from . import codecs
        infos = [f.result() for f in slot.futures]
        lo, hi = slot.pixel_bytes, slot.nbytes
        if self.native:      # (as in _upload: the batch is a buffer of its own)
            pix = torch.empty((slot.pixel_bytes,), dtype=torch.uint8, device=self.device)
            fdev, base = torch.empty((hi - lo,), dtype=torch.uint8, device=self.device), lo
        else:
            pix, fdev, base = slot.dev, slot.dev, 0
        fdev[lo - base:hi - base].copy_(slot.host[lo:hi], non_blocking=True)
        host = slot.host.numpy()
        for info, (path, top, left, h, w, _, o), (fo, size) in zip(infos, slot.plan, slot.files):
            region = pix[o:o + h * w * 3]
            if info is not None:
                try:
                    blob = fdev[fo - base:fo - base + size]
                    if self.train:
                        whole = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=self.device)
                        codecs.jpeg_decode_into(info, blob, whole, stream=stream_handle)
                        region.view(h, w, 3).copy_(whole[top:top + h, left:left + w])
                    else:
                        codecs.jpeg_decode_into(info, blob, region, stream=stream_handle)
                    continue
                except codecs.JpegDecodeError:
                    pass
            self.fallbacks += 1
            self.fallbacks_total += 1
            dst = host[o:o + h * w * 3].reshape(h, w, 3)
            if self.train:
                _decode_window(path, top, left, h, w, dst)
            else:
                _decode_whole(path, dst)
            region.copy_(slot.host[o:o + h * w * 3], non_blocking=True)
        return pix

    def _upload(self, slot):
        for f in slot.futures:
            f.result()                           # (re-raises decode errors here)
        B = len(slot.items)
        S = self.resize_size if self.train else self.img_size

        def run(stream_handle):
            if self.store is not None:
                return self._upload_cached(slot, stream_handle)
            if self.decode == "device":
                pix = self._upload_files(slot, stream_handle)
                if self.native:
                    return pix
                out = torch.empty((2 * B, 3, S, S), dtype=torch.float32, device=self.device)
                if self.train:
                    c = self.img_size
                    if all(p_[6] == i * c * c * 3 for i, p_ in enumerate(slot.plan)):      # (the 16-byte alignment left no gaps: one call, as "host")
                        input_transform(pix[:2 * B * c * c * 3].view(2 * B, c, c, 3), S, [p_[5] for p_ in slot.plan], out=out, stream=stream_handle)
                    else:
                        for i, p_ in enumerate(slot.plan):
                            input_transform(pix[p_[6]:p_[6] + c * c * 3].view(1, c, c, 3), S, [p_[5]], out=out[i:i + 1], stream=stream_handle)
                else:
                    for i, (path, _, _, h, w, _, o) in enumerate(slot.plan):
                        input_transform(pix[o:o + h * w * 3].view(1, h, w, 3), S, None, out=out[i:i + 1], stream=stream_handle)
                return out
            if self.native:      # the batch IS the copied bytes: a buffer of its own (slot.dev is overwritten by the slot's next batch)
                dev = torch.empty((slot.nbytes,), dtype=torch.uint8, device=self.device)
                dev.copy_(slot.host[:slot.nbytes], non_blocking=True)
                return dev
            slot.dev[:slot.nbytes].copy_(slot.host[:slot.nbytes], non_blocking=True)
            out = torch.empty((2 * B, 3, S, S), dtype=torch.float32, device=self.device)
            if self.train:
                c = self.img_size
                pix = slot.dev[:slot.nbytes].view(2 * B, c, c, 3)
                input_transform(pix, S, [p[5] for p in slot.plan], out=out, stream=stream_handle)
            else:
                for i, (path, _, _, h, w, _, o) in enumerate(slot.plan):
                    input_transform(slot.dev[o:o + h * w * 3].view(1, h, w, 3), S, None, out=out[i:i + 1], stream=stream_handle)
            return out

        if self.emulated:
            slot.out = run(None)
            return
        with torch.cuda.stream(self.side):
            slot.out = run(self.side.cuda_stream)
            slot.copied = torch.cuda.Event()
            slot.copied.record(self.side)
            slot.ready = slot.copied

    def __iter__(self):
        self.fallbacks = 0
        self._pass += 1
        order = self._order()
        bs = self.batch_size
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        if self.drop_last and batches and len(batches[-1]) < bs:
            batches.pop()
        queue = collections.deque()
        nxt = 0
        free = collections.deque(self.slots)
        while nxt < len(batches) or queue:
            while nxt < len(batches) and free and len(queue) < self.prefetch + 1:
                slot = free.popleft()
                self._submit(slot, batches[nxt])
                queue.append(slot)
                nxt += 1
            head = queue[0]
            if head.out is None:
                self._upload(head)
            for s in list(queue)[1:]:            # upload later batches whose decode has already finished
                if s.out is None and all(f.done() for f in s.futures):
                    self._upload(s)
                elif s.out is None and self.store is not None:
                    break                        # a caching loader uploads in batch order: a later batch may hit what this one makes resident
            queue.popleft()
            out, names = head.out, [it[2] for it in head.items]
            if not self.emulated:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(head.ready)
                for t in (head.transient if isinstance(out, list) else [out]):      # (views into the store are never freed before close())
                    t.record_stream(cur)
            B = len(head.items)
            if isinstance(out, list):            # cache="device", native: the resident images themselves, and buffers of their own for declined files
                paths = [(str(it[0]), str(it[1])) for it in head.items]
                head.out = None
                free.append(head)
                yield NativeBatch(out[0::2], out[1::2], names, paths)
                continue
            if self.native:
                imgs = [out[o:o + h * w * 3].view(1, h, w, 3) for _, _, _, h, w, _, o in head.plan]
                paths = [(str(it[0]), str(it[1])) for it in head.items]
                head.out = None
                free.append(head)
                yield NativeBatch(imgs[0::2], imgs[1::2], names, paths)
                continue
            pair = out.view(B, 2, *out.shape[1:])
            head.out = None
            free.append(head)
            yield Batch(pair[:, 0], pair[:, 1], names)


def get_train_loader(root, img_size=512, resize_size=256, batch_size=8, shuffle=True, num_workers=8, drop_last=True, device=None, generator=None,
                     shard=None, shard_seed=0, workers="thread", decode=None, cache=None, cache_bytes=None):
    """data_loader.py:72-90 with the transform on the device"""
    return DeviceLoader(ReferenceDataset(root), batch_size, img_size, resize_size, True, shuffle, drop_last, num_workers, device, generator=generator,
                        shard=shard, shard_seed=shard_seed, workers=workers, decode=decode, cache=cache, cache_bytes=cache_bytes)


def get_test_loader(root, img_size=512, batch_size=8, shuffle=False, num_workers=4, device=None, generator=None, workers="thread", decode=None, cache=None,
                    cache_bytes=None):
    """data_loader.py:93-110.  img_size=0: the native mode of DeviceLoader (NativeBatch: the decoded files as they are, for tester.run_test /
    tester.enhance_native to enhance at their own size)"""
    return DeviceLoader(ReferenceDataset(root), batch_size, img_size, img_size, False, shuffle, False, num_workers, device, generator=generator,
                        workers=workers, decode=decode, cache=cache, cache_bytes=cache_bytes)


class InputFetcher:
    """data_loader.py:113-133: endless iteration, restarting the loader when it runs out; the tensors are already on the device"""

    def __init__(self, loader):
        self.loader = loader
        self.iter = None

    def _fetch_refs(self):
        if self.iter is None:
            self.iter = iter(self.loader)
        try:
            return next(self.iter)
        except StopIteration:
            self.iter = iter(self.loader)
            return next(self.iter)

    def __next__(self):
        return self._fetch_refs()
