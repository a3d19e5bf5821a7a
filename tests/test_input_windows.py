"""uegan_input_transform_windows / data.input_transform_windows: the input transform over crop windows read in place out of images resident on the
device.  The oracle is Pillow itself (oracle.uegan_oracle.train_transform / test_transform), and the result must also be torch.equal to
data.input_transform of the contiguous copies of the same windows."""
import numpy as np
import pytest
import torch

from helpers import BACKENDS, use_backend
from oracle import uegan_oracle as O
from uegan_amd import _lib, data


def _resident(dev):
    """four images carved out of ONE buffer of seeded noise, so that a wrong pitch or origin reads wrong bytes: a 40 x 52 whose base address is odd,
    a 36 x 36, a 61 x 70 ("big") and the 61 x 33 pitched view big[:, 3:36] -> {name: (device tensor, the same pixels as a numpy array)}"""
    buf = torch.from_numpy(np.random.default_rng(2024).integers(0, 256, size=1 + 40 * 52 * 3 + 36 * 36 * 3 + 61 * 70 * 3 + 7, dtype=np.uint8))
    on = buf.to(dev)
    out, off = {}, 1
    for name, (h, w) in (("a", (40, 52)), ("b", (36, 36)), ("big", (61, 70))):
        out[name] = (on[off:off + h * w * 3].view(h, w, 3), buf[off:off + h * w * 3].view(h, w, 3).numpy())
        off += h * w * 3
    out["view"] = (out["big"][0][:, 3:36], np.ascontiguousarray(out["big"][1][:, 3:36]))
    assert out["a"][0].data_ptr() % 4 != 0 and not out["view"][0].is_contiguous() and out["view"][0].shape == (61, 33, 3)
    return out


def _crops(images, windows, wh, ww):
    return torch.stack([im[t:t + wh, l:l + ww] for im, (t, l) in zip(images, windows)]).contiguous()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("win,resize", [(32, 16), (37, 20), (20, 20), (20, 33), (48, 13)])
def test_windows_of_mixed_images_match_pillow(backend, win, resize):
    """every image the window fits in, in ONE call: windows at (0, 0) and at (H - win, W - win) -- the latter ends on the image's last byte -- and
    the four flip codes in turn"""
    dev = use_backend(backend)
    res = _resident(dev)
    names = [n for n in ("a", "b", "view", "big") if res[n][1].shape[0] >= win and res[n][1].shape[1] >= win]
    assert names and (win > 36 or len(names) == 4)
    images, arrays, windows = [], [], []
    for n in names:
        h, w = res[n][1].shape[:2]
        for origin in ((0, 0), (h - win, w - win)):
            images.append(res[n][0])
            arrays.append(res[n][1])
            windows.append(origin)
    if len(images) < 4:                  # (48 x 48 fits the big image only: two more windows of it, so that every flip code occurs)
        images, arrays, windows = images * 2, arrays * 2, windows + [(5, 9), (13, 0)]
    flips = [i % 4 for i in range(len(images))]
    out = data.input_transform_windows(images, windows, win, resize, flips)
    assert out.shape == (len(images), 3, resize, resize) and out.dtype == torch.float32
    for i, (a, (t, l)) in enumerate(zip(arrays, windows)):
        assert torch.equal(out[i].cpu(), O.train_transform(a, t, l, win, resize, flips[i])), (i, names, windows[i])
    assert torch.equal(out, data.input_transform(_crops(images, windows, win, win), resize, flips))
    # without flips, into a caller's tensor
    mine = torch.full_like(out, 7.0)
    assert data.input_transform_windows(images, windows, win, resize, out=mine) is mine
    assert torch.equal(mine, data.input_transform(_crops(images, windows, win, win), resize))


@pytest.mark.parametrize("backend", BACKENDS)
def test_whole_image_windows(backend):
    """the window is the whole image (the test loader's case): non-square, through the pitched view, next to a contiguous image of the same size"""
    dev = use_backend(backend)
    res = _resident(dev)
    same = res["big"][0][:, 37:70].contiguous()
    out = data.input_transform_windows([res["view"][0], same], [(0, 0), (0, 0)], (61, 33), 24)
    assert torch.equal(out[0].cpu(), O.test_transform(res["view"][1], 24))
    assert torch.equal(out[1].cpu(), O.test_transform(np.ascontiguousarray(res["big"][1][:, 37:70]), 24))
    assert torch.equal(out, data.input_transform(torch.stack([res["view"][0], same]).contiguous(), 24))
    # a rectangular window and a rectangular output
    out = data.input_transform_windows([res["a"][0], res["big"][0]], [(3, 30), (40, 0)], (21, 22), (10, 17), [2, 1])
    assert torch.equal(out, data.input_transform(_crops([res["a"][0], res["big"][0]], [(3, 30), (40, 0)], 21, 22), (10, 17), [2, 1]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_more_windows_than_one_call_takes(backend):
    """70 windows in one Python call: two launches (INPUT_MAX_IMAGES is 64)"""
    dev = use_backend(backend)
    res = _resident(dev)
    assert data.MAX_IMAGES_PER_CALL == 64
    g = np.random.default_rng(7)
    names = [("a", "b", "view", "big")[i % 4] for i in range(70)]
    images = [res[n][0] for n in names]
    windows = [(int(g.integers(0, res[n][1].shape[0] - 7)), int(g.integers(0, res[n][1].shape[1] - 7))) for n in names]
    flips = [int(f) for f in g.integers(0, 4, size=70)]
    before = _lib.n_calls
    out = data.input_transform_windows(images, windows, 8, 4, flips)
    assert _lib.n_calls - before == 2
    for i in (0, 63, 64, 69):
        assert torch.equal(out[i].cpu(), O.train_transform(res[names[i]][1], windows[i][0], windows[i][1], 8, 4, flips[i])), i
    assert torch.equal(out, data.input_transform(_crops(images, windows, 8, 8), 4, flips))


@pytest.mark.parametrize("backend", BACKENDS)
def test_above_the_grid_cap(backend):
    """the horizontal pass caps its grid at WINDOWS_BLOCKS_PER_IMAGE = 512 blocks of 256 threads per image (csrc/input.hip) and loops by grid
    stride above that: a window of 400 x 400 -> 340 x 340 is 400 * 340 = 136000 items > 131072.  This is the case above the cap; every other
    case of this file is below it."""
    dev = use_backend(backend)
    assert 400 * 340 > 512 * 256
    a = np.random.default_rng(11).integers(0, 256, size=(420, 410, 3), dtype=np.uint8)
    im = torch.from_numpy(a).to(dev)
    windows = [(0, 0), (20, 10), (7, 3)]
    flips = [3, 0, 1]
    out = data.input_transform_windows([im] * 3, windows, 400, 340, flips)
    assert torch.equal(out, data.input_transform(_crops([im] * 3, windows, 400, 400), 340, flips))
    for i in (0, 1):
        assert torch.equal(out[i].cpu(), O.train_transform(a, windows[i][0], windows[i][1], 400, 340, flips[i]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_window_outside_its_image_is_refused(backend):
    """a window that leaves its image returns a status before anything is launched: `out`, prefilled with a sentinel, is untouched -- also when
    the windows before it in the same call are fine"""
    dev = use_backend(backend)
    res = _resident(dev)
    a, view = res["a"][0], res["view"][0]                 # 40 x 52, and 61 x 33 with a pitch of 70 pixels
    bad = [([a], [(9, 0)]), ([a], [(0, 21)]), ([a], [(-1, 0)]), ([a], [(0, -1)]), ([view], [(0, 2)]), ([view], [(30, 0)]),
           ([a, view, a], [(8, 20), (29, 1), (8, 21)]), ([a], [(2 ** 31 - 20, 0)])]
    for images, windows in bad:
        out = torch.full((len(images), 3, 16, 16), -9.0, dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match="leaves its"):
            data.input_transform_windows(images, windows, 32, 16, out=out)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert bool((out == -9.0).all()), windows
    out = data.input_transform_windows([a, view], [(8, 20), (29, 1)], 32, 16)          # the largest origins that fit
    assert torch.equal(out, data.input_transform(_crops([a, view], [(8, 20), (29, 1)], 32, 32), 16))
    # what the Python wrapper refuses itself
    with pytest.raises(ValueError):
        data.input_transform_windows([a], [(0, 0), (1, 1)], 32, 16)
    with pytest.raises(ValueError):
        data.input_transform_windows([a.permute(1, 0, 2)], [(0, 0)], 32, 16)          # pixels not contiguous
    with pytest.raises(ValueError):
        data.input_transform_windows([a[:, :, :2]], [(0, 0)], 32, 16)
    with pytest.raises(ValueError):
        data.input_transform_windows([], [], 32, 16)


def test_the_launcher_checks_its_descriptors():
    """the C entry point alone, on the emulator: counts, null pointers and a pitch below the width are refused with UEGAN_E_INVALID (-1)"""
    import ctypes
    dev = use_backend("emu")
    lib = _lib.load()
    im = torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev)
    tab, k = data._device_table(8, 4, dev)
    tmp = torch.zeros((1, 8, 4, 3), dtype=torch.uint8)
    out = torch.full((1, 3, 4, 4), -9.0)

    def call(desc, n, wh=8, ww=8):
        return lib.uegan_input_transform_windows(desc, n, wh, ww, 4, 4, tab.data_ptr(), k, tab.data_ptr(), k, tmp.data_ptr(), out.data_ptr(), None)
    good = (_lib.Window * 1)(_lib.Window(im.data_ptr(), 8, 0, 0, 0, 8, 8))
    assert call(good, 1) == 0 and not bool((out == -9.0).any())
    out.fill_(-9.0)
    assert call(good, 0) == -1 and call(good, 65) == -1 and call(None, 1) == -1 and call(good, 1, 0, 8) == -1
    for fields in ((None, 8, 0, 0, 0, 8, 8), (im.data_ptr(), 7, 0, 0, 0, 8, 8), (im.data_ptr(), 8, 0, 0, 0, 0, 8), (im.data_ptr(), 8, 1, 0, 0, 8, 8)):
        assert call((_lib.Window * 1)(_lib.Window(*fields)), 1) == -1, fields
        assert b"input_transform_windows" in lib.uegan_last_error()
    assert bool((out == -9.0).all())
    assert ctypes.sizeof(_lib.Window) == 32 and lib.uegan_version() == 105
