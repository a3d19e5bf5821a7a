"""uegan_montage_u8 (csrc/metrics.hip) through tester.montage_u8: 1..4 images side by side, quantised in one pass, bit-equal to the oracle's
`to_uint8_image(torch.cat(images, 3))` -- what save_image(torch.cat([denorm(a), denorm(b), ...], 3)) writes (trainer.py:182-183,244-245,
tester.py:73-74) -- on the scalar path, the vector path, the launcher's fall-back for a misaligned source and across both grid caps."""
import pytest
import torch

from helpers import BACKENDS, use_backend
from oracle import uegan_oracle as O
from uegan_amd import tester


def _images(seed, n, B, H, W):
    """tests/test_metrics.py::_images' generator: smooth + noise, partly outside [-1, 1], so both clamps act"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        base = torch.nn.functional.interpolate(torch.rand(B, 3, 5, 7, generator=g), size=(H, W), mode="bilinear", align_corners=True) * 2.4 - 1.2
        out.append(base + 0.05 * torch.randn(B, 3, H, W, generator=g))
    return out


def _check(images, dev, on_device=None):
    want = O.to_uint8_image(torch.cat(images, 3))
    assert int(want.min()) == 0 and int(want.max()) == 255          # both clamps are exercised
    got = tester.montage_u8(*(on_device if on_device is not None else [x.to(dev) for x in images]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_montage_scalar_path_odd_width(backend, n):
    dev = use_backend(backend)
    _check(_images(10 + n, n, 2, 5, 7), dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_vector_path(backend):
    dev = use_backend(backend)
    _check(_images(21, 3, 1, 16, 24), dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_misaligned_source_falls_back(backend):
    """the shape qualifies for the vector path, but the first source starts 1 float (4 bytes) into its buffer: 16-byte loads would be misaligned"""
    dev = use_backend(backend)
    a, b = _images(22, 2, 3, 8, 12)
    buf = torch.empty(a.numel() + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _check([a, b], dev, on_device=[view, b.to(dev)])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1028, 1024), (1, 513, 513)], ids=["vector", "scalar"])
def test_montage_past_the_grid_cap(shape):
    """the launcher caps its grid at MONTAGE_MAX_BLOCKS blocks of MONTAGE_THREADS threads (4 pixels per thread on the vector path, 1 on the
    scalar path): just above that count the kernels take their grid-stride loop a second time"""
    dev = use_backend("gpu")
    B, H, W = shape
    per_thread = tester.MONTAGE_VEC if W % tester.MONTAGE_VEC == 0 else 1
    cap = tester.MONTAGE_MAX_BLOCKS * tester.MONTAGE_THREADS * per_thread
    assert cap < B * H * W <= cap * 1.01
    _check(_images(23, 1, B, H, W), dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_montage_arguments_and_single_image(backend):
    dev = use_backend(backend)
    imgs = [x.to(dev) for x in _images(24, 5, 2, 8, 12)]
    with pytest.raises(ValueError):
        tester.montage_u8()
    with pytest.raises(ValueError):
        tester.montage_u8(*imgs)
    with pytest.raises(ValueError):
        tester.montage_u8(imgs[0], imgs[1][:, :, :, :8])
    with pytest.raises(ValueError):
        tester.montage_u8(imgs[0], imgs[1][:1])
    with pytest.raises(TypeError):
        tester.montage_u8(imgs[0], imgs[1].double())
    assert torch.equal(tester.montage_u8(imgs[0]), tester.to_uint8_image(imgs[0]))
