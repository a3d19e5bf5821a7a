"""The dataset cache (DeviceLoader(cache="device"), data.set_dataset_cache, UEGAN_DATASET_CACHE): every decoded file stays in device memory from its
first touch on and the batches are cut out of the resident images.  The oracle is equality with the loader that caches nothing: the same seed gives
the same names and bit-identical tensors, with thread and process workers, either decoder, sharded, and after the files are gone."""
import json
import os
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import jpeg_decode_helpers as JH
import uegan_amd
from helpers import BACKENDS, use_backend
from test_data import _make_tree
from uegan_amd import data, models, ops, runner

SIZES = [(40, 52), (36, 36), (61, 33)]


def _tree(monkeypatch, tmp_path):
    """7 pairs below the relative, dot-free root "data" (the sample name is the path up to its first '.') -> the arrays the files were written from"""
    monkeypatch.chdir(tmp_path)
    Path("data").mkdir()
    return _make_tree(Path("data"), 7, SIZES)


def _train(dev, cache, seed=11, **kw):
    kw = dict(dict(img_size=32, resize_size=16, batch_size=3, shuffle=True, num_workers=3), **kw)
    return data.get_train_loader("data", device=dev, generator=torch.Generator().manual_seed(seed), cache=cache, **kw)


def _passes(loader, n):
    return [[(b.img_name, b.img_exp.cpu().clone(), b.img_raw.cpu().clone()) for b in loader] for _ in range(n)]


def _same(got, want):
    assert len(got) == len(want) and all(len(g) == len(w) and len(g) > 0 for g, w in zip(got, want))
    for g, w in zip(got, want):
        for (gn, ge, gr), (wn, we, wr) in zip(g, w):
            assert gn == wn and torch.equal(ge, we) and torch.equal(gr, wr), (gn, wn)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("workers", ["thread", "process"])
def test_train_batches_equal_the_uncached_loaders(backend, workers, tmp_path, monkeypatch):
    dev = use_backend(backend)
    _tree(monkeypatch, tmp_path)
    got = {}
    for cache in ("none", "device"):
        loader = _train(dev, cache, workers=workers, num_workers=2)
        try:
            assert loader.cache == cache and len(loader) == 2
            got[cache] = _passes(loader, 3)
            if cache == "none":
                assert (loader.cache_hits, loader.cache_misses, loader.cache_declined, loader.cache_entries, loader.cache_bytes_used) == (0, 0, 0, 0, 0)
            else:
                assert loader.cache_hits + loader.cache_misses == 3 * 12 and loader.cache_declined == 0 and loader.cache_misses == loader.cache_entries
        finally:
            loader.close()
    _same(got["device"], got["none"])
    assert got["none"][0][0][1].shape == (3, 3, 16, 16)


@pytest.mark.parametrize("backend", BACKENDS)
def test_counters(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    _tree(monkeypatch, tmp_path)
    loader = _train(dev, "device", drop_last=False)
    try:
        for n in range(1, 4):
            assert sum(len(b.img_name) for b in loader) == 7
            assert (loader.cache_misses, loader.cache_hits, loader.cache_declined) == (14, 14 * (n - 1), 0)
        assert loader.cache_entries == 14
        assert loader.cache_bytes_used == 2 * sum((h * w * 3 + 15) // 16 * 16 for h, w in (SIZES * 3)[:7])
    finally:
        loader.close()
    # drop_last: a pass touches the first 6 pairs of its permutation.  The permutations are replayed from the seed: the loader's generator also
    # serves the crops and flips of the 12 images of a pass, in the order data.draw_train_params documents
    ds = data.ReferenceDataset("data")
    g = torch.Generator().manual_seed(11)
    seen, misses, hits = set(), 0, 0
    loader = _train(dev, "device")
    try:
        for _ in range(4):
            perm = torch.randperm(7, generator=g).tolist()[:6]
            for idx in perm:
                for path in ds[idx][:2]:
                    data.draw_train_params(*data._image_size(path), 32, g)
            misses += 2 * len(set(perm) - seen)
            hits += 2 * len(set(perm) & seen)
            seen |= set(perm)
            assert [n for b in loader for n in b.img_name] == [ds[i][2] for i in perm]
            assert (loader.cache_misses, loader.cache_hits) == (misses, hits)
        assert len(seen) == 7 and loader.cache_entries == 14 and hits > 0
    finally:
        loader.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_no_file_access_after_the_first_pass(backend, tmp_path, monkeypatch):
    """after one full pass the tree is deleted: the train, test and native loaders go on yielding what an uncached loader yielded while it existed"""
    dev = use_backend(backend)
    arrs = _tree(monkeypatch, tmp_path)
    plain = _train(dev, "none", drop_last=False)
    want_train = _passes(plain, 2)
    plain.close()
    plain = data.get_test_loader("data", img_size=24, batch_size=4, num_workers=2, device=dev, cache="none")
    want_test = _passes(plain, 1)
    plain.close()
    train = _train(dev, "device", drop_last=False)
    test = data.get_test_loader("data", img_size=24, batch_size=4, num_workers=2, device=dev, cache="device")
    native = data.get_test_loader("data", img_size=0, batch_size=3, num_workers=2, device=dev, cache="device")
    try:
        first = _passes(train, 1)
        _same(_passes(test, 1), want_test)
        assert sum(len(b.img_name) for b in native) == 7
        shutil.rmtree("data")
        assert not os.path.exists("data")
        _same(first + _passes(train, 1), want_train)
        _same(_passes(test, 1), want_test)
        assert (test.cache_misses, test.cache_hits, native.cache_misses) == (14, 14, 14)
        seen = 0
        for batch in native:
            assert isinstance(batch, data.NativeBatch) and len(batch.img_exp) == len(batch.img_raw) == len(batch.paths)
            for (pe, pr), e, r in zip(batch.paths, batch.img_exp, batch.img_raw):
                for path, t in ((pe, e), (pr, r)):
                    a = arrs[(Path(path).parent.name, int(Path(path).stem[2:]))]
                    assert t.dtype == torch.uint8 and t.shape == (1,) + a.shape and t.data_ptr() % 16 == 0
                    assert np.array_equal(t[0].cpu().numpy(), a), path
                    seen += 1
        assert seen == 14 and native.cache_hits == 14
    finally:
        for ld in (train, test, native):
            ld.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_budget_declines_what_does_not_fit(backend, tmp_path, monkeypatch):
    """a budget that holds exactly the first 5 images touched (each rounded up to 16 bytes): they stay resident, every other file is decoded on
    every touch, and the tensors are still those of the uncached loader"""
    dev = use_backend(backend)
    _tree(monkeypatch, tmp_path)
    ds = data.ReferenceDataset("data")
    touched = [path for i in range(7) for path in ds[i][:2]]                  # shuffle=False: listing order, label file before raw file
    sizes = [data._image_size(p) for p in touched]
    budget = sum((h * w * 3 + 15) // 16 * 16 for h, w in sizes[:5])
    for make in (lambda cache, **kw: _train(dev, cache, shuffle=False, drop_last=False, **kw),
                 lambda cache, **kw: data.get_test_loader("data", img_size=24, batch_size=3, num_workers=2, device=dev, cache=cache, **kw)):
        plain = make("none")
        want = _passes(plain, 2)
        plain.close()
        loader = make("device", cache_bytes=budget)
        try:
            _same(_passes(loader, 2), want)
            assert loader.cache_entries == 5 and loader.cache_bytes_used == budget
            assert sorted(loader.store.entries) == sorted(str(p) for p in touched[:5])
            assert (loader.cache_misses, loader.cache_hits, loader.cache_declined) == (5, 5, 2 * 9)
        finally:
            loader.close()
        smaller = make("device", cache_bytes=budget - 1)                      # one byte less: the fifth image is declined, and so is every later one
        try:
            _same(_passes(smaller, 2), want)
            assert smaller.cache_entries == 4 and smaller.cache_bytes_used <= budget - 1 and smaller.cache_declined == 2 * 10
        finally:
            smaller.close()


def _jpeg_tree():
    """four pairs of baseline JPEG files (4:4:4, 4:2:0 with restart markers, 4:2:2 optimised, grayscale), one raw file a PNG"""
    from PIL import Image
    spec = [((40, 52), "4:4:4", {}), ((33, 47), "4:2:0", {"restart_marker_rows": 1}), ((64, 64), "4:2:2", {"optimize": True}), ((36, 36), "gray", {})]
    for d in ("label", "raw"):
        Path("src", d).mkdir(parents=True)
        for i, ((h, w), ss, kw) in enumerate(spec):
            a = JH.photo_like(40 + i + 10 * (d == "raw"), h, w)
            if (d, i) == ("raw", 0):
                Image.fromarray(a, "RGB").save(Path("src", d, "im00.png"))
            elif ss == "gray":
                Path("src", d, "im%02d.jpg" % i).write_bytes(JH.pillow_jpeg(a[..., 1].copy(), 90))
            else:
                Path("src", d, "im%02d.jpg" % i).write_bytes(JH.pillow_jpeg(a, 90, ss, **kw))


@pytest.mark.parametrize("backend", BACKENDS)
def test_device_decoder_fills_the_store(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    monkeypatch.chdir(tmp_path)
    _jpeg_tree()
    made = {"train": lambda **kw: data.get_train_loader("src", 32, 16, batch_size=3, shuffle=True, num_workers=2, drop_last=False, device=dev,
                                                        generator=torch.Generator().manual_seed(5), **kw),
            "test": lambda **kw: data.get_test_loader("src", 24, batch_size=3, num_workers=2, device=dev, **kw)}
    for mode, make in made.items():
        plain = make(decode="host", cache="none")
        want = _passes(plain, 2)
        plain.close()
        loader = make(decode="device", cache="device")
        try:
            _same(_passes(loader, 1), want[:1])
            assert loader.fallbacks == 1 and (loader.cache_misses, loader.cache_hits) == (8, 0), mode
            _same(_passes(loader, 1), want[1:])
            assert loader.fallbacks == 0 and loader.fallbacks_total == 1 and (loader.cache_misses, loader.cache_hits) == (8, 8), mode
        finally:
            loader.close()
    # native: the store's own images, equal to the host decoder's; and a budget of nothing: every file is declined and still decoded on the device
    plain = data.get_test_loader("src", 0, batch_size=3, num_workers=2, device=dev, decode="host", cache="none")
    want = [(b.img_name, [t.cpu().clone() for t in list(b.img_exp) + list(b.img_raw)]) for b in plain]
    plain.close()
    for budget, declined in ((None, 0), (0, 16)):
        loader = data.get_test_loader("src", 0, batch_size=3, num_workers=2, device=dev, decode="device", cache="device", cache_bytes=budget)
        try:
            for n in range(2):
                got = [(b.img_name, [t.cpu().clone() for t in list(b.img_exp) + list(b.img_raw)]) for b in loader]
                assert len(got) == len(want) == 2
                for (gn, gt), (wn, wt) in zip(got, want):
                    assert gn == wn and len(gt) == len(wt) and all(torch.equal(a, b) for a, b in zip(gt, wt))
                assert loader.fallbacks == (1 if n == 0 or declined else 0)
            assert loader.cache_declined == declined and loader.cache_entries == (0 if declined else 8)
        finally:
            loader.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_sharded_loaders(backend, tmp_path, monkeypatch):
    """two ranks, two epochs: 7 pairs are padded by wrap-around to 8, so one file comes round twice in an epoch"""
    dev = use_backend(backend)
    _tree(monkeypatch, tmp_path)
    for rank in range(2):
        got = {}
        for cache in ("none", "device"):
            loader = _train(dev, cache, seed=100 + rank, batch_size=1, num_workers=1, drop_last=False, shard=(rank, 2), shard_seed=3)
            try:
                got[cache] = _passes(loader, 2)
                assert len(got[cache][0]) == len(loader) == 4
                if cache == "device":
                    assert loader.cache_hits + loader.cache_misses == 16 and loader.cache_misses == loader.cache_entries
            finally:
                loader.close()
        _same(got["device"], got["none"])


def test_an_abandoned_pass_leaves_no_unfilled_entry(tmp_path, monkeypatch):
    """an iterator dropped after its first batch has planned misses it never uploaded: the next pass decodes those files again"""
    dev = use_backend("emu")
    _tree(monkeypatch, tmp_path)
    plain = _train(dev, "none", shuffle=False, batch_size=2, drop_last=False)
    want = _passes(plain, 1)
    plain.close()
    loader = _train(dev, "device", shuffle=False, batch_size=2, drop_last=False)
    try:
        it = iter(loader)
        next(it)
        del it
        # the generator has moved on, so the crops differ from `want`'s: compare the names, and every tensor with a fresh uncached pass
        # drawn from a generator in the same state
        state = loader.generator.get_state()
        got = _passes(loader, 1)
        twin = _train(dev, "none", shuffle=False, batch_size=2, drop_last=False)
        twin.generator.set_state(state)
        _same(got, _passes(twin, 1))
        twin.close()
        assert [n for b in got[0] for n in b[0]] == [n for b in want[0] for n in b[0]]
        assert loader.cache_entries == 14
    finally:
        loader.close()


def test_selection(monkeypatch):
    use_backend("emu")
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert data.get_dataset_cache() == "none" and uegan_amd.set_dataset_cache is data.set_dataset_cache
    assert uegan_amd.get_dataset_cache is data.get_dataset_cache and data.DATASET_CACHE_DEFAULT_BYTES == 16 << 30
    with pytest.raises(ValueError, match="unknown dataset cache 'host'"):
        data.set_dataset_cache("host")
    with pytest.raises(ValueError, match="unknown dataset cache 'gpu'"):
        data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False, cache="gpu")
    with pytest.raises(ValueError, match="needs the dataset cache 'device'"):
        data.set_dataset_cache("none", 2)
    for bad in (0, -1, float("nan"), float("inf"), "many", True):
        with pytest.raises(ValueError, match="positive number of gigabytes"):
            data.set_dataset_cache("device", bad)
    with pytest.raises(ValueError, match="cache_bytes"):
        data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False, cache="none", cache_bytes=1 << 20)
    assert data.get_dataset_cache() == "none"
    try:
        assert data.set_dataset_cache("device", 0.5) == "none" and data.get_dataset_cache() == "device"
        loader = data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False)
        assert loader.cache == "device" and loader.store.budget == 1 << 29
        loader.close()
        loader = data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False, cache="none")
        assert loader.cache == "none" and loader.store is None
        loader.close()
        assert data.set_dataset_cache("device") == "device"
        loader = data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False, cache_bytes=4096)
        assert loader.store.budget == 4096
        loader.close()
        loader = data.DeviceLoader(data.ReferenceDataset(golden), 1, train=False)
        assert loader.store.budget == 16 << 30 and not loader.store.chunks          # (nothing is allocated before the first image)
        loader.close()
    finally:
        data.set_dataset_cache("none")

    # the command line: both variables are parsed, every refusal names its variable and comes before any loader exists
    made = []
    monkeypatch.setattr(data, "DeviceLoader", lambda *a, **k: made.append(a) or pytest.fail("a loader was made"))
    argv = ["--mode", "test", "--is_test_nima", "False"]
    for name, gb, match in (("gpu", None, "UEGAN_DATASET_CACHE='gpu'"), ("Device", None, "UEGAN_DATASET_CACHE='Device'"), ("", None, "UEGAN_DATASET_CACHE=''"),
                            (None, "4", "UEGAN_DATASET_CACHE_GB='4' needs UEGAN_DATASET_CACHE=device"),
                            ("none", "4", "UEGAN_DATASET_CACHE_GB='4' needs UEGAN_DATASET_CACHE=device"),
                            ("device", "0", "UEGAN_DATASET_CACHE_GB='0'"), ("device", "-2", "UEGAN_DATASET_CACHE_GB='-2'"),
                            ("device", "lots", "UEGAN_DATASET_CACHE_GB='lots'"), ("device", "nan", "UEGAN_DATASET_CACHE_GB='nan'"),
                            ("device", "inf", "UEGAN_DATASET_CACHE_GB='inf'"), ("device", "", "UEGAN_DATASET_CACHE_GB=''")):
        for var, val in (("UEGAN_DATASET_CACHE", name), ("UEGAN_DATASET_CACHE_GB", gb)):
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)
        with pytest.raises(ValueError, match=match):
            runner.main(argv)
        assert data.get_dataset_cache() == "none" and not made
    try:
        monkeypatch.setenv("UEGAN_DATASET_CACHE", "device")
        monkeypatch.setenv("UEGAN_DATASET_CACHE_GB", "1.5")
        runner._apply_dataset_cache()
        assert data.get_dataset_cache() == "device" and data._dataset_cache_bytes == 3 << 29
        monkeypatch.delenv("UEGAN_DATASET_CACHE_GB")
        runner._apply_dataset_cache()
        assert data._dataset_cache_bytes == 16 << 30
        monkeypatch.setenv("UEGAN_DATASET_CACHE", "none")
        runner._apply_dataset_cache()
        assert data.get_dataset_cache() == "none"
    finally:
        data.set_dataset_cache("none")


def _checkpoint(save_root):
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    mdir = Path(save_root) / "UEGAN-FiveK" / "models"
    mdir.mkdir(parents=True)
    torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("size", ["32", "0"])
def test_command_line_test_mode(backend, size, tmp_path, monkeypatch):
    """python -m uegan_amd --mode test: the same result files and the same test_metrics.json with UEGAN_DATASET_CACHE=device as without it"""
    use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    root = "data" if size == "32" else "small"     # (data._image_size remembers sizes per path, and these paths are relative)
    Path(root).mkdir()
    n = 2                                          # (the generator's forward is what takes the time on the emulator: few and small images)
    _make_tree(Path(root), n, SIZES if size == "32" else [(32, 40), (36, 32)])
    argv = ["--mode", "test", "--test_img_dir", root, "--test_img_size", size, "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "3", "--is_test_nima", "False"]
    for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_PNG_ENCODER", "UEGAN_INPUT_DECODER", "UEGAN_DATASET_CACHE", "UEGAN_DATASET_CACHE_GB"):
        monkeypatch.delenv(k, raising=False)
    out = []
    try:
        for save_root, cache in (("results", None), ("results_cached", "device")):
            _checkpoint(save_root)
            if cache:
                monkeypatch.setenv("UEGAN_DATASET_CACHE", cache)
                monkeypatch.setenv("UEGAN_DATASET_CACHE_GB", "0.25")
            runner.main(argv + ["--save_root_dir", save_root])
            assert data.get_dataset_cache() == (cache or "none")
            base = Path(save_root) / "UEGAN-FiveK" / "test"
            m = json.loads((base / "test_metrics.json").read_text())
            m.pop("checkpoint")
            out.append((m, {str(p.relative_to(base)): p.read_bytes() for p in sorted(base.rglob("*.png"))}))
    finally:
        data.set_dataset_cache("none")
    assert out[0] == out[1] and len(out[0][0]["names"]) == n and len(out[0][1]) == 2 * n


@pytest.mark.gpu
def test_command_line_train_mode_validates_from_the_store(tmp_path, monkeypatch):
    """two epochs with a validation after each: the first validation fills the store, the second misses nothing.  On the GPU only, like the other
    --mode train tests (tests/test_runner.py): four training steps take minutes on the emulator."""
    use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    for sub, n, sizes in (("train", 2, [(100, 110)]), ("val", 3, [(40, 52), (36, 36)])):
        Path("data", sub).mkdir(parents=True)
        _make_tree(Path("data", sub), n, sizes)
    argv = ["--mode", "train", "--train_img_dir", "data/train", "--val_img_dir", "data/val", "--image_size", "96", "--resize_size", "96",
            "--train_batch_size", "1", "--g_conv_dim", "8", "--d_conv_dim", "8", "--vgg_weights", "seeded", "--pool_size", "3", "--test_img_size", "32",
            "--val_batch_size", "2", "--model_save_epoch", "9", "--compute_dtype", "float32", "--num_workers", "2", "--total_epochs", "2",
            "--num_epochs_start_val", "0", "--val_each_epochs", "1", "--info_step", "100", "--sample_step", "100", "--is_test_psnr_ssim", "True",
            "--is_test_nima", "False"]
    for k in ("UEGAN_IMAGE_FORMAT", "UEGAN_JPEG_QUALITY", "UEGAN_PNG_ENCODER", "UEGAN_INPUT_DECODER", "UEGAN_DATASET_CACHE_GB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("UEGAN_DATASET_CACHE", "device")
    try:
        runner.main(argv)
    finally:
        data.set_dataset_cache("none")
    with open(Path("results") / "UEGAN-FiveK" / "validation" / "validation.jsonl") as f:
        lines = [json.loads(s) for s in f]
    assert [r.get("epoch") for r in lines] == [1.0, 2.0, None] and all(r["images"] == 3 for r in lines[:2])
    assert lines[0]["dataset_cache"] == {"hits": 0, "misses": 6, "declined": 0}
    assert lines[1]["dataset_cache"] == {"hits": 6, "misses": 0, "declined": 0}
    assert all(np.isfinite(r["psnr"]) and np.isfinite(r["ssim"]) for r in lines[:2])
