"""uegan_amd/runner.py: init_weights, `--mode test` and `--mode train` end to end (main.py, trainer.py:39-146,171-309, tester.py:41-103) on small
PNG trees, against the pieces the runner is built from (tester.run_test, trainer.Trainer, data loaders) driven directly."""
import json
import os
import random
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import BACKENDS, use_backend
from oracle import uegan_oracle as O
from test_data import _make_tree
from test_train_step import NAMES, _check_losses
from uegan_amd import data, losses, models, nima, ops, runner, tester, trainer

CKPT_KEYS = {"G_net", "D_net", "epoch", "g_optimizer", "d_optimizer", "lr_scheduler_g", "lr_scheduler_d"}      # trainer.py:199-207


def _conv_weights(net):
    return {k: v for k, v in net.state_dict().items() if v.dim() == 4}


# ---- init_weights (CPU) ----
def test_init_weights_orthogonal_gain():
    torch.manual_seed(5)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    before = ops._weight_epoch[0]
    runner.init_weights(G, "orthogonal", 0.02)
    runner.init_weights(D, "orthogonal", 0.02)
    assert ops._weight_epoch[0] >= before + 2                  # the packed copies are dropped
    assert sum(k.endswith("weight_orig") for k in _conv_weights(D)) >= 5      # the spectral-norm convolutions: `.weight` is weight_orig there
    for net in (G, D):
        ws = _conv_weights(net)
        assert ws
        for k, w in ws.items():
            sv = torch.linalg.svdvals(w.double().reshape(w.shape[0], -1))
            assert float((sv - 0.02).abs().max()) <= 1e-5 * 0.02, (k, float(sv.min()), float(sv.max()))
        biases = [v for k, v in net.state_dict().items() if k.endswith("bias")]
        assert biases and all(float(b.abs().max()) == 0.0 for b in biases)


def test_init_weights_normal_and_unknown():
    torch.manual_seed(6)
    G = models.Generator(8, "none", "LeakyReLU", False)
    runner.init_weights(G, "normal", 0.02)
    w = max(_conv_weights(G).values(), key=lambda t: t.numel())
    assert abs(float(w.std()) - 0.02) <= 0.1 * 0.02 and abs(float(w.mean())) <= 0.1 * 0.02
    for kind in ("xavier", "kaiming"):
        runner.init_weights(G, kind)
        assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in _conv_weights(G).values())
    for kind in ("none", "xavier_uniform", "", "Orthogonal"):
        with pytest.raises(NotImplementedError):
            runner.init_weights(G, kind)


# ---- shared fixtures ----
def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB")).copy()


def _nima_file(path):
    torch.save(nima.seeded_state_dict(7), path)
    return str(path)


def _load_scorer(path, dev):
    m = nima.NIMA()
    m.load_state_dict(torch.load(path, weights_only=True))
    return m.to(dev).eval()


# ---- --mode test ----
@pytest.mark.parametrize("backend", BACKENDS)
def test_test_mode_matches_run_test(backend, tmp_path, monkeypatch):
    dev = use_backend(backend)
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)            # a relative, dot-free data root: the sample name is the path up to its first '.'
    root = Path("data")
    root.mkdir()
    _make_tree(root, 5, [(40, 52), (36, 36), (61, 33)])
    torch.manual_seed(11)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    mdir = Path("results") / "UEGAN-FiveK" / "models"
    mdir.mkdir(parents=True)
    torch.save({"G_net": G.state_dict(), "D_net": D.state_dict()}, mdir / "UEGAN-FiveK_rahinge_2.0.pth")
    argv = ["--mode", "test", "--test_img_dir", "data", "--test_img_size", "32", "--g_conv_dim", "8", "--is_test_psnr_ssim", "True",
            "--compute_dtype", "float32", "--pretrained_model", "2.0", "--num_workers", "2", "--val_batch_size", "3"]
    scorer = None
    if backend == "gpu":
        argv += ["--nima_weights", _nima_file(tmp_path / "nima.pth")]
        scorer = _load_scorer(tmp_path / "nima.pth", dev)
    else:
        argv += ["--is_test_nima", "False"]
    got = runner.main(argv)

    # the parent API on the same tree (its enhance() calls recorded: the compare images are made of the same raw / fake tensors)
    G = G.to(dev)
    loader = data.get_test_loader("data", 32, 3, False, 2, device=dev)
    seen = []

    def enhance(G_, x):
        y = tester_enhance(G_, x)
        seen.append((x.detach().cpu().clone(), y.detach().cpu().clone()))
        return y
    tester_enhance = tester.enhance
    monkeypatch.setattr(tester, "enhance", enhance)
    want = tester.run_test(G, loader, save_dir="want", tag="2.00", nima=scorer)
    monkeypatch.setattr(tester, "enhance", tester_enhance)
    loader.close()
    out = Path("results") / "UEGAN-FiveK" / "test"
    names = sorted(os.listdir("want"))
    assert len(names) == 5 and sorted(os.listdir(out / "test_results")) == names
    for f in names:
        assert np.array_equal(_png(out / "test_results" / f), _png(Path("want") / f)), f
    pairs = torch.cat([O.to_uint8_image(torch.cat([raw, fake], 3)) for raw, fake in seen])
    assert [tuple(raw.shape[2:]) for raw, _ in seen] == [(32, 32), (32, 32)] and pairs.shape[0] == 5
    for i, name in enumerate(want["names"]):
        f = out / "test_compare" / ("%s_2.00_testRealRaw_testFakeExp.png" % name)
        assert np.array_equal(_png(f), pairs[i].numpy()), f
    assert len(os.listdir(out / "test_compare")) == 5
    with open(out / "test_metrics.json") as f:
        saved = json.load(f)
    keys = ["mean_psnr", "mean_ssim"] + (["mean_nima"] if scorer is not None else [])
    for k in keys:
        assert saved[k] == pytest.approx(want[k], rel=1e-12) and got[k] == saved[k], k
    assert saved["names"] == want["names"] and ("mean_nima" in saved) == (scorer is not None)


# ---- --mode train ----
def _train_argv(extra):
    return ["--mode", "train", "--train_img_dir", "data/train", "--val_img_dir", "data/val", "--image_size", "96", "--resize_size", "96",
            "--train_batch_size", "2", "--g_conv_dim", "8", "--d_conv_dim", "8", "--vgg_weights", "seeded", "--pool_size", "3", "--test_img_size", "32",
            "--val_batch_size", "2", "--model_save_epoch", "1", "--lr_num_epochs_decay", "1", "--lr_decay_ratio", "2", "--compute_dtype", "float32",
            "--num_workers", "2"] + extra


def _trees():
    for sub, n, sizes in (("train", 4, [(100, 110)]), ("val", 3, [(40, 52), (36, 36)])):
        root = Path("data") / sub
        root.mkdir(parents=True)
        _make_tree(root, n, sizes)


class _Spy:
    """wraps Trainer.train_step / loss_items: per call the generator's learning rate and weights at entry and the step's fake_exp"""

    def __init__(self, monkeypatch, keep_weights=False):
        self.lrs, self.fakes, self.weights, self.loss_reads = [], [], [], 0
        step, items = trainer.Trainer.train_step, trainer.Trainer.loss_items
        spy = self

        def train_step(self, real_raw, real_exp):
            spy.lrs.append(self.g_optimizer.lr)
            if keep_weights:
                spy.weights.append({k: v.detach().cpu().clone() for k, v in self.G.state_dict().items()})
            out = step(self, real_raw, real_exp)
            spy.fakes.append(self.fake_exp.detach().cpu().clone())
            return out

        def loss_items(self):
            spy.loss_reads += 1
            return items(self)

        monkeypatch.setattr(trainer.Trainer, "train_step", train_step)
        monkeypatch.setattr(trainer.Trainer, "loss_items", loss_items)


@pytest.mark.gpu
def test_train_mode_end_to_end(tmp_path, monkeypatch):
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    _trees()
    argv = _train_argv(["--total_epochs", "3", "--num_epochs_start_val", "1", "--val_each_epochs", "1", "--info_step", "2", "--sample_step", "3",
                        "--is_test_psnr_ssim", "True", "--nima_weights", _nima_file(tmp_path / "nima.pth")])
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        runner.main(argv)
    out = Path("results") / "UEGAN-FiveK"
    ver = "UEGAN-FiveK_rahinge_"

    # checkpoints: the reference's names (float epoch) and keys
    assert sorted(os.listdir(out / "models")) == [ver + "1.0.pth", ver + "2.0.pth", ver + "3.0.pth"]
    for e in (1.0, 2.0, 3.0):
        ck = torch.load(out / "models" / (ver + "%s.pth" % e), weights_only=True)
        assert set(ck) == CKPT_KEYS and ck["epoch"] == e

    # validation: strictly after --num_epochs_start_val epochs (trainer.py:214), so not at the end of epoch 1.0
    assert sorted(os.listdir(out / "validation")) == ["validation.jsonl", "validation_2.0", "validation_3.0", "validation_compare_2.0",
                                                      "validation_compare_3.0"]
    for e in ("2.0", "3.0"):
        fakes = sorted(os.listdir(out / "validation" / ("validation_" + e)))
        pairs = sorted(os.listdir(out / "validation" / ("validation_compare_" + e)))
        assert fakes == ["im%02d_%s0_valFakeExp.png" % (i, e) for i in range(3)]
        assert pairs == ["im%02d_%s0_valRealRaw_valFakeExp.png" % (i, e) for i in range(3)]
        assert _png(out / "validation" / ("validation_" + e) / fakes[0]).shape == (32, 32, 3)
        assert _png(out / "validation" / ("validation_compare_" + e) / pairs[0]).shape == (32, 64, 3)
    with open(out / "validation" / "validation.jsonl") as f:
        lines = [json.loads(s) for s in f]
    assert [r.get("epoch") for r in lines] == [2.0, 3.0, None] and set(lines[-1]) == {"best"}
    for k in ("nima", "psnr", "ssim"):
        vals = [r[k] for r in lines[:2]]
        assert all(np.isfinite(v) and v > 0 for v in vals)
        best = lines[-1]["best"][k]
        assert best["value"] == max(vals) and lines[:2][[r[k] for r in lines[:2]].index(best["value"])]["epoch"] == best["epoch"]

    # samples at steps 3 and 6: raw | fake | exp side by side, the middle panel is that step's fake_exp
    assert len(spy.fakes) == 6
    samples = sorted(os.listdir(out / "samples"))
    assert len(samples) == 4
    for step, tag in ((3, "1.50"), (6, "3.00")):
        mine = [s for s in samples if "_%s_" % tag in s]
        assert len(mine) == 2 and all(s.endswith("_realRaw_fakeExp_realExp.png") for s in mine)
        want = O.to_uint8_image(spy.fakes[step - 1])
        for s in mine:
            i = int(s.split("_")[2])
            img = _png(out / "samples" / s)
            assert img.shape == (96, 288, 3)
            assert np.array_equal(img[:, 96:192], want[i].numpy()), s

    # a step that prints nothing reads nothing: 6 steps, --info_step 2
    assert spy.loss_reads == 3
    # the schedule: set_epoch(e) after step e * steps_per_epoch (trainer.py:131-134), seen at the entry of the next step
    for e in (0, 1, 2):
        assert spy.lrs[2 * e + 1] == pytest.approx(1e-4 * trainer.lambda_rule(e, 1, 2), rel=1e-12, abs=0.0)
    with open(out / "logs" / "train_log.jsonl") as f:
        log = [json.loads(s) for s in f]
    assert [r["step"] for r in log] == [2, 4, 6] and [r["epoch"] for r in log] == [1.0, 2.0, 3.0]

    # the same six steps without the runner
    runner.setup_seed(1990)
    G = models.Generator(8, "none", "LeakyReLU", False)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge")
    runner.init_weights(G, "orthogonal", 0.02)
    runner.init_weights(D, "orthogonal", 0.02)
    P = losses.PerceptualLoss(vgg_weights="seeded")
    loader = data.get_train_loader("data/train", 96, 96, 2, True, 2, True, device=dev, generator=runner.loader_generator(1990))
    T = trainer.Trainer(G.to(dev), D.to(dev), P.to(dev), pool_size=3)
    T.lr_scheduler_g.lr_lambda = T.lr_scheduler_d.lr_lambda = lambda e: trainer.lambda_rule(e, 1, 2)      # (1 at epoch 0: the initial rates stand)
    fetcher = data.InputFetcher(loader)
    for step in range(6):
        batch = next(fetcher)
        T.train_step(batch.img_raw, batch.img_exp)
        if (step + 1) % 2 == 0:
            _check_losses(log[step // 2], [T.loss_items()[k] for k in NAMES], step + 1)
        if step % 2 == 0:
            T.set_epoch(step // 2)
    loader.close()

    # and the checkpoint the run ended with serves --mode test
    res = runner.main(["--mode", "test", "--test_img_dir", "data/val", "--test_img_size", "32", "--g_conv_dim", "8", "--pretrained_model", "3.0",
                       "--compute_dtype", "float32", "--is_test_nima", "False", "--is_test_psnr_ssim", "True", "--num_workers", "2", "--val_batch_size", "2"])
    assert res["mean_psnr"] == lines[1]["psnr"] and res["mean_ssim"] == lines[1]["ssim"]


@pytest.mark.gpu
def test_train_mode_resumes(tmp_path, monkeypatch):
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    monkeypatch.chdir(tmp_path)
    _trees()
    quiet = ["--num_epochs_start_val", "9", "--info_step", "100", "--sample_step", "100", "--is_test_nima", "False"]
    runner.main(_train_argv(quiet + ["--total_epochs", "1"]))
    mdir = Path("results") / "UEGAN-FiveK" / "models"
    assert os.listdir(mdir) == ["UEGAN-FiveK_rahinge_1.0.pth"]
    saved = torch.load(mdir / "UEGAN-FiveK_rahinge_1.0.pth", weights_only=True, map_location="cpu")
    with monkeypatch.context() as mp:
        spy = _Spy(mp, keep_weights=True)
        runner.main(_train_argv(quiet + ["--total_epochs", "2", "--pretrained_model", "1.0"]))
    assert len(spy.fakes) == 2 and spy.loss_reads == 0
    assert set(spy.weights[0]) == set(saved["G_net"]) and all(torch.equal(spy.weights[0][k], saved["G_net"][k]) for k in saved["G_net"])
    assert not all(torch.equal(spy.weights[1][k], saved["G_net"][k]) for k in saved["G_net"])
    assert spy.lrs[0] == pytest.approx(1e-4 * trainer.lambda_rule(0, 1, 2))          # the optimizer's state as saved after epoch 1.0
    assert sorted(os.listdir(mdir)) == ["UEGAN-FiveK_rahinge_1.0.pth", "UEGAN-FiveK_rahinge_2.0.pth"]
    assert not os.path.exists(Path("results") / "UEGAN-FiveK" / "logs" / "train_log.jsonl")


# ---- Trainer(idt_loss_type=) ----
@pytest.mark.gpu
def test_trainer_idt_loss_type_l2():
    dev = use_backend("gpu")
    ops.set_compute_dtype(torch.float32)
    torch.manual_seed(21)
    G = models.Generator(8, "none", "LeakyReLU", False).to(dev)
    D = models.Discriminator(8, "none", "LeakyReLU", True, "rahinge").to(dev)
    P = losses.PerceptualLoss(vgg_weights="seeded", width_div=8).to(dev)
    T = trainer.Trainer(G, D, P, pool_size=0, rng=random.Random(3), idt_loss_type="l2")
    g = torch.Generator().manual_seed(22)
    raw = (torch.rand(2, 3, 96, 96, generator=g) * 2 - 1).to(dev)
    exp = (torch.rand(2, 3, 96, 96, generator=g) * 2 - 1).to(dev)
    with torch.no_grad():
        idt = G(exp)
        want = 0.1 * float(losses.MultiscaleRecLoss(3, "l2", True)(idt, exp))
        other = 0.1 * float(losses.MultiscaleRecLoss(3, "l1", True)(idt, exp))
    T.train_step(raw, exp)
    got = T.loss_items()["g_idt"]
    assert abs(got - want) <= 1e-3 * abs(want) + 1e-6, (got, want)
    assert abs(got - other) > 10 * (1e-3 * abs(other) + 1e-6), (got, other)          # (the two criteria differ on this input)
