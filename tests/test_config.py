"""uegan_amd/config.py: the reference's flag table (config.py:11-81) with strict booleans, the project's own flags, the start-up refusals and
`python -m uegan_amd --help`.  No device is touched."""
import os
import subprocess
import sys

import pytest

from helpers import ROOT
from uegan_amd import config, runner

# every flag of the reference with its default (config.py:11-81), typed here by hand
REFERENCE_DEFAULTS = {
    "mode": "train", "adv_loss_type": "rahinge", "image_size": 512, "resize_size": 256, "test_img_size": 512, "g_conv_dim": 32, "d_conv_dim": 32,
    "shuffle": True, "drop_last": True, "version": "UEGAN-FiveK", "init_type": "orthogonal", "adv_input": True, "g_use_sn": False, "d_use_sn": True,
    "g_act_fun": "LeakyReLU", "d_act_fun": "LeakyReLU", "g_norm_fun": "none", "d_norm_fun": "none",
    "pretrained_model": 0.0, "total_epochs": 100, "train_batch_size": 10, "val_batch_size": 1, "num_workers": 8, "seed": 1990, "g_lr": 1e-4,
    "d_lr": 4e-4, "lr_decay": True, "lr_num_epochs_decay": 50, "lr_decay_ratio": 50, "optimizer_type": "adam", "beta1": 0.5, "beta2": 0.999,
    "alpha": 0.9, "lambda_adv": 0.10, "lambda_percep": 1.0, "lambda_idt": 0.10, "idt_loss_type": "l1", "pool_size": 50,
    "num_epochs_start_val": 8, "val_each_epochs": 2,
    "train_img_dir": "./data/fivek/train", "val_img_dir": "./data/fivek/val", "test_img_dir": "./data/fivek/test", "save_root_dir": "./results",
    "val_label_dir": "./data/fivek/val/label/", "test_label_dir": "./data/fivek/test/label/", "model_save_path": "models", "sample_path": "samples",
    "log_path": "logs", "val_result_path": "validation", "test_result_path": "test",
    "log_step": 100, "info_step": 100, "sample_step": 100, "model_save_epoch": 1,
    "parallel": False, "gpu_ids": [0, 1, 2, 3], "use_tensorboard": False, "is_print_network": True, "is_test_nima": True, "is_test_psnr_ssim": False,
}
PROJECT_DEFAULTS = {"compute_dtype": "bfloat16", "precise": False, "vgg_weights": None, "nima_weights": None}


def test_defaults_are_the_references():
    got = vars(config.get_config([]))
    assert set(got) == set(REFERENCE_DEFAULTS) | set(PROJECT_DEFAULTS)
    for k, want in {**REFERENCE_DEFAULTS, **PROJECT_DEFAULTS}.items():
        assert got[k] == want and type(got[k]) is type(want), (k, got[k], want)
    assert [f[0] for f in config.REFERENCE_FLAGS] == list(REFERENCE_DEFAULTS)          # the reference's order too


def test_values_parse_to_the_flags_types():
    a = config.get_config(["--mode", "test", "--image_size", "96", "--pretrained_model", "2.5", "--g_lr", "3e-4", "--gpu_ids", "0,2",
                           "--compute_dtype", "float32", "--vgg_weights", "seeded", "--nima_weights", "w.pth", "--precise", "yes"])
    assert (a.mode, a.image_size, a.pretrained_model, a.g_lr, a.gpu_ids) == ("test", 96, 2.5, 3e-4, [0, 2])
    assert (a.compute_dtype, a.vgg_weights, a.nima_weights, a.precise) == ("float32", "seeded", "w.pth", True)
    with pytest.raises(SystemExit):
        config.get_config(["--compute_dtype", "float64"])


@pytest.mark.parametrize("flag", ["shuffle", "drop_last", "adv_input", "lr_decay", "use_tensorboard", "is_test_nima", "precise"])
def test_booleans_are_strict(flag):
    for text in ("true", "True", "TRUE", "1", "yes", "Yes"):
        assert getattr(config.get_config(["--" + flag, text]), flag) is True
    for text in ("false", "False", "FALSE", "0", "no", "NO"):
        assert getattr(config.get_config(["--" + flag, text]), flag) is False
    for text in ("", "t", "ru", "tru", "2", "on", "none", "truefalse"):          # the reference's substring test takes the first four for True
        with pytest.raises(SystemExit):
            config.get_config(["--" + flag, text])


OK = ["--is_test_nima", "False"]


@pytest.mark.parametrize("argv,exc,words", [
    (OK + ["--parallel", "True"], NotImplementedError, ["--parallel", "dist_smoke"]),
    (OK + ["--use_tensorboard", "True"], NotImplementedError, ["--use_tensorboard"]),
    ([], ValueError, ["--is_test_nima False", "--nima_weights"]),
    (["--is_test_nima", "True"], ValueError, ["--is_test_nima False", "--nima_weights"]),
])
def test_startup_refusals_name_their_flag(argv, exc, words, tmp_path, monkeypatch):
    with pytest.raises(exc) as e:
        config.validate(config.get_config(argv))
    for w in words:
        assert w in str(e.value)
    monkeypatch.chdir(tmp_path)
    for mode in ("train", "test"):
        with pytest.raises(exc):
            runner.main(argv + ["--mode", mode])
    assert os.listdir(tmp_path) == []               # refused before anything was created


def test_accepted_configurations_and_unknown_mode():
    config.validate(config.get_config(OK))
    config.validate(config.get_config(["--nima_weights", "nima.pth"]))
    with pytest.raises(NotImplementedError):
        runner.main(OK + ["--mode", "export"])


def test_module_help_exits_zero():
    r = subprocess.run([sys.executable, "-m", "uegan_amd", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--mode", "--pretrained_model", "--compute_dtype", "--nima_weights", "--vgg_weights", "--precise"):
        assert flag in r.stdout
