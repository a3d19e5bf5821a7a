"""Command-line flags of `python -m uegan_amd`: the reference's flag table (config.py:11-81: same names, types and defaults) plus the
project's own switches.

    get_config(argv=None)   parse (sys.argv[1:] when argv is None) -> argparse.Namespace; touches no device and no file
    validate(args)          the start-up refusals: what the flags ask for and this project does not do, each naming its flag

Differences from the reference, on purpose:
  * booleans accept true/false/1/0/yes/no in any letter case and reject everything else.  The reference's `str2bool` is a substring test
    (`v.lower() in 'true'`: "", "t", "ru" are True, "1" and "yes" are False) and its `--shuffle` / `--use_tensorboard` are `type=str`, so
    `--shuffle False` is the truthy string "False"; neither is reproduced.
  * `--gpu_ids` parses "0,1,2,3" into a list of ints (the reference has no type there: a value given on the command line stays a string).
"""
import argparse

import torch

_TRUE, _FALSE = ("true", "1", "yes"), ("false", "0", "no")


def str2bool(v):
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in _TRUE:
        return True
    if s in _FALSE:
        return False
    raise argparse.ArgumentTypeError("expected one of true/false/1/0/yes/no, got %r" % (v,))


def int_list(v):
    if isinstance(v, (list, tuple)):
        return [int(i) for i in v]
    return [int(i) for i in str(v).replace("[", "").replace("]", "").split(",") if i.strip()]


# (name, type, default, help) in the reference's order and sections
_MODEL = [
    ("mode", str, "train", "train|test"),
    ("adv_loss_type", str, "rahinge", "quality loss: ls|original|hinge|rahinge|rals"),
    ("image_size", int, 512, "side of the random training crop"),
    ("resize_size", int, 256, "side of the training image after resizing the crop"),
    ("test_img_size", int, 512, "side of validation and test images after resizing; 0: no resizing, every image is enhanced and scored at its own size"),
    ("g_conv_dim", int, 32, "filters of the generator's first layer"),
    ("d_conv_dim", int, 32, "filters of the discriminator's first layer"),
    ("shuffle", str2bool, True, "shuffle the training set"),
    ("drop_last", str2bool, True, "drop the last incomplete training batch"),
    ("version", str, "UEGAN-FiveK", "name of the run: sub-directory of --save_root_dir and prefix of the checkpoint files"),
    ("init_type", str, "orthogonal", "normal|xavier|kaiming|orthogonal"),
    ("adv_input", str2bool, True, "the discriminator also sees the raw input as a fake"),
    ("g_use_sn", str2bool, False, "spectral normalisation in the generator"),
    ("d_use_sn", str2bool, True, "spectral normalisation in the discriminator"),
    ("g_act_fun", str, "LeakyReLU", "LeakyReLU|ReLU|Swish|SELU|none"),
    ("d_act_fun", str, "LeakyReLU", "LeakyReLU|ReLU|Swish|SELU|none"),
    ("g_norm_fun", str, "none", "BatchNorm|InstanceNorm|none"),
    ("d_norm_fun", str, "none", "BatchNorm|InstanceNorm|none"),
]
_TRAINING = [
    ("pretrained_model", float, 0.0, "epoch of the checkpoint to resume from (train) or to evaluate (test); 0: from scratch"),
    ("total_epochs", int, 100, "epochs to train"),
    ("train_batch_size", int, 10, "training batch"),
    ("val_batch_size", int, 1, "validation and test batch"),
    ("num_workers", int, 8, "image decoding workers"),
    ("seed", int, 1990, "seed of every random number generator"),
    ("g_lr", float, 1e-4, "generator learning rate"),
    ("d_lr", float, 4e-4, "discriminator learning rate"),
    ("lr_decay", str2bool, True, "step the learning-rate schedule at the first step of every epoch"),
    ("lr_num_epochs_decay", int, 50, "epoch at which the linear decay starts"),
    ("lr_decay_ratio", int, 50, "epochs over which the rate decays to zero"),
    ("optimizer_type", str, "adam", "adam|rmsprop"),
    ("beta1", float, 0.5, "Adam beta1"),
    ("beta2", float, 0.999, "Adam beta2"),
    ("alpha", float, 0.9, "RMSprop alpha"),
    ("lambda_adv", float, 0.10, "weight of the quality (adversarial) loss"),
    ("lambda_percep", float, 1.0, "weight of the fidelity (VGG) loss"),
    ("lambda_idt", float, 0.10, "weight of the identity loss"),
    ("idt_loss_type", str, "l1", "identity loss: l1|l2|smoothl1"),
    ("pool_size", int, 50, "history buffer of generated images; 0: none"),
]
_VALIDATION = [
    ("num_epochs_start_val", int, 8, "validate only after this many epochs"),
    ("val_each_epochs", int, 2, "validate every this many epochs"),
]
_DIRECTORIES = [
    ("train_img_dir", str, "./data/fivek/train", None),
    ("val_img_dir", str, "./data/fivek/val", None),
    ("test_img_dir", str, "./data/fivek/test", None),
    ("save_root_dir", str, "./results", None),
    ("val_label_dir", str, "./data/fivek/val/label/", "unused: the labels come from the val loader (second sub-folder of --val_img_dir)"),
    ("test_label_dir", str, "./data/fivek/test/label/", "unused: the labels come from the test loader (second sub-folder of --test_img_dir)"),
    ("model_save_path", str, "models", None),
    ("sample_path", str, "samples", None),
    ("log_path", str, "logs", None),
    ("val_result_path", str, "validation", None),
    ("test_result_path", str, "test", None),
]
_STEPS = [
    ("log_step", int, 100, "TensorBoard period of the reference: unused"),
    ("info_step", int, 100, "print and log the losses every this many steps"),
    ("sample_step", int, 100, "write sample images every this many steps"),
    ("model_save_epoch", int, 1, "write a checkpoint every this many epochs"),
]
_MISC = [
    ("parallel", str2bool, False, "refused: multi-GPU training goes through trainer.Trainer(group=) (tools/dist_smoke.py)"),
    ("gpu_ids", int_list, [0, 1, 2, 3], "unused (see --parallel)"),
    ("use_tensorboard", str2bool, False, "refused: the losses go to <log_path>/train_log.jsonl"),
    ("is_print_network", str2bool, True, "print the parameter counts"),
    ("is_test_nima", str2bool, True, "NIMA score of the enhanced images (needs --nima_weights)"),
    ("is_test_psnr_ssim", str2bool, False, "PSNR / SSIM of the enhanced images against the labels"),
]
REFERENCE_FLAGS = _MODEL + _TRAINING + _VALIDATION + _DIRECTORIES + _STEPS + _MISC

COMPUTE_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m uegan_amd", description="Train or test UEGAN on one MI355X.")
    for title, flags in (("model", _MODEL), ("training", _TRAINING), ("validation", _VALIDATION), ("directories", _DIRECTORIES),
                         ("periods", _STEPS), ("misc", _MISC)):
        group = parser.add_argument_group(title)
        for name, typ, default, text in flags:
            group.add_argument("--" + name, type=typ, default=default, help=text)
    group = parser.add_argument_group("this project")
    group.add_argument("--compute_dtype", choices=sorted(COMPUTE_DTYPES), default="bfloat16",
                       help="storage dtype of activations and packed weights (uegan_amd.set_compute_dtype)")
    group.add_argument("--precise", type=str2bool, default=False, help="hi + lo pairs for the generator's full-resolution tensors (uegan_amd.set_precise)")
    group.add_argument("--vgg_weights", type=str, default=None,
                       help="vgg19-dcbb9e9d.pth, or 'seeded' for the stand-in; default: PerceptualLoss's own search ($UEGAN_VGG19_WEIGHTS, ./models/)")
    group.add_argument("--nima_weights", type=str, default=None, help="state dict of uegan_amd.nima.NIMA (needed by --is_test_nima True)")
    return parser


def get_config(argv=None):
    return build_parser().parse_args(argv)


def validate(args):
    """Refuse at start-up what would otherwise fail late or be silently ignored."""
    if args.parallel:
        raise NotImplementedError("--parallel True is not supported by this command line: one process drives one GPU.  Multi-GPU training goes "
                                  "through trainer.Trainer(group=...), one process per GPU (tools/dist_smoke.py); run with --parallel False")
    if args.use_tensorboard:
        raise NotImplementedError("--use_tensorboard True is not supported: the losses are appended to <save_root_dir>/<version>/<log_path>/"
                                  "train_log.jsonl; run with --use_tensorboard False")
    if args.is_test_nima and not args.nima_weights:
        raise ValueError("--is_test_nima True (the default) needs --nima_weights PATH, a state dict for uegan_amd.nima.NIMA; "
                         "pass it, or run with --is_test_nima False")
    return args
