"""`python -m uegan_amd --mode train|test`: the reference's main.py, Trainer.train (trainer.py:39-146) and Tester.test (tester.py:41-103)
over this package's pieces -- data.get_train_loader / get_test_loader / InputFetcher, trainer.Trainer, tester.run_test, nima.NIMA.

    main(argv=None)                        parse (config.get_config), refuse what is not supported (config.validate), seed, dispatch on --mode
    train(args)                            the epoch loop: train_step, loss line + samples + checkpoints, validation with best-epoch tracking
    test(args)                             enhance a test set from a checkpoint: images, compare montages, NIMA / PSNR / SSIM
    init_weights(net, init_type, gain)     trainer.py:357-390
    setup_seed(seed)                       utils.py:149-155

What differs from the reference, on purpose:
  * validation and test loaders are not shuffled (the reference shuffles both: main.py:37,45): the order only decides which file is written
    first, and a fixed order makes the logged means reproducible to the last bit.
  * the val loader resizes to --test_img_size (main.py:35-38 passes no size, so the reference validates at 512 whatever the flag says).
  * PSNR / SSIM compare against the loader's label image (--test_img_size 0: against the label file as it is), NIMA / PSNR / SSIM means are true
    means (tester.run_test's docstring).
  * --test_img_size 0 is the native size (tester.enhance_native): no resize, outputs at the size of their source, "sizes" in test_metrics.json.
  * the training loader draws from its own generator seeded with --seed (`loader_generator`), not from the global one: what validation or a
    sample draws never shifts the training data.
  * UEGAN_PNG_ENCODER=device in the environment: samples, validation and test images are encoded on the device (tester.write_pngs); same pixels.
  * UEGAN_IMAGE_FORMAT=jpeg (with UEGAN_JPEG_QUALITY=1..100, default 95) in the environment: those files are baseline JPEGs named .jpg, encoded on
    the device (tester.write_images); the metrics are computed before encoding and equal those of a PNG run.  UEGAN_JPEG_OPTIMIZE=1 with it:
    every file carries its own Huffman tables (smaller files, the same pixels after decoding).
  * UEGAN_DATASET_CACHE=device (with UEGAN_DATASET_CACHE_GB=<GiB per loader>, default 16) in the environment: the train, validation and test
    loaders keep every decoded file in device memory from its first touch on (data.set_dataset_cache); the same tensors.  validation.jsonl then
    carries each validation's hits / misses / declined under "dataset_cache".
  * a step that prints nothing reads nothing from the device: the five losses are fetched (Trainer.loss_items) every --info_step only.
"""
import json
import os
import random
import time

import numpy as np
import torch

from . import _lib as L
from . import config, data, models, nima, ops, tester, trainer
from .losses import PerceptualLoss


def setup_seed(seed):
    """utils.py:149-155 (its two cudnn switches have no counterpart: no kernel of this package goes through a vendor library)"""
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def loader_generator(seed):
    """the generator `train` hands to its training loader (shuffle order, crops, flips)"""
    return torch.Generator().manual_seed(int(seed))


def init_weights(net, init_type="kaiming", gain=0.02):
    """trainer.py:357-390 for the four documented types: every module whose class name contains 'Conv' and that has `.weight` (for a
    spectral-norm convolution that is weight_orig) gets the named initialisation and a zero bias; the affine norm layers of the
    BatchNorm / InstanceNorm variants get weight ~ N(1, gain), bias 0.  Draws from torch's global generator, module by module in
    `net.modules()` order.  Anything else raises NotImplementedError."""
    if init_type not in ("normal", "xavier", "kaiming", "orthogonal"):
        raise NotImplementedError("Initialization method [{}] is not implemented".format(init_type))
    with torch.no_grad():
        for m in net.modules():
            name = type(m).__name__
            w = getattr(m, "weight", None)
            b = getattr(m, "bias", None)
            if "Conv" in name and w is not None:
                if init_type == "normal":
                    torch.nn.init.normal_(w, 0.0, gain)
                elif init_type == "xavier":
                    torch.nn.init.xavier_normal_(w, gain=gain)
                elif init_type == "kaiming":
                    torch.nn.init.kaiming_normal_(w, a=0, mode="fan_in")
                else:
                    torch.nn.init.orthogonal_(w, gain=gain)
            elif ("BatchNorm2d" in name or "InstanceNorm2d" in name) and w is not None:
                torch.nn.init.normal_(w, 1.0, gain)
            else:
                continue
            if b is not None:
                b.zero_()
    ops.invalidate_weight_caches()
    return net


def _device():
    return torch.device("cpu") if L.is_emulated() else torch.device("cuda:0")


def _paths(args):
    root = os.path.join(args.save_root_dir, args.version)
    return {k: os.path.join(root, getattr(args, k)) for k in ("model_save_path", "sample_path", "log_path", "val_result_path", "test_result_path")}


def checkpoint_name(args, epoch):
    """trainer.py:208 / :403: `epoch` is the float (step + 1) / steps_per_epoch, so the files read ..._1.0.pth, ..._2.0.pth"""
    return "{}_{}_{}.pth".format(args.version, args.adv_loss_type, epoch)


def _apply_modes(args):
    ops.set_compute_dtype(config.COMPUTE_DTYPES[args.compute_dtype])
    ops.set_precise(args.precise)


def _count(net, name, args):
    if args.is_print_network:
        n = sum(p.numel() for p in net.parameters())
        print("=== [{}]: {} parameters ({:.4f} M) ===".format(name, n, n / 1e6))


def build_generator(args, dev):
    G = models.Generator(args.g_conv_dim, args.g_norm_fun, args.g_act_fun, args.g_use_sn)
    _count(G, "Generator", args)
    return G.to(dev) if dev.type != "cpu" else G


def _load_nima(args, dev):
    if not args.is_test_nima:
        return None
    model = nima.NIMA()
    model.load_state_dict(torch.load(args.nima_weights, map_location="cpu", weights_only=True))
    return model.to(dev).eval()


class _Best:
    """trainer.py:47-52,266-283: best value and its epoch per metric, strict `<`, starting from 0.0 at epoch 0"""

    def __init__(self, names):
        self.value = {k: 0.0 for k in names}
        self.epoch = {k: 0 for k in names}

    def update(self, name, value, epoch):
        if self.value[name] < value:
            self.value[name], self.epoch[name] = value, epoch

    def as_dict(self):
        return {k: {"value": self.value[k], "epoch": self.epoch[k]} for k in self.value}


def _append(path, record):
    with open(path, "a") as f:
        f.write(json.dumps(record) + "\n")


def validate_epoch(args, G, loader, scorer, out_root, epoch, best):
    """trainer.py:213-286: enhance the validation set, write `validation_<epoch>/` and `validation_compare_<epoch>/`, score, track the best"""
    tag = "{:0>3.2f}".format(epoch)
    before = (loader.cache_hits, loader.cache_misses, loader.cache_declined)
    res = tester.run_test(G, loader, save_dir=os.path.join(out_root, "validation_" + str(epoch)), tag=tag, metrics=args.is_test_psnr_ssim, nima=scorer,
                          suffix="valFakeExp", compare_dir=os.path.join(out_root, "validation_compare_" + str(epoch)),
                          compare_suffix="valRealRaw_valFakeExp")
    record = {"epoch": epoch, "images": len(res["names"])}
    if loader.cache == "device":      # this validation's touches of the resident store: from the second validation on there are no misses
        record["dataset_cache"] = {"hits": loader.cache_hits - before[0], "misses": loader.cache_misses - before[1],
                                   "declined": loader.cache_declined - before[2]}
    if scorer is not None:
        record["nima"] = res["mean_nima"]
        best.update("nima", res["mean_nima"], epoch)
        print("====== Avg. NIMA: {:>.4f} ======".format(res["mean_nima"]))
    if args.is_test_psnr_ssim:
        record["psnr"], record["ssim"] = res["mean_psnr"], res["mean_ssim"]
        best.update("psnr", res["mean_psnr"], epoch)
        best.update("ssim", res["mean_ssim"], epoch)
        print("====== Avg. PSNR: {:>.4f} dB ======".format(res["mean_psnr"]))
        print("====== Avg. SSIM: {:>.4f}  ======".format(res["mean_ssim"]))
    _append(os.path.join(out_root, "validation.jsonl"), record)
    return record


def train(args):
    dev = _device()
    _apply_modes(args)
    paths = _paths(args)
    for p in paths.values():
        os.makedirs(p, exist_ok=True)
    G = models.Generator(args.g_conv_dim, args.g_norm_fun, args.g_act_fun, args.g_use_sn)                              # trainer.py:315-316
    D = models.Discriminator(args.d_conv_dim, args.d_norm_fun, args.d_act_fun, args.d_use_sn, args.adv_loss_type)
    _count(G, "Generator", args)
    _count(D, "Discriminator", args)
    if args.init_type:                                                                                                 # :330-332
        init_weights(G, args.init_type, 0.02)
        init_weights(D, args.init_type, 0.02)
    if dev.type != "cpu":
        G, D = G.to(dev), D.to(dev)
    percep = PerceptualLoss(vgg_weights=args.vgg_weights)
    percep = percep.to(dev) if dev.type != "cpu" else percep
    scorer = _load_nima(args, dev)
    loader = data.get_train_loader(args.train_img_dir, args.image_size, args.resize_size, args.train_batch_size, args.shuffle, args.num_workers,
                                   args.drop_last, device=dev, generator=loader_generator(args.seed))
    val_loader = data.get_test_loader(args.val_img_dir, args.test_img_size, args.val_batch_size, False, args.num_workers, device=dev)
    try:
        return _train_loop(args, dev, paths, G, D, percep, scorer, loader, val_loader)
    finally:
        loader.close()
        val_loader.close()


def _train_loop(args, dev, paths, G, D, percep, scorer, loader, val_loader):
    T = trainer.Trainer(G, D, percep, pool_size=args.pool_size, g_lr=args.g_lr, d_lr=args.d_lr, beta1=args.beta1, beta2=args.beta2,
                        lambda_adv=args.lambda_adv, lambda_percep=args.lambda_percep, lambda_idt=args.lambda_idt, adv_input=args.adv_input,
                        adv_loss_type=args.adv_loss_type, optimizer_type=args.optimizer_type, alpha=args.alpha, idt_loss_type=args.idt_loss_type)

    def rule(epoch):                                                                                                   # trainer.py:348-349
        return trainer.lambda_rule(epoch, args.lr_num_epochs_decay, args.lr_decay_ratio)
    if args.lr_decay:                                       # (--lr_decay False: the rates stay at --g_lr / --d_lr, no scheduler ever steps)
        for sch in (T.lr_scheduler_g, T.lr_scheduler_d):
            sch.lr_lambda = rule
            sch._apply()                                    # LambdaLR's initial step (epoch 0) under the flags' rule

    steps_per_epoch = len(loader)
    if steps_per_epoch == 0:
        raise ValueError("--train_img_dir %s holds fewer image pairs than one batch (--train_batch_size %d)" % (args.train_img_dir, args.train_batch_size))
    model_save_step = int(args.model_save_epoch * steps_per_epoch)
    total_steps = int(args.total_epochs * steps_per_epoch)
    val_start_steps = int(args.num_epochs_start_val * steps_per_epoch)
    val_each_steps = int(args.val_each_epochs * steps_per_epoch)
    start_step = 0
    if args.pretrained_model:                                                                                          # :60-62, :402-423
        start_step = int(args.pretrained_model * steps_per_epoch)
        T.load_checkpoint(os.path.join(paths["model_save_path"], checkpoint_name(args, args.pretrained_model)), map_location=dev)
        print("=========== loaded trained models (epochs: {})! ===========".format(args.pretrained_model))
    best = _Best((["nima"] if scorer is not None else []) + (["psnr", "ssim"] if args.is_test_psnr_ssim else []))
    log_file = os.path.join(paths["log_path"], "train_log.jsonl")
    fetcher = data.InputFetcher(loader)
    print("======================================= start training =======================================")
    t0 = time.time()
    for step in range(start_step, total_steps):
        batch = next(fetcher)
        real_raw, real_exp = batch.img_raw, batch.img_exp
        T.train_step(real_raw, real_exp)                                                                               # :77-119
        epoch = (step + 1) / steps_per_epoch

        if (step + 1) % args.info_step == 0:                                                                           # :174-177
            v = T.loss_items()
            elapsed = time.time() - t0
            print("Elapse:{:>.12s}, D_Step:{:>6d}/{}, G_Step:{:>6d}/{}, D_loss:{:>.4f}, G_loss:{:>.4f}, G_percep_loss:{:>.4f}, G_adv_loss:{:>.4f}, "
                  "G_idt_loss:{:>.4f}".format(_hms(elapsed), step + 1, total_steps, step + 1, total_steps, v["d_loss"], v["g_loss"], v["g_percep"],
                                              v["g_adv"], v["g_idt"]))
            _append(log_file, dict(step=step + 1, epoch=epoch, elapsed_s=round(elapsed, 3), **v))
        if (step + 1) % args.sample_step == 0:                                                                         # :180-183
            tester.write_images([os.path.join(paths["sample_path"], "{:s}_{:0>3.2f}_{:0>2d}_realRaw_fakeExp_realExp.png".format(name, epoch, i))
                                 for i, name in enumerate(batch.img_name)], tester.montage_u8(real_raw, T.fake_exp, real_exp))
        if model_save_step and (step + 1) % model_save_step == 0:                                                      # :186-210
            T.save_checkpoint(os.path.join(paths["model_save_path"], checkpoint_name(args, epoch)), epoch)
            print("======= Save model checkpoints into {} ======".format(paths["model_save_path"]))

        if (step + 1) > val_start_steps and val_each_steps and (step + 1) % val_each_steps == 0:                       # :214-215
            validate_epoch(args, G, val_loader, scorer, paths["val_result_path"], epoch, best)

        if args.lr_decay and step % steps_per_epoch == 0:                                                              # :131-138
            T.set_epoch(step // steps_per_epoch)
            print("====== Epoch: {:>3d}/{}, learning rate of G: [{}], of D: [{}] ======".format((step + 1) // steps_per_epoch, args.total_epochs,
                                                                                             T.g_optimizer.lr, T.d_optimizer.lr))
    T.sync()
    if best.value:                                                                                                     # :143, :289-309
        _append(os.path.join(paths["val_result_path"], "validation.jsonl"), {"best": best.as_dict()})
    print("=========== Complete training ===========")
    return T


def _hms(seconds):
    s = int(seconds)
    return "%d:%02d:%02d" % (s // 3600, s // 60 % 60, s % 60)


def test(args):
    dev = _device()
    _apply_modes(args)
    paths = _paths(args)
    out = paths["test_result_path"]
    os.makedirs(out, exist_ok=True)
    G = build_generator(args, dev)
    ck_path = os.path.join(paths["model_save_path"], checkpoint_name(args, args.pretrained_model))                     # tester.py:133-146
    ck = torch.load(ck_path, map_location=dev, weights_only=True)
    G.load_state_dict(ck["G_net"])
    print("=========== loaded trained models (epochs: {})! ===========".format(args.pretrained_model))
    scorer = _load_nima(args, dev)
    loader = data.get_test_loader(args.test_img_dir, args.test_img_size, args.val_batch_size, False, args.num_workers, device=dev)
    try:
        res = tester.run_test(G, loader, save_dir=os.path.join(out, "test_results"), tag="{:0>3.2f}".format(args.pretrained_model),
                              metrics=args.is_test_psnr_ssim, nima=scorer, compare_dir=os.path.join(out, "test_compare"))
    finally:
        loader.close()
    if scorer is not None:
        print("====== Avg. NIMA: {:>.4f} ======".format(res["mean_nima"]))
    if args.is_test_psnr_ssim:
        print("====== Avg. PSNR: {:>.4f} dB ======".format(res["mean_psnr"]))
        print("====== Avg. SSIM: {:>.4f}  ======".format(res["mean_ssim"]))
    res = dict(res, checkpoint=ck_path)
    if not args.is_test_psnr_ssim:
        res.pop("psnr"), res.pop("ssim")
    with open(os.path.join(out, "test_metrics.json"), "w") as f:
        json.dump(res, f, indent=1)
    return res


PNG_ENCODER_ENV = "UEGAN_PNG_ENCODER"


def _apply_png_encoder():
    """UEGAN_PNG_ENCODER=device|pillow in the environment selects who encodes every PNG of the run (tester.set_png_encoder); unset: the selection
    stays (default "pillow").  It is not a flag: the flag set is the reference's."""
    name = os.environ.get(PNG_ENCODER_ENV)
    if name is None:
        return
    if name not in tester.PNG_ENCODERS:
        raise ValueError("%s=%r: expected one of %s" % (PNG_ENCODER_ENV, name, ", ".join(tester.PNG_ENCODERS)))
    tester.set_png_encoder(name)


INPUT_DECODER_ENV = "UEGAN_INPUT_DECODER"


def _apply_input_decoder():
    """UEGAN_INPUT_DECODER=host|device in the environment selects who decodes the input files of the run's loaders (data.set_input_decoder: "device"
    decodes baseline JPEG files on the device, bit-exact with Pillow, and leaves every other file to Pillow); unset: the selection stays (default
    "host").  Any other value is refused by name.  It is not a flag: the flag set is the reference's."""
    name = os.environ.get(INPUT_DECODER_ENV)
    if name is None:
        return
    if name not in data.INPUT_DECODERS:
        raise ValueError("%s=%r: expected one of %s" % (INPUT_DECODER_ENV, name, ", ".join(data.INPUT_DECODERS)))
    data.set_input_decoder(name)


DATASET_CACHE_ENV = "UEGAN_DATASET_CACHE"
DATASET_CACHE_GB_ENV = "UEGAN_DATASET_CACHE_GB"


def _apply_dataset_cache():
    """UEGAN_DATASET_CACHE=none|device in the environment selects where the run's train, validation and test loaders keep the decoded files
    (data.set_dataset_cache: "device" keeps every decoded image in device memory from its first touch on and cuts the batches out of the resident
    images), UEGAN_DATASET_CACHE_GB=<positive number> the budget of "device" per loader in GiB (default 16); unset: the selection stays (default
    "none").  Any other value is refused by name, and so is a budget without UEGAN_DATASET_CACHE=device.  They are not flags: the flag set is the
    reference's."""
    name, gb = os.environ.get(DATASET_CACHE_ENV), os.environ.get(DATASET_CACHE_GB_ENV)
    if name is not None and name not in data.DATASET_CACHES:
        raise ValueError("%s=%r: expected one of %s" % (DATASET_CACHE_ENV, name, ", ".join(data.DATASET_CACHES)))
    budget = None
    if gb is not None:
        if name != "device":
            raise ValueError("%s=%r needs %s=device" % (DATASET_CACHE_GB_ENV, gb, DATASET_CACHE_ENV))
        try:
            budget = float(gb)
        except ValueError:
            budget = None
        if budget is None or not (budget > 0 and budget != float("inf")):
            raise ValueError("%s=%r: expected a positive number" % (DATASET_CACHE_GB_ENV, gb))
    if name is not None:
        data.set_dataset_cache(name, budget)


IMAGE_FORMAT_ENV = "UEGAN_IMAGE_FORMAT"
JPEG_QUALITY_ENV = "UEGAN_JPEG_QUALITY"
JPEG_OPTIMIZE_ENV = "UEGAN_JPEG_OPTIMIZE"


def _apply_image_format():
    """UEGAN_IMAGE_FORMAT=png|jpeg in the environment selects the container of every image the run writes (tester.set_image_format),
    UEGAN_JPEG_QUALITY=1..100 the quality of "jpeg" (default 95) and UEGAN_JPEG_OPTIMIZE=0|1 whether its files carry their own Huffman tables
    (default 0); unset: the selection stays (default "png").  Any other value is refused by name, and so is a quality or an optimize=1 without
    UEGAN_IMAGE_FORMAT=jpeg.  They are not flags: the flag set is the reference's."""
    name, quality, optimize = os.environ.get(IMAGE_FORMAT_ENV), os.environ.get(JPEG_QUALITY_ENV), os.environ.get(JPEG_OPTIMIZE_ENV)
    if name is not None and name not in tester.IMAGE_FORMATS:
        raise ValueError("%s=%r: expected one of %s" % (IMAGE_FORMAT_ENV, name, ", ".join(tester.IMAGE_FORMATS)))
    if quality is not None:
        if name != "jpeg":
            raise ValueError("%s=%r needs %s=jpeg" % (JPEG_QUALITY_ENV, quality, IMAGE_FORMAT_ENV))
        if not (quality.isascii() and quality.isdigit() and 1 <= int(quality) <= 100):
            raise ValueError("%s=%r: expected an integer in [1, 100]" % (JPEG_QUALITY_ENV, quality))
    if optimize is not None:
        if optimize not in ("0", "1"):
            raise ValueError("%s=%r: expected 0 or 1" % (JPEG_OPTIMIZE_ENV, optimize))
        if optimize == "1" and name != "jpeg":
            raise ValueError("%s=%r needs %s=jpeg" % (JPEG_OPTIMIZE_ENV, optimize, IMAGE_FORMAT_ENV))
    if name == "jpeg":
        tester.set_image_format("jpeg", quality=int(quality) if quality is not None else 95, optimize=optimize == "1")
    elif name == "png":
        tester.set_image_format("png")


def main(argv=None):
    _apply_png_encoder()
    _apply_image_format()
    _apply_input_decoder()
    _apply_dataset_cache()
    args = argv if hasattr(argv, "mode") else config.get_config(argv)
    if args.mode not in ("train", "test"):
        raise NotImplementedError("Mode [{}] is not found".format(args.mode))                                          # main.py:50
    config.validate(args)
    setup_seed(args.seed)
    return train(args) if args.mode == "train" else test(args)
