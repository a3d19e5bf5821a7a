"""uegan_amd: MI355X-native (gfx950 HIP) implementation of the UEGAN training / inference hot path.

Drop-in mirror of the reference's `models.py` / `losses.py` class API (`uegan_amd.models`, `uegan_amd.losses`) plus
the step driver (`uegan_amd.trainer`), inference helper (`uegan_amd.tester`) and the train / test command line
(`python -m uegan_amd`: `uegan_amd.runner`, flags in `uegan_amd.config`).  All device arithmetic lives in
libuegan_hip.so (uegan_amd/csrc, C ABI in include/uegan_hip.h); there is no CPU fallback.
"""
from . import _lib  # noqa: F401
from .ops import set_compute_dtype, get_compute_dtype, invalidate_weight_caches, set_precise, precise  # noqa: F401
from . import models, losses, trainer, tester  # noqa: F401
from .tester import set_png_encoder, get_png_encoder, set_image_format, get_image_format, get_jpeg_optimize  # noqa: F401
from .data import set_input_decoder, get_input_decoder, set_dataset_cache, get_dataset_cache  # noqa: F401
from . import config, runner  # noqa: F401
from .models import Generator, Discriminator  # noqa: F401
from .losses import PerceptualLoss, GANLoss, MultiscaleRecLoss, TVLoss  # noqa: F401

__all__ = ["Generator", "Discriminator", "PerceptualLoss", "GANLoss", "MultiscaleRecLoss", "TVLoss", "set_compute_dtype",
           "get_compute_dtype", "invalidate_weight_caches", "set_precise", "precise", "set_png_encoder", "get_png_encoder", "set_image_format", "get_image_format", "get_jpeg_optimize", "set_input_decoder", "get_input_decoder", "set_dataset_cache", "get_dataset_cache", "models", "losses", "trainer", "tester", "config", "runner"]
