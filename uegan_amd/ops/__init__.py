"""torch.autograd.Function wrappers over the C ABI of libuegan_hip.so, one module per role; this file only gathers their names.

PyTorch is plumbing here: device memory (caching allocator), the current HIP stream and the autograd graph.
Every arithmetic step of the hot path is a hand-written gfx950 kernel reached through ctypes (uegan_amd/_lib.py).
Activations inside the networks are explicit NHWC tensors ([B,H,W,C]) in the compute dtype (fp32 or bf16);
module boundaries keep the reference's NCHW fp32 contract (data_loader.py:79-81).

  core         process-wide state (compute dtype, precise mode, weight epochs), gradient sinks, the ctypes helpers, lib(), workspace()
  layout       the NCHW <-> NHWC boundary
  conv         weight packing, the convolution node, the raw_conv_* launchers
  elementwise  resampling, pooling, InstanceNorm, the attention hub, element-wise nodes
  loss         loss nodes
  optim        FusedAdamL2
(the PNG / JPEG file codecs live in uegan_amd/codecs.py; their names are gathered here too)

Process-wide values that change (split_k, fuse_epilogues, _weight_epoch, the compute dtype) are one-element lists edited in place or are read
through their getter, so a name gathered here is the object its readers use.  lib() resolves _lib.load() at every call: _lib.load is the one
place to watch or replace for "did anything reach the kernel library".
"""
from .. import _lib as L  # noqa: F401
# (codecs imports .ops.core, so it can only be imported once this package has begun to: uegan_amd/__init__.py imports .ops before anything names codecs)
from ..codecs import (JPEG_MAX_SIDE, JPEG_SUBSAMPLINGS, PNG_MAX_BAND, deflate_bands, jpeg_build_tables, jpeg_capacity,  # noqa: F401
                      jpeg_coeffs, jpeg_encode, jpeg_histogram, jpeg_qtables, jpeg_sizes, png_encode,
                      JpegDecodeError, JpegUnsupported, jpeg_decode, jpeg_decode_coeffs, jpeg_decode_into, jpeg_info)
from .conv import (ConvCfg, ConvExtras, PackedWeight, PackTable, SNCall, StatsHolder, _ConvFn, _desc, _sub_desc, conv2d,  # noqa: F401
                   raw_conv_dgrad, raw_conv_fwd, raw_conv_wgrad, refuse_stale_pack, specnorm_sigma, split_k)
from .core import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, IN_EPS, PAD_REFLECT, PAD_ZERO, SN_EPS, GradSink, _chk, _dt, _farr, _p,  # noqa: F401
                   _ptr_table, _sink_of, _stream, _weight_epoch, chunk_elems, cpad, fuse_epilogues, get_compute_dtype,
                   invalidate_weight_caches, lib, precise, set_compute_dtype, set_precise, workspace)
from .elementwise import (gam_bwd_ws_bytes, gam_hub, instnorm, instnorm_pair, maxpool2x2, moments_acc_new, moments_finish,  # noqa: F401
                          moments_window_acc, mul, raw_act_bwd, residual_clamp, residual_clamp_pair, upsample2x, zero_)
from .layout import copy_images, raw_to_nchw_grad, raw_to_nhwc, to_nchw, to_nhwc, to_nhwc_pair  # noqa: F401
from .loss import REC_KINDS, gather_scalars, loss_sum, multiscale_l1, multiscale_rec, perceptual_taps_loss, rahinge  # noqa: F401
from .optim import FusedAdamL2  # noqa: F401
