"""Process-wide state and the small helpers every op module shares: the compute dtype, the precise mode, weight epochs, gradient sinks,
and the ctypes plumbing (pointers, dtype codes, the stream, the library handle, workspaces)."""
import ctypes as C

import torch

from .. import _lib as L


ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
PAD_ZERO, PAD_REFLECT = 0, 1
IN_EPS = 1e-5
SN_EPS = 1e-12

_compute_dtype = [torch.float32]      # (one-element lists: a rebound value reaches every module that holds the list)
_weight_epoch = [0]


def set_compute_dtype(dt):
    """Storage dtype of activations / packed weights inside G, D and VGG: torch.float32 (parity mode), torch.bfloat16 (throughput mode;
    fp32 accumulation, fp32 master weights / statistics / losses) or torch.float16 (the same bytes and MFMA rate with 11 instead of 8
    significant bits: libuegan_hip_f16.so, the same kernel sources with fp16 as the 16-bit storage format -- what the generator's O(1)
    activations want; training in it needs Trainer(loss_scale=...): fp16's exponent range does not hold raw gradients).
    Process-wide; do not switch between a forward and its backward."""
    if dt not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("compute dtype must be float32, bfloat16 or float16")
    if dt != torch.float32:
        L.use_half_format("fp16" if dt == torch.float16 else "bf16")
    _compute_dtype[0] = dt      # (the packed-weight caches are keyed on the dtype: nothing to invalidate)


def get_compute_dtype():
    return _compute_dtype[0]


_precise = [False]


def set_precise(flag):
    """`precise` mode of the 16-bit storage dtypes (meant for torch.float16): the generator's full-resolution tensors (the image, x1, the attention
    branch ga1, y4 * x1, dec5.0's result) travel as hi + lo PAIRS of 16-bit planes and the weights of the five thin layers as pairs too, the residual
    + clamp is formed from dec5.1's fp32 result (uegan_conv2d_fwd_ex) -- the enhanced pixels then sit inside north_star's 1e-3 of the fp32 reference
    (the backward pass is unchanged: it reads the hi planes).  No effect in float32 mode.  Process-wide."""
    _precise[0] = bool(flag)


# the generator's product (models.py:69) and residual + clamp (models.py:70-72) formed by the epilogues of dec4 / dec5.1 in the plain 16-bit modes
# (uegan_conv2d_fwd_ex); False: the separate elementwise kernels of round 5 (A/B: bench.py --no-fuse-epilogues).  The precise mode always fuses.
fuse_epilogues = [True]


def precise():
    """is the precise mode in force for the current compute dtype?"""
    return _precise[0] and _compute_dtype[0] != torch.float32


def invalidate_weight_caches(params=None):
    """Call after weights were modified behind autograd's back (`.data` edits, in-place kernels): the packed bf16/fp32 copies the
    conv kernels read are re-made on next use.  With `params` only those tensors' copies are invalidated (what FusedAdamL2.step
    does for the tensors it updated -- the frozen VGG19 and the other network keep theirs); without, every cache in the process."""
    if params is None:
        _weight_epoch[0] += 1
    else:
        for p in params:
            p._uegan_epoch = getattr(p, "_uegan_epoch", 0) + 1


class GradSink:
    """Where a parameter's gradient lives inside an optimizer's flat fp32 bucket (FusedAdamL2): the weight-gradient kernels write
    (first touch after zero_grad) or accumulate (later touches) there directly and hand autograd `None`, so there is no
    per-parameter `grad += dw` kernel and no temporary."""
    __slots__ = ("view", "dirty", "owner", "index")

    def __init__(self, view):
        self.view, self.dirty = view, False
        self.owner, self.index = None, -1        # trainer.GradBucket: told when this parameter's gradient has been written

    def mark(self):
        """the gradient (or its first contribution) is in the bucket"""
        first = not self.dirty
        self.dirty = True
        if self.owner is not None:
            if first:
                self.owner.notify(self.index)
            else:
                self.owner.touched_again(self.index)      # (raises if this parameter's all-reduce chunk is already in flight)


def _sink_of(p):
    if p is None or not p.requires_grad:
        return None
    s = getattr(p, "_uegan_sink", None)
    if s is None or p.grad is None or p.grad.data_ptr() != s.view.data_ptr():
        return None
    return s


def _dt(t):
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16 or t.dtype == torch.float16:      # code 1 = "the 16-bit storage format" of the loaded build
        if (t.dtype == torch.float16) != (L.half_format() == "fp16"):
            raise TypeError("a %s tensor reached the %s build of the kernel library (uegan_amd.set_compute_dtype selects it)"
                            % (t.dtype, L.half_format()))
        return 1
    raise TypeError("unsupported dtype %s" % t.dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    if L.is_emulated():
        return None
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    emu = L.is_emulated()
    for t in ts:
        if t is None:
            continue
        if not emu and not t.is_cuda:
            raise RuntimeError("uegan_amd ops need CUDA/HIP tensors (there is no CPU path)")
        if not t.is_contiguous():
            raise RuntimeError("uegan_amd internal error: non-contiguous tensor reached a kernel")


def lib():
    return L.load()


def chunk_elems(dtype):
    """elements per 16-byte chunk: every NHWC tensor the kernels see has a channel count that is a multiple of this"""
    return 8 if dtype in (torch.bfloat16, torch.float16) else 4


def cpad(c, dtype):
    e = chunk_elems(dtype)
    return (c + e - 1) // e * e


def _farr(vals):
    return None if vals is None else (C.c_float * len(vals))(*[float(v) for v in vals])


def _ptr_table(ts):
    return (C.c_void_p * len(ts))(*[_p(t) for t in ts])


def workspace(nbytes, device, least=0):
    """an fp32 scratch tensor of at least max(nbytes, least) bytes for a kernel's workspace argument; None when that is 0"""
    n = (max(nbytes, least) + 3) // 4
    return torch.empty((n,), dtype=torch.float32, device=device) if n else None
