"""The layout boundary: module inputs and outputs are NCHW fp32 (data_loader.py:79-81), everything between is NHWC in the compute dtype."""
import ctypes as C

import torch

from .. import _lib as L
from .core import _chk, _compute_dtype, _dt, _farr, _p, _stream, cpad, lib


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype, a, b, pair=False):
        x = x.contiguous()
        if x.dtype != torch.float32:
            raise TypeError("module inputs must be float32 NCHW (data_loader.py:79-81)")
        B, Cc, H, W = x.shape
        Cp = cpad(Cc, dtype)                      # zero-padded to one 16-byte chunk (3 -> 8 bf16 / 4 fp32)
        y = torch.empty((B, H, W, Cp), dtype=dtype, device=x.device)
        _chk(x, y)
        fn = lib().uegan_nchw_to_nhwc_pair if pair else lib().uegan_nchw_to_nhwc      # (pair: the image's lo plane in its own spare channels)
        L.check(fn(_dt(y), _p(x), _p(y), B, Cc, Cp, H, W, _farr(a), _farr(b), _stream()))
        ctx.a, ctx.C = a, Cc
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, H, W, Cp = g.shape
        gx = torch.empty((B, ctx.C, H, W), dtype=torch.float32, device=g.device)
        L.check(lib().uegan_nhwc_to_nchw(_dt(g), _p(g), _p(gx), B, ctx.C, Cp, H, W, _farr(ctx.a), _stream()))
        return gx, None, None, None, None


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, channels):
        x = x.contiguous()
        B, H, W, Cp = x.shape
        Cc = Cp if channels is None else channels
        y = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
        _chk(x, y)
        L.check(lib().uegan_nhwc_to_nchw(_dt(x), _p(x), _p(y), B, Cc, Cp, H, W, None, _stream()))
        ctx.dtype, ctx.Cp = x.dtype, Cp
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, Cc, H, W = g.shape
        gx = torch.empty((B, H, W, ctx.Cp), dtype=ctx.dtype, device=g.device)
        L.check(lib().uegan_nchw_to_nhwc(_dt(gx), _p(g), _p(gx), B, Cc, ctx.Cp, H, W, None, None, _stream()))
        return gx, None


class _ToNHWCPair(torch.autograd.Function):
    """two NCHW fp32 batches -> one NHWC tensor [Ba + Bb, H, W, Cp] (a batch concatenation that never exists in NCHW)"""

    @staticmethod
    def forward(ctx, xa, xb, dtype, pair=False):
        y = raw_to_nhwc([xa, xb], dtype, pair=pair)
        ctx.Ba, ctx.C = xa.shape[0], xa.shape[1]
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        ga = raw_to_nchw_grad(g[:ctx.Ba], ctx.C) if ctx.needs_input_grad[0] else None
        gb = raw_to_nchw_grad(g[ctx.Ba:], ctx.C) if ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def to_nhwc(x, dtype=None, a=None, b=None, pair=False):
    """pair: channels [C, 2C) of the padded pixel receive the lo plane of the image (uegan_nchw_to_nhwc_pair; 16-bit dtypes)"""
    return _ToNHWC.apply(x, dtype or _compute_dtype[0], a, b, pair)      # (the list core.set_compute_dtype edits in place)


def to_nhwc_pair(xa, xb, dtype=None, pair=False):
    """two image sets -> one batch-concatenated NHWC tensor (`pair` as in to_nhwc: unrelated to the two sets)"""
    return _ToNHWCPair.apply(xa, xb, dtype or _compute_dtype[0], pair)


def to_nchw(x, channels=None):
    """NHWC (possibly channel-padded) -> NCHW fp32 keeping the first `channels` channels"""
    return _ToNCHW.apply(x, channels)


def raw_to_nhwc(xs, dtype, a=None, b=None, pair=False):
    """several NCHW fp32 image batches of one shape -> ONE NHWC tensor [sum(B_i), H, W, Cp] (batch-concatenated)"""
    xs = [x.detach().contiguous() for x in xs]
    B0, Cc, H, W = xs[0].shape
    for x in xs:
        if x.dtype != torch.float32 or tuple(x.shape[1:]) != (Cc, H, W):
            raise TypeError("module inputs must be float32 NCHW batches of one image shape (data_loader.py:79-81)")
    Cp = cpad(Cc, dtype)
    Bt = sum(x.shape[0] for x in xs)
    y = torch.empty((Bt, H, W, Cp), dtype=dtype, device=xs[0].device)
    _chk(y, *xs)
    off = 0
    fn = lib().uegan_nchw_to_nhwc_pair if pair else lib().uegan_nchw_to_nhwc
    for x in xs:
        L.check(fn(_dt(y), _p(x), _p(y[off:]), x.shape[0], Cc, Cp, H, W, _farr(a), _farr(b), _stream()))
        off += x.shape[0]
    return y


def raw_to_nchw_grad(g_nhwc, channels, a=None):
    """gradient of raw_to_nhwc's conversion for one source: NHWC -> NCHW fp32, times the forward's per-channel scale a"""
    B, H, W, Cp = g_nhwc.shape
    gx = torch.empty((B, channels, H, W), dtype=torch.float32, device=g_nhwc.device)
    L.check(lib().uegan_nhwc_to_nchw(_dt(g_nhwc), _p(g_nhwc), _p(gx), B, channels, Cp, H, W, _farr(a), _stream()))
    return gx


def copy_images(dst, src_a, src_b, dst_idx, src_idx):
    """dst[dst_idx[i]] = src_a[src_idx[i]] if src_idx[i] >= 0 else src_b[~src_idx[i]] (whole images; stacks of contiguous fp32
    images of one shape).  utils.py:41-46 as one gather / one scatter (include/uegan_hip.h uegan_copy_images)."""
    for t in (dst, src_a, src_b):
        if t.dtype != torch.float32 or tuple(t.shape[1:]) != tuple(dst.shape[1:]):
            raise RuntimeError("copy_images: float32 image stacks of one image shape expected")
    _chk(dst, src_a, src_b)
    elems = dst[0].numel()
    n = len(dst_idx)
    for s0 in range(0, n, 64):
        di, si = dst_idx[s0:s0 + 64], src_idx[s0:s0 + 64]
        for d, s in zip(di, si):
            if not (0 <= d < dst.shape[0]) or not (0 <= (s if s >= 0 else ~s) < (src_a if s >= 0 else src_b).shape[0]):
                raise IndexError("copy_images: index out of range")
        L.check(lib().uegan_copy_images(_p(dst), _p(src_a), _p(src_b), (C.c_int32 * len(di))(*di), (C.c_int32 * len(si))(*si), len(di), elems,
                                        _stream()))
