"""Resampling, pooling, InstanceNorm and its moments, the attention hub, and the element-wise nodes."""
import torch

from .. import _lib as L
from .conv import StatsHolder, _wgrad_done, _wgrad_target, raw_conv_fwd, refuse_stale_pack
from .core import ACT_NONE, IN_EPS, _chk, _dt, _p, _sink_of, _stream, lib, workspace


class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, H, W, Cc = x.shape
        y = torch.empty((B, 2 * H, 2 * W, Cc), dtype=x.dtype, device=x.device)
        _chk(x)
        L.check(lib().uegan_upsample2x_fwd(_dt(x), _p(x), _p(y), B, H, W, Cc, _stream()))
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, H2, W2, Cc = g.shape
        gx = torch.empty((B, H2 // 2, W2 // 2, Cc), dtype=g.dtype, device=g.device)
        L.check(lib().uegan_upsample2x_bwd(_dt(g), _p(g), _p(gx), B, H2 // 2, W2 // 2, Cc, _stream()))
        return gx


class _MaxPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, in_act):
        ctx.in_act = in_act
        x = x.contiguous()
        B, H, W, Cc = x.shape
        y = torch.empty((B, H // 2, W // 2, Cc), dtype=x.dtype, device=x.device)
        _chk(x)
        L.check(lib().uegan_maxpool2x2_fwd(_dt(x), _p(x), _p(y), B, H, W, Cc, _stream()))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        B, H, W, Cc = x.shape
        gx = torch.empty_like(x)
        L.check(lib().uegan_maxpool2x2_bwd_act(_dt(x), ctx.in_act, _p(x), _p(g), _p(gx), B, H, W, Cc, _stream()))
        return gx, None


def _instnorm_into(x, y, pre):
    """y = InstanceNorm(x) -> the [2, B, C] (mean, rstd) used: `pre` where the producing convolution delivered it (one pass), else computed here"""
    B, H, W, Cc = x.shape
    if pre is not None:
        L.check(lib().uegan_instnorm_apply(_dt(x), _p(x), _p(y), _p(pre[0]), _p(pre[1]), B, H * W, Cc, _stream()))
        return pre
    stats = torch.empty((2, B, Cc), dtype=torch.float32, device=x.device)
    tmp = torch.empty((lib().uegan_reduce_workspace_floats(B, H * W, Cc),), dtype=torch.float32, device=x.device)
    L.check(lib().uegan_instnorm_fwd(_dt(x), _p(x), _p(y), _p(stats[0]), _p(stats[1]), _p(tmp), B, H * W, Cc, IN_EPS, _stream()))
    return stats


class _InstNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pre=None, x_lo=None, lo_out=None):
        """pre: [2, B, C] (mean, rstd) of x already known (StatsHolder.value): only the normalising pass runs.  x_lo (with pre): x is a hi + lo pair,
        and so is the result -- its lo plane goes into the one-element list lo_out"""
        x = x.contiguous()
        B, H, W, Cc = x.shape
        y = torch.empty_like(x)
        _chk(x, x_lo)
        if x_lo is not None:
            if pre is None:
                raise RuntimeError("instnorm of a hi + lo pair needs the moments from the producing convolution")
            stats = pre
            ylo = torch.empty_like(x)
            L.check(lib().uegan_instnorm_apply_pair(_dt(x), _p(x), _p(x_lo), _p(y), _p(ylo), _p(stats[0]), _p(stats[1]), B, H * W, Cc, _stream()))
            lo_out.append(ylo)
        else:
            stats = _instnorm_into(x, y, pre)
        ctx.save_for_backward(y, stats)
        return y

    @staticmethod
    def backward(ctx, g):
        y, stats = ctx.saved_tensors
        g = g.contiguous()
        B, H, W, Cc = y.shape
        dx = torch.empty_like(y)
        tmp = torch.empty((lib().uegan_reduce_workspace_floats(B, H * W, Cc),), dtype=torch.float32, device=y.device)
        L.check(lib().uegan_instnorm_bwd(_dt(y), _p(g), _p(y), _p(stats[1]), _p(dx), _p(tmp), B, H * W, Cc, _stream()))
        return dx, None, None, None


def gam_bwd_ws_bytes(dtype, B, HW, Cc, x_act):
    """workspace of the one-pass attention backward (uegan_gam_bwd) for an encoder activation [B, HW, Cc] in `dtype` that act `x_act` produced; 0: the
    library declines (fp32 storage, C other than 32 / 64, the UEGAN_TUNE_GAM_BWD knob off) and the caller keeps the separate passes"""
    if dtype == torch.float32:
        return 0
    return lib().uegan_gam_bwd_ws_bytes(1, B, HW, Cc, x_act)


class _GamHub(torch.autograd.Function):
    """An encoder activation x and its attention module y = IN(W[:, :C] x) (models.GAM) as ONE node: forward -> (x once per remaining consumer ..., y);
    backward receives all of their gradients in one call and issues uegan_gam_bwd, which returns the gradient of the encoder convolution's
    PRE-activation (x's activation backward included: that convolution runs with premasked=True) and the module's weight gradient."""

    @staticmethod
    def forward(ctx, x, weight, cfg, x_act, n_x, wsb):
        x = x.contiguous()
        holder = StatsHolder()
        z, d, ihwo = raw_conv_fwd(x, None, weight, None, cfg, stats=holder)
        y = torch.empty_like(z)
        stats = _instnorm_into(z, y, holder.value)
        ctx.cfg, ctx.d, ctx.ihwo, ctx.pack_version = cfg, d, ihwo, cfg.packed.version
        ctx.x_act, ctx.wsb, ctx.wsink = x_act, wsb, _sink_of(weight)
        ctx.save_for_backward(x, y, stats, weight)
        return tuple(x.view_as(x) for _ in range(n_x)) + (y,)

    @staticmethod
    def backward(ctx, *gs):
        x, y, stats, weight = ctx.saved_tensors
        cfg, d = ctx.cfg, ctx.d
        gy = gs[-1]
        adds = [g.contiguous() for g in gs[:-1] if g is not None]
        if gy is None or len(adds) > 2:
            raise RuntimeError("gam_hub backward: the attention output's gradient and at most two further gradients of x expected")
        refuse_stale_pack(cfg.packed, ctx.ihwo, ctx.pack_version,
                          "gam_hub backward: the module's weight was updated by an optimizer step after this forward; run backward() before step()")
        gy = gy.contiguous()
        _chk(gy, *adds)
        B, H, W, Cc = x.shape
        dz_enc = torch.empty_like(x)
        ws = workspace(ctx.wsb, x.device)
        sink, dw, _, acc = _wgrad_target(ctx.wsink, None, False, ctx.needs_input_grad[1], None, weight, cfg.cin_used, 0, x.device)
        L.check(lib().uegan_gam_bwd(_dt(x), _p(gy), _p(y), _p(x), _p(stats[1]), _p(ctx.ihwo), _p(adds[0]) if adds else None,
                                    _p(adds[1]) if len(adds) > 1 else None, ctx.x_act, _p(dz_enc), _p(dw), d.Cin_total, d.Cin_w, 1 if acc else 0,
                                    _p(ws), ctx.wsb, B, H * W, Cc, _stream()))
        dw, _ = _wgrad_done(sink, ctx.wsink, None, False, dw, None)
        return dz_enc, dw, None, None, None, None


def gam_hub(x, weight, cfg, x_act, n_x, wsb):
    """-> (x, ... n_x aliases ..., IN(conv1x1(x))): see _GamHub; wsb: gam_bwd_ws_bytes(x, x_act), non-zero"""
    return _GamHub.apply(x, weight, cfg, x_act, n_x, wsb)


class _Mul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, act_a, act_b, given=None):
        """given: the product, already formed by the epilogue of the convolution that produced `a` (ConvExtras.prod): no kernel runs here"""
        ctx.acts = (act_a, act_b)
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        if given is not None:
            y = given.view_as(given)
        else:
            y = torch.empty_like(a)
            L.check(lib().uegan_mul_fwd(_dt(a), _p(a), _p(b), _p(y), a.numel(), _stream()))
        ctx.save_for_backward(a, b)
        return y

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da, db = torch.empty_like(a), torch.empty_like(b)
        L.check(lib().uegan_mul_bwd_act(_dt(a), ctx.acts[0], ctx.acts[1], _p(g), _p(a), _p(b), _p(da), _p(db), a.numel(), _stream()))
        return da, db, None, None, None


class _ResidualClamp(torch.autograd.Function):
    """out(NCHW fp32) = clamp(res(NHWC) + x(NCHW fp32), -1, 1)   models.py:72"""

    @staticmethod
    def forward(ctx, res, x, res_act=ACT_NONE, given=None):
        """given: (out,) already written by the epilogue of the convolution that produced res (ConvExtras.res_out): no kernel runs here"""
        ctx.res_act = res_act
        res, x = res.contiguous(), x.contiguous()
        B, H, W, Cp = res.shape
        Cc = x.shape[1]
        _chk(res, x)
        if given is not None:
            out = given[0].view_as(given[0])
        else:
            out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=res.device)
            L.check(lib().uegan_residual_clamp_fwd(_dt(res), _p(res), _p(x), _p(out), B, Cc, Cp, H, W, _stream()))
        ctx.save_for_backward(res, x)
        return out

    @staticmethod
    def backward(ctx, g):
        res, x = ctx.saved_tensors
        g = g.contiguous()
        B, H, W, Cp = res.shape
        Cc = x.shape[1]
        dres = torch.empty_like(res)
        dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        L.check(lib().uegan_residual_clamp_bwd_act(_dt(res), ctx.res_act, _p(g), _p(res), _p(x), _p(dres), _p(dx), B, Cc, Cp, H, W, _stream()))
        return dres, dx, None, None


class _ResidualClampPair(torch.autograd.Function):
    """models.py:72 for a generator pass over two image sets at once: res [Ba + Bb, H, W, Cp] -> clamp(res[:Ba] + xa), clamp(res[Ba:] + xb)
    as two separate NCHW fp32 tensors (each is consumed by its own losses)"""

    @staticmethod
    def forward(ctx, res, xa, xb, res_act=ACT_NONE, given=None):
        """given: (oa, ob) already written by dec5.1's epilogue (ConvExtras.res_out)"""
        ctx.res_act = res_act
        res, xa, xb = res.contiguous(), xa.contiguous(), xb.contiguous()
        Bt, H, W, Cp = res.shape
        Ba, Cc = xa.shape[0], xa.shape[1]
        _chk(res, xa, xb)
        if given is not None:
            oa, ob = given[0].view_as(given[0]), given[1].view_as(given[1])
        else:
            oa = torch.empty_like(xa)
            ob = torch.empty_like(xb)
            st = _stream()
            L.check(lib().uegan_residual_clamp_fwd(_dt(res), _p(res), _p(xa), _p(oa), Ba, Cc, Cp, H, W, st))
            L.check(lib().uegan_residual_clamp_fwd(_dt(res), _p(res[Ba:]), _p(xb), _p(ob), Bt - Ba, Cc, Cp, H, W, st))
        ctx.save_for_backward(res, xa, xb)
        return oa, ob

    @staticmethod
    def backward(ctx, ga, gb):
        res, xa, xb = ctx.saved_tensors
        Bt, H, W, Cp = res.shape
        Ba, Cc = xa.shape[0], xa.shape[1]
        dres = torch.empty_like(res)
        st = _stream()
        dxa = dxb = None
        for g, x, r, dr, nb, idx in ((ga, xa, res, dres, Ba, 1), (gb, xb, res[Ba:], dres[Ba:], Bt - Ba, 2)):
            if g is None:
                dr.zero_()             # this output was not used by any loss
                continue
            g = g.contiguous()
            dx = torch.empty_like(x) if ctx.needs_input_grad[idx] else None
            L.check(lib().uegan_residual_clamp_bwd_act(_dt(res), ctx.res_act, _p(g), _p(r), _p(x), _p(dr), _p(dx), nb, Cc, Cp, H, W, st))
            if idx == 1:
                dxa = dx
            else:
                dxb = dx
        return dres, dxa, dxb, None, None


def residual_clamp_pair(res, xa, xb, res_act=ACT_NONE, given=None):
    return _ResidualClampPair.apply(res, xa, xb, res_act, given)


def upsample2x(x, at=None):
    """at=(oy, ox, GH, GW): x is the tile at origin (oy, ox) of a global GH x GW map -> the matching window of the GLOBAL x2 result
    (uegan_upsample2x_fwd_at: the align_corners sampling phase is the whole map's).  Forward only: raises while gradients are enabled."""
    if at is None:
        return _Upsample2x.apply(x)
    if torch.is_grad_enabled():
        raise RuntimeError("upsample2x(at=) is an inference kernel without a backward: call it under torch.no_grad()")
    oy, ox, GH, GW = (int(v) for v in at)
    x = x.contiguous()
    B, H, W, Cc = x.shape
    if not (0 <= oy and 0 <= ox and oy + H <= GH and ox + W <= GW):
        raise ValueError("upsample2x: the %d x %d tile at (%d, %d) does not lie inside its %d x %d map" % (H, W, oy, ox, GH, GW))
    y = torch.empty((B, 2 * H, 2 * W, Cc), dtype=x.dtype, device=x.device)
    _chk(x)
    L.check(lib().uegan_upsample2x_fwd_at(_dt(x), _p(x), _p(y), B, H, W, Cc, oy, ox, GH, GW, _stream()))
    return y


def moments_acc_new(B, Cc, device):
    """zeroed accumulators for moments_window_acc: float64 [2, B, C] (sum z, sum z^2)"""
    return torch.zeros((2, B, Cc), dtype=torch.float64, device=device)


def moments_window_acc(x, window, acc, x_lo=None):
    """acc (moments_acc_new) += (sum z, sum z^2) over rows [y0, y1) x columns [x0, x1) of the NHWC map x, read in place; x_lo: z is the pair
    x + x_lo.  Deterministic: the same windows in the same order give the same bits (uegan_moments_window_acc)."""
    y0, y1, x0, x1 = (int(v) for v in window)
    B, H, W, Cc = x.shape
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError("moments_window_acc: rows [%d, %d) x columns [%d, %d) is no window of a %d x %d map" % (y0, y1, x0, x1, H, W))
    if acc.dtype != torch.float64 or tuple(acc.shape) != (2, B, Cc) or (x_lo is not None and (x_lo.shape != x.shape or x_lo.dtype != x.dtype)):
        raise ValueError("moments_window_acc: float64 [2, B, C] accumulators and a lo plane of x's shape expected")
    _chk(x, x_lo, acc)
    tmp = torch.empty((lib().uegan_moments_window_workspace_bytes(B, Cc) // 8,), dtype=torch.float64, device=x.device)
    L.check(lib().uegan_moments_window_acc(_dt(x), _p(x), _p(x_lo), B, H, W, Cc, y0, y1, x0, x1, _p(acc[0]), _p(acc[1]), _p(tmp), _stream()))
    return acc


def moments_finish(acc, count, eps=IN_EPS):
    """accumulators over `count` pixels per (image, channel) -> fp32 [2, B, C] (mean, rstd): the layout of StatsHolder.value and instnorm(pre=);
    biased variance (uegan_moments_finish; eps < 0: the variance itself in place of rstd)"""
    _chk(acc)
    _, B, Cc = acc.shape
    out = torch.empty((2, B, Cc), dtype=torch.float32, device=acc.device)
    L.check(lib().uegan_moments_finish(_p(acc[0]), _p(acc[1]), float(count), float(eps), _p(out[0]), _p(out[1]), B * Cc, _stream()))
    return out


def maxpool2x2(x, in_act=ACT_NONE):
    """in_act: the activation whose (deferred) gradient the pool's backward applies for x's producer (see ConvCfg)."""
    return _MaxPool2x2.apply(x, in_act)


def instnorm(x, pre=None):
    return _InstNorm.apply(x, pre)


def instnorm_pair(x, x_lo, pre):
    """InstanceNorm of the pair (x, x_lo) with its moments `pre` -> (y, y_lo); y_lo is a plain tensor outside the graph (the backward reads y)"""
    lo = []
    y = _InstNorm.apply(x, pre, x_lo, lo)
    return y, lo[0]


def mul(a, b, act_a=ACT_NONE, act_b=ACT_NONE, given=None):
    """act_a / act_b: the activation whose (deferred) gradient the backward applies for a's / b's producer (see ConvCfg); given: see _Mul"""
    return _Mul.apply(a, b, act_a, act_b, given)


def residual_clamp(res, x, res_act=ACT_NONE, given=None):
    """res_act: the activation that produced res, its gradient deferred to this op's backward (see ConvCfg); given: see _ResidualClamp"""
    return _ResidualClamp.apply(res, x, res_act, given)


def raw_act_bwd(g, y, act):
    dz = torch.empty_like(g)
    L.check(lib().uegan_act_bwd(_dt(g), act, _p(g), _p(y), _p(dz), g.numel(), _stream()))
    return dz


def zero_(t):
    """t.zero_() as a stream memset (uegan_fill_zero)"""
    _chk(t)
    L.check(lib().uegan_fill_zero(_p(t), t.numel() * t.element_size(), _stream()))
    return t
