"""Loss nodes: relativistic-average hinge, multi-scale reconstruction, the perceptual taps loss, and the weighted sum of device scalars."""
import ctypes as C

import torch

from .. import _lib as L
from .core import ACT_NONE, IN_EPS, _chk, _dt, _p, _ptr_table, _stream, lib


class _RaHinge(torch.autograd.Function):
    """GANLoss('rahinge') over lists of prediction maps (losses.py:348-362, 393-409); returns shape [1]."""

    @staticmethod
    def forward(ctx, for_discriminator, nscales, *maps):
        reals = [m.contiguous() for m in maps[:nscales]]
        fakes = [m.contiguous() for m in maps[nscales:]]
        for r, f in zip(reals, fakes):
            if r.dtype != torch.float32 or f.dtype != torch.float32 or r.numel() != f.numel():
                raise RuntimeError("rahinge: maps must be float32 with matching sizes")
        dev = reals[0].device
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        tmp = torch.empty((lib().uegan_rahinge_workspace_floats(nscales),), dtype=torch.float32, device=dev)
        n = (C.c_int64 * nscales)(*[r.numel() for r in reals])
        _chk(*reals, *fakes)
        L.check(lib().uegan_rahinge_fwd(nscales, _ptr_table(reals), _ptr_table(fakes), n, 1 if for_discriminator else 0, _p(loss), _p(tmp),
                                        _stream()))
        ctx.for_d, ctx.nscales = for_discriminator, nscales
        ctx.save_for_backward(tmp, *reals, *fakes)
        return loss

    @staticmethod
    def backward(ctx, g):
        tmp = ctx.saved_tensors[0]
        ns = ctx.nscales
        reals, fakes = ctx.saved_tensors[1:1 + ns], ctx.saved_tensors[1 + ns:]
        g = g.contiguous().float()
        greal = [torch.empty_like(r) if ctx.needs_input_grad[2 + i] else None for i, r in enumerate(reals)]
        gfake = [torch.empty_like(f) if ctx.needs_input_grad[2 + ns + i] else None for i, f in enumerate(fakes)]
        n = (C.c_int64 * ns)(*[r.numel() for r in reals])
        L.check(lib().uegan_rahinge_bwd(ns, _ptr_table(reals), _ptr_table(fakes), n, 1 if ctx.for_d else 0, _p(tmp), _p(g), _ptr_table(greal),
                                        _ptr_table(gfake), _stream()))
        return (None, None) + tuple(greal) + tuple(gfake)


def rahinge(real_preds, fake_preds, for_discriminator):
    return _RaHinge.apply(bool(for_discriminator), len(real_preds), *real_preds, *fake_preds)


REC_KINDS = {"l1": 0, "smoothl1": 1, "l2": 2}


class _MsRec(torch.autograd.Function):
    """MultiscaleRecLoss.forward (losses.py:219-231): criterion `kind` at `nscales` scales, AvgPool2d(2,2) between, weights 2^-i."""

    @staticmethod
    def forward(ctx, pred, gt, kind, nscales):
        pred, gt = pred.contiguous(), gt.contiguous()
        if pred.dtype != torch.float32 or gt.dtype != torch.float32 or pred.shape != gt.shape:
            raise RuntimeError("multiscale reconstruction loss: float32 NCHW tensors of equal shape expected")
        B, Cc, H, W = pred.shape
        loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
        scratch = torch.empty((lib().uegan_msrec_scratch_floats(),), dtype=torch.float32, device=pred.device)
        _chk(pred, gt)
        L.check(lib().uegan_msrec_fwd(_p(pred), _p(gt), _p(loss), _p(scratch), B, Cc, H, W, kind, nscales, _stream()))
        ctx.save_for_backward(pred, gt)
        ctx.kind, ctx.nscales = kind, nscales
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        g = g.contiguous().float().reshape(1)
        B, Cc, H, W = pred.shape
        gp = torch.empty_like(pred)
        L.check(lib().uegan_msrec_bwd(_p(pred), _p(gt), _p(g), _p(gp), B, Cc, H, W, ctx.kind, ctx.nscales, _stream()))
        return gp, None, None, None


def multiscale_rec(pred, gt, kind="l1", nscales=3):
    return _MsRec.apply(pred, gt, REC_KINDS[kind], int(nscales))


def multiscale_l1(pred, gt):
    return multiscale_rec(pred, gt, "l1", 3)


class _Percep(torch.autograd.Function):
    """sum_t w_t * MSE(IN(x_t), IN(y_t)) over VGG taps (losses.py:30-34). Gradient flows to the x taps only."""

    @staticmethod
    def forward(ctx, weights_act, ntaps, *taps):
        weights, ctx.in_act = weights_act
        xs = [t.contiguous() for t in taps[:ntaps]]
        ys = [t.contiguous() for t in taps[ntaps:]]
        dev = xs[0].device
        loss = torch.zeros((1,), dtype=torch.float32, device=dev)
        tmps = []
        st = _stream()
        _chk(*xs, *ys)
        for w, x, y in zip(weights, xs, ys):
            B, H, W, Cc = x.shape
            tmp = torch.empty((3 * lib().uegan_reduce_workspace_floats(B, H * W, Cc),), dtype=torch.float32, device=dev)
            L.check(lib().uegan_percep_tap_fwd(_dt(x), _p(x), _p(y), float(w), _p(loss), _p(tmp), B, H * W, Cc, IN_EPS, st))
            tmps.append(tmp)
        ctx.weights, ctx.ntaps = weights, ntaps
        ctx.save_for_backward(*xs, *ys, *tmps)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        nt = ctx.ntaps
        sv = ctx.saved_tensors
        xs, ys, tmps = sv[:nt], sv[nt:2 * nt], sv[2 * nt:]
        g = g.contiguous().float().reshape(1)
        st = _stream()
        grads = []
        for i, (w, x, y, tmp) in enumerate(zip(ctx.weights, xs, ys, tmps)):
            if not ctx.needs_input_grad[2 + i]:
                grads.append(None)
                continue
            B, H, W, Cc = x.shape
            gx = torch.empty_like(x)
            L.check(lib().uegan_percep_tap_bwd_act(_dt(x), ctx.in_act, _p(x), _p(y), float(w), _p(g), _p(gx), _p(tmp), B, H * W, Cc, IN_EPS, st))
            grads.append(gx)
        return (None, None) + tuple(grads) + (None,) * nt


def perceptual_taps_loss(x_taps, y_taps, weights, in_act=ACT_NONE):
    """in_act: the x taps' producers deferred their activation gradient to their consumers (see ConvCfg); applied here."""
    return _Percep.apply((tuple(weights), in_act), len(x_taps), *x_taps, *y_taps)


def gather_scalars(terms):
    """[n] fp32 device vector of n <= 8 device scalars (uegan_gather_scalars): the step's logged losses in ONE buffer, so that reading them
    back is one copy and one host sync instead of five (trainer.py:98-119 calls .item() five times)"""
    ts = [t.detach().contiguous().float().reshape(-1)[:1] for t in terms]
    out = torch.empty((len(ts),), dtype=torch.float32, device=ts[0].device)
    _chk(*ts)
    L.check(lib().uegan_gather_scalars(len(ts), _ptr_table(ts), _p(out), _stream()))
    return out


class _LossSum(torch.autograd.Function):
    """total = sum_i w_i * t_i over device scalars, left to right (trainer.py:104-115); also hands back the scaled terms for logging"""

    @staticmethod
    def forward(ctx, weights, *terms):
        ts = [t.contiguous().float().reshape(1) for t in terms]
        n = len(ts)
        dev = ts[0].device
        total = torch.empty((1,), dtype=torch.float32, device=dev)
        scaled = torch.empty((n,), dtype=torch.float32, device=dev)
        _chk(*ts)
        L.check(lib().uegan_scalar_wsum(n, _ptr_table(ts), (C.c_float * n)(*weights), _p(total), _p(scaled), _stream()))
        ctx.weights, ctx.shapes = weights, [t.shape for t in terms]
        ctx.mark_non_differentiable(scaled)
        return total, scaled

    @staticmethod
    def backward(ctx, g, _gs):
        n = len(ctx.weights)
        g = g.contiguous().float().reshape(1)
        gout = torch.empty((n,), dtype=torch.float32, device=g.device)
        L.check(lib().uegan_scalar_wsum_bwd(n, (C.c_float * n)(*ctx.weights), _p(g), _p(gout), _stream()))
        return (None,) + tuple(gout[i].reshape(s) for i, s in enumerate(ctx.shapes))


def loss_sum(terms, weights):
    """(sum_i w_i * t_i as a [1] tensor, the n scaled terms as a detached [n] tensor) for device-scalar losses"""
    return _LossSum.apply(tuple(float(w) for w in weights), *terms)
