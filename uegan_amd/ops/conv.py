"""Weight packing and the convolution: the autograd node (conv2d), the graph-free raw_conv_* launchers of uegan_amd/fused.py, and the ONE set
of launch sequences both go through (_fwd, _dgrad, _wgrad, refuse_stale_pack)."""
import ctypes as C
import weakref

import torch

from .. import _lib as L
from .core import (ACT_NONE, IN_EPS, PAD_REFLECT, SN_EPS, _chk, _dt, _p, _sink_of, _stream, _weight_epoch, chunk_elems, cpad,
                   get_compute_dtype, lib, workspace)


class PackedWeight:
    """Cache of the two packed copies (OHWI for forward/wgrad, IHWO for dgrad) of one OIHW fp32 weight."""

    def __init__(self):
        self.key = None
        self.ohwi = None
        self.ihwo = None
        self.ohwi_lo = None       # pair=True: the lo part of the OHWI copy (uegan_pack_weights_pair)
        self.version = 0          # bumped whenever the packed buffers are rewritten IN PLACE (PackTable.repack)

    def get(self, w, dtype, cin_pad, cout_pad, key_src=None, cin_used=None, pair=False, dup=False):
        """cin_used: pack only the first cin_used input channels of w (a column slice of the master weight); pair: also the lo part of the forward copy
        (self.ohwi_lo); dup 1: input channels [Cin, 2 Cin) of the forward copies repeat [0, Cin) (the source carries its own lo plane there), dup 2: they hold
        the LO part of [0, Cin) (the weight pair inside one matrix, for a kernel that reads the source's channels twice: stride-2 forwards)"""
        src = w if key_src is None else key_src
        key = (src.data_ptr(), src._version, _weight_epoch[0], getattr(src, "_uegan_epoch", 0), dtype, tuple(w.shape), str(w.device), cin_pad,
               cout_pad, cin_used, bool(pair), int(dup))
        if key != self.key:
            wd = w.detach()
            if wd.dtype != torch.float32:
                raise TypeError("master weights must be float32")
            wd = wd.contiguous()
            co, ci_total, kh, kw = wd.shape
            ci = ci_total if cin_used is None else cin_used
            kp = lib().uegan_packed_k(kh * kw * cin_pad)
            kp2 = lib().uegan_packed_k(kh * kw * cout_pad)
            self.ohwi = torch.empty((cout_pad, kp), dtype=dtype, device=wd.device)
            self.ihwo = torch.empty((cin_pad, kp2), dtype=dtype, device=wd.device)
            self.ohwi_lo = torch.empty((cout_pad, kp), dtype=dtype, device=wd.device) if pair else None
            _chk(wd)
            L.check(lib().uegan_pack_weights_pair(_dt(self.ohwi), _p(wd), co, ci, ci_total, kh, kw, cout_pad, cin_pad, _p(self.ohwi),
                                                  _p(self.ihwo), _p(self.ohwi_lo), int(dup), _stream()))
            self.key = key
            # remembered on the master tensor: the optimizer that updates it re-packs all of its copies in one launch (repack_all)
            self.args = (wd.data_ptr(), co, ci, ci_total, kh, kw, cout_pad, cin_pad, kp, kp2, _p(self.ohwi_lo) or 0, int(dup))
            self.src = weakref.ref(src)
            packs = getattr(src, "_uegan_packs", None)
            if packs is None:
                packs = src._uegan_packs = []
            if not any(r() is self for r in packs):
                packs.append(weakref.ref(self))
        return self.ohwi, self.ihwo

    def ohwi_for(self, ihwo):
        """the forward (OHWI) pack that belongs to the data-gradient pack `ihwo` a graph node saved -- None when the packs have been re-made since"""
        return self.ohwi if self.ihwo is ihwo else None

    def _fresh_key(self):
        """the key get() would compute now for the arguments of the last pack (after an in-place optimizer step on the master)"""
        src = self.src()
        k = self.key
        return (src.data_ptr(), src._version, _weight_epoch[0], getattr(src, "_uegan_epoch", 0)) + k[4:]      # (dtype ... pair, dup unchanged)


class PackTable:
    """Device table for uegan_pack_weights_multi over the packed copies of a set of master weights; rebuilt when a copy was
    (re)allocated or a new one appeared."""

    def __init__(self):
        self.sig, self.table, self.total, self.n, self.dtype = None, None, 0, 0, None

    def repack(self, params):
        packs, dtype = [], get_compute_dtype()
        for p in params:
            for r in getattr(p, "_uegan_packs", ()):
                pw = r()
                if pw is not None and pw.key is not None and pw.src() is p and pw.ohwi.dtype == dtype and pw.args[0] == p.data_ptr():
                    packs.append(pw)
        if not packs:
            return
        sig = tuple((id(pw), pw.ohwi.data_ptr(), pw.ihwo.data_ptr()) + pw.args for pw in packs)
        if sig != self.sig:
            ents = (L.PackEntry * len(packs))()
            start = 0
            for e, pw in zip(ents, packs):
                wptr, co, ci, ci_total, kh, kw, cout_pad, cin_pad, kp, kp2, lo_ptr, dup = pw.args
                e.w_oihw, e.w_ohwi, e.w_ihwo, e.start = wptr, pw.ohwi.data_ptr(), pw.ihwo.data_ptr(), start
                e.w_ohwi_lo, e.flags = (lo_ptr or None), dup
                e.Cout, e.Cin, e.Cin_total, e.KH, e.KW, e.Cout_pad, e.Cin_pad, e.Kp, e.Kp2 = co, ci, ci_total, kh, kw, cout_pad, cin_pad, kp, kp2
                start += cout_pad * kp + cin_pad * kp2
            host = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8)
            self.table = host.to(packs[0].ohwi.device)
            self.sig, self.total, self.n, self.dtype = sig, start, len(packs), _dt(packs[0].ohwi)
        L.check(lib().uegan_pack_weights_multi(self.dtype, _p(self.table), self.n, self.total, _stream()))
        for pw in packs:
            pw.key = pw._fresh_key()
            pw.version += 1


class ConvCfg:
    """Static configuration of one conv layer.  `in_act` / `premasked` implement deferred activation gradients (an exact
    restructuring, include/uegan_hip.h uegan_conv2d_dgrad_act): `in_act` = the activation that produced this conv's input
    x1 -- the data gradient is multiplied by act'(x1) in the dgrad epilogue; `premasked` = every consumer of this conv's
    output does that for it, so backward() skips its own act_bwd pass.  Only a module that owns the whole chain may set them
    (losses.VGG19_relu with deferred_act_grad=True); the defaults are plain autograd semantics."""
    __slots__ = ("stride", "pad_mode", "act", "packed", "packed_il", "in_act", "premasked", "cin_used")

    def __init__(self, stride, pad_mode, act, cin_used=None):
        self.stride, self.pad_mode, self.act = stride, pad_mode, act
        self.packed = PackedWeight()
        self.packed_il = PackedWeight()     # stride-2 forwards on a weight pair: [hi | lo] per tap in one matrix (ConvExtras.pair_w)
        self.in_act, self.premasked = ACT_NONE, False
        self.cin_used = cin_used        # the conv uses only the first cin_used input channels of its weight tensor (models.GAM)


class SNCall:
    """Spectral-norm state of ONE forward call: sigma (device fp32 [2] = sigma, 1/sigma) and the u, v used."""
    __slots__ = ("sigma", "u", "v")

    def __init__(self, sigma, u, v):
        self.sigma, self.u, self.v = sigma, u, v


def _desc(x1, x2, weight, cfg):
    B, H, W, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[3]
    co, ci_total, kh, kw = weight.shape
    ci = ci_total if cfg.cin_used is None else cfg.cin_used
    e = chunk_elems(x1.dtype)
    if C1 % e or C2 % e:
        raise RuntimeError("conv: NHWC tensors must carry channel counts padded to multiples of %d (got %d, %d)" % (e, C1, C2))
    if not (ci == C1 + C2 or (C2 == 0 and cpad(ci, x1.dtype) == C1)):
        raise RuntimeError("conv: weight expects %d input channels, got %d" % (ci, C1 + C2))
    pad = (kh - 1) // 2
    Ho = (H + 2 * pad - kh) // cfg.stride + 1
    Wo = (W + 2 * pad - kw) // cfg.stride + 1
    if cfg.pad_mode == PAD_REFLECT and (pad >= H or pad >= W):
        raise RuntimeError("Padding size should be less than the corresponding input dimension (pad %d, input %dx%d)" % (pad, H, W))
    return L.ConvDesc(_dt(x1), B, H, W, C1, C2, Ho, Wo, cpad(co, x1.dtype), kh, kw, cfg.stride, pad, cfg.pad_mode, cfg.act, ci, co, ci_total)


class ConvExtras:
    """Extras of ONE forward convolution (uegan_conv2d_fwd_ex): the request (constructor) and, after the call, what the kernel produced.
      x1_lo / x2_lo   lo planes of the sources (hi + lo pairs, see set_precise)
      pair_w          multiply by the weights as a hi + lo pair;  dup_cin: the source carries its own lo plane in channels [Cin, 2 Cin) (to_nhwc(pair=True))
      want_lo         -> y_lo: the lo plane of the result
      mul / mul_lo    -> prod (/ prod_lo when want_mul_lo): act(...) * (mul + mul_lo) formed from the fp32 result (models.py:69)
      res             (xa,) or (xa, xb): NCHW fp32 image sets -> res_out: clamp(act(...) + x, -1, 1) per set (models.py:70-72), from the fp32 result
    taken: did a kernel honour the request?  False: the plain convolution ran and every output field is None -- a caller that only asked for an
    epilogue (mul / res) then runs the separate kernel; a request that involves pairs raises instead (there is no plain equivalent)."""
    __slots__ = ("x1_lo", "x2_lo", "pair_w", "dup_cin", "want_lo", "mul", "mul_lo", "want_mul_lo", "res", "y_lo", "prod", "prod_lo", "res_out", "taken")

    def __init__(self, x1_lo=None, x2_lo=None, pair_w=False, dup_cin=False, want_lo=False, mul=None, mul_lo=None, want_mul_lo=False, res=None):
        self.x1_lo, self.x2_lo, self.pair_w, self.dup_cin, self.want_lo = x1_lo, x2_lo, pair_w, dup_cin, want_lo
        self.mul, self.mul_lo, self.want_mul_lo, self.res = mul, mul_lo, want_mul_lo, res
        self.y_lo = self.prod = self.prod_lo = self.res_out = None
        self.taken = False

    def needs_pairs(self):
        return self.x1_lo is not None or self.x2_lo is not None or self.pair_w or self.want_lo or self.want_mul_lo or self.mul_lo is not None


def _conv_fwd_ex(d, x1, x2, ohwi, ohwi_lo, biasc, scale, y, ex, stats, interleaved=False):
    """uegan_conv2d_fwd_ex for one layer: fills ex's output fields (and stats.value); False: nothing was launched.
    interleaved: ohwi is the [hi | lo] matrix of a stride-2 forward (ConvCfg.packed_il)"""
    dev, dt = x1.device, x1.dtype
    e = L.ConvEx()
    e.w_interleaved = 1 if interleaved else 0
    shape = (d.B, d.Ho, d.Wo, d.Cout)
    e.x1_lo, e.x2_lo, e.w_lo = _p(ex.x1_lo), _p(ex.x2_lo), _p(ohwi_lo)
    y_lo = torch.empty(shape, dtype=dt, device=dev) if ex.want_lo else None
    prod = torch.empty(shape, dtype=dt, device=dev) if ex.mul is not None else None
    prod_lo = torch.empty(shape, dtype=dt, device=dev) if (ex.mul is not None and ex.want_mul_lo) else None
    e.y_lo, e.mul, e.mul_lo, e.y_mul, e.y_mul_lo = _p(y_lo), _p(ex.mul), _p(ex.mul_lo), _p(prod), _p(prod_lo)
    outs = None
    if ex.res is not None:
        xs = [x.detach().contiguous() for x in ex.res]
        if any(x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != d.Cout_w or tuple(x.shape[2:]) != (d.Ho, d.Wo) for x in xs) or \
                sum(x.shape[0] for x in xs) != d.B or len(xs) > 2:
            raise RuntimeError("conv residual epilogue: one or two float32 NCHW image sets covering the batch expected")
        outs = [torch.empty_like(x) for x in xs]
        e.res_x, e.res_out, e.res_split = _p(xs[0]), _p(outs[0]), xs[0].shape[0]
        if len(xs) == 2:
            e.res_x2, e.res_out2 = _p(xs[1]), _p(outs[1])
        _chk(*xs)
    _chk(ex.x1_lo, ex.x2_lo, ex.mul, ex.mul_lo)
    st = ws = None
    if stats is not None:
        wsb = lib().uegan_conv2d_fwd_ex_workspace_bytes(C.byref(d), C.byref(e))
        if wsb:
            st = torch.empty((2, d.B, d.Cout), dtype=torch.float32, device=dev)
            ws = torch.empty(((wsb + 3) // 4,), dtype=torch.float32, device=dev)      # (core.workspace() spelled out: no extra Python frame on a forward launch)
            e.mean, e.rstd, e.stats_workspace, e.stats_workspace_bytes, e.eps = _p(st[0]), _p(st[1]), _p(ws), wsb, IN_EPS
    taken = C.c_int(0)
    L.check(lib().uegan_conv2d_fwd_ex(C.byref(d), C.byref(e), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), C.byref(taken), _stream()))
    if not taken.value:
        return False
    ex.taken, ex.y_lo, ex.prod, ex.prod_lo, ex.res_out = True, y_lo, prod, prod_lo, (tuple(outs) if outs is not None else None)
    if stats is not None:
        stats.value = st if (taken.value & 2) else None
    return True


split_k = [True]      # small-grid forwards (single-image inference) may split their K loop over several workgroups per tile (uegan_conv2d_fwd_splitk)


def _fwd(d, x1, x2, ohwi, biasc, scale, y, stats=None):
    """THE forward launch of a plain convolution (conv2d without extras, raw_conv_fwd without pool).  stats: a StatsHolder -- the InstanceNorm that
    follows wants the per-(image, channel) moments of y, and the streaming kernel's epilogue emits them where it takes the layer
    (uegan_conv2d_fwd_stats); else uegan_conv2d_fwd -- with a workspace for a split-K launch where the library would use one (the deep layers of a
    single-image forward)"""
    if stats is not None:
        wsb = lib().uegan_conv2d_fwd_stats_workspace_bytes(C.byref(d))
        if wsb:
            st = torch.empty((2, d.B, d.Cout), dtype=torch.float32, device=x1.device)
            ws = torch.empty(((wsb + 3) // 4,), dtype=torch.float32, device=x1.device)      # (core.workspace() spelled out: no extra Python frame on a forward launch)
            produced = C.c_int(0)
            L.check(lib().uegan_conv2d_fwd_stats(C.byref(d), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), _p(st[0]), _p(st[1]), IN_EPS, _p(ws), wsb,
                                                 C.byref(produced), _stream()))
            stats.value = st if produced.value else None
            return
        stats.value = None
    if split_k[0] and x1.dtype != torch.float32 and d.B * d.Ho * d.Wo <= 65536 and d.Cout >= 64:
        wsb = lib().uegan_conv2d_fwd_splitk_workspace_bytes(C.byref(d))
        if wsb:
            ws = torch.empty(((wsb + 3) // 4,), dtype=torch.float32, device=x1.device)      # (core.workspace() spelled out: no extra Python frame on a forward launch)
            L.check(lib().uegan_conv2d_fwd_splitk(C.byref(d), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), _p(ws), wsb, _stream()))
            return
    L.check(lib().uegan_conv2d_fwd(C.byref(d), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), _stream()))


def refuse_stale_pack(packed, ihwo, version, message):
    """torch raises its "modified by an inplace operation" version error for `out = net(x); optimizer.step(); out.backward()`; the optimizer's
    one-launch re-pack (PackTable.repack) rewrites the packed copy `ihwo` a graph saved at `version`, so the same pattern is refused here"""
    if packed.ihwo is ihwo and packed.version != version:
        raise RuntimeError(message)


def _dgrad(d, dz, ihwo, scale, dx1, dx2, in_act=ACT_NONE, x_act=None):
    """THE data-gradient launch: dx1 (, dx2) = dgrad(dz) [* in_act'(x_act)] into the caller's tensors; the workspace is non-empty for a small
    reflect-padded map (pad-grid dgrad + fold)"""
    dwsb = lib().uegan_conv2d_dgrad_workspace_bytes(C.byref(d))
    dws = workspace(dwsb, dz.device)
    if in_act != ACT_NONE:
        if dx2 is not None:
            raise RuntimeError("conv: in_act (deferred activation gradient) needs a single-input conv")
        L.check(lib().uegan_conv2d_dgrad_act(C.byref(d), _p(dz), _p(ihwo), _p(scale), _p(dx1), _p(dws), dwsb, in_act, _p(x_act), _stream()))
    else:
        L.check(lib().uegan_conv2d_dgrad_ws(C.byref(d), _p(dz), _p(ihwo), _p(scale), _p(dx1), _p(dx2), _p(dws), dwsb, _stream()))


def _wgrad(d, x1, x2, dz, scale, weight, wsink, bsink, has_bias, want_w, sn=None, cin_used=None, finish=None):
    """THE weight-gradient launch -> (dw, db) for autograd, None where the gradient went into the parameters' sinks (_wgrad_target);
    finish(dw): runs between the launch and the hand-over, on this call's gradient in place"""
    wsb = lib().uegan_conv2d_wgrad_workspace_bytes(C.byref(d))
    ws = workspace(wsb, dz.device, least=4)
    sink, dw, db, acc = _wgrad_target(wsink, bsink, has_bias, want_w, sn, weight, cin_used, d.Cout_w, dz.device)
    L.check(lib().uegan_conv2d_wgrad_acc(C.byref(d), _p(x1), _p(x2), _p(dz), _p(scale), _p(dw), _p(db), _p(ws), wsb, acc, _stream()))
    if finish is not None:
        finish(dw)
    return _wgrad_done(sink, wsink, bsink, has_bias, dw, db)


def _wgrad_target(wsink, bsink, has_bias, want_w, sn, weight, cin_used, n_bias, dev):
    """where a layer's weight (and bias) gradient goes -> (sink, dw, db, acc): straight into the optimizer's flat bucket when both gradients live
    there (acc: beta = 1 after the first touch; the spectral-norm correction works in place on ONE call's gradient, so it needs the first touch),
    else into fresh tensors for autograd"""
    sink = (wsink is not None and want_w and (not has_bias or (bsink is not None and bsink.dirty == wsink.dirty)) and (sn is None or not wsink.dirty))
    if sink:
        return True, wsink.view, (bsink.view if has_bias else None), (3 if wsink.dirty else 0)
    # (a column-slice conv writes only its own columns: the rest of the gradient is zero)
    dw = (torch.zeros if cin_used is not None else torch.empty)(weight.shape, dtype=torch.float32, device=dev)
    db = torch.empty((n_bias,), dtype=torch.float32, device=dev) if has_bias else None
    return False, dw, db, 0


def _wgrad_done(sink, wsink, bsink, has_bias, dw, db):
    """after the weight-gradient launch: what autograd gets (None where the gradient went into a sink, which is told)"""
    if not sink:
        return dw, db
    wsink.mark()
    if has_bias:
        bsink.mark()
    return None, None


class _ConvFn(torch.autograd.Function):
    """y = act(scale * conv(pad(cat[x1,x2]), W) + b)  -- uegan_conv2d_fwd / dgrad / wgrad."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, cfg, sn, wkey, n_out=1, stats=None, ex=None, premasked=None):
        x1 = x1.contiguous()
        x2 = None if x2 is None else x2.contiguous()
        d = _desc(x1, x2, weight, cfg)
        pair_w = ex is not None and ex.pair_w
        ohwi, ihwo = cfg.packed.get(weight, x1.dtype, d.C1 + d.C2, d.Cout, wkey, cfg.cin_used, pair=pair_w and cfg.stride != 2,
                                    dup=1 if (ex is not None and ex.dup_cin) else 0)
        y = torch.empty((d.B, d.Ho, d.Wo, d.Cout), dtype=x1.dtype, device=x1.device)
        biasc = None if bias is None else bias.detach().contiguous()
        scale = None if sn is None else sn.sigma[1:]
        _chk(x1, x2, y, biasc)
        done = False
        if ex is not None and pair_w and cfg.stride == 2 and x1.dtype != torch.float32:
            # a stride-2 forward on a weight pair: the pair lives in ONE matrix, per tap the hi part of the input channels' weights and then their lo part
            # (the kernel reads the source's channels twice); the plain packs above still serve the backward
            w_il, _ = cfg.packed_il.get(weight, x1.dtype, 2 * (d.C1 + d.C2), d.Cout, wkey, cfg.cin_used, dup=2)
            done = _conv_fwd_ex(d, x1, x2, w_il, None, biasc, scale, y, ex, stats, interleaved=True)
        elif ex is not None:
            done = x1.dtype != torch.float32 and _conv_fwd_ex(d, x1, x2, ohwi, cfg.packed.ohwi_lo if pair_w else None, biasc, scale, y, ex, stats)
            if not done and ex.needs_pairs():
                raise RuntimeError("conv: no kernel takes this layer (%dx%d, %d + %d -> %d channels on %dx%d) with hi + lo pairs (the precise mode covers "
                                   "the conv_dim = 32 generator's full-resolution layers in a 16-bit storage dtype)"
                                   % (d.KH, d.KW, d.C1, d.C2, d.Cout, d.H, d.W))
        if not done:
            _fwd(d, x1, x2, ohwi, biasc, scale, y, stats)
        ctx.cfg, ctx.sn, ctx.d, ctx.ihwo = cfg, sn, d, ihwo
        # (premasked is the layer's static setting unless THIS call's consumer says otherwise: gam_hub takes over the activation backward of the
        # encoder layers in front of the full-resolution attention modules only where the library offers the one-pass kernel)
        ctx.premasked = cfg.premasked if premasked is None else bool(premasked)
        ctx.pack_version = cfg.packed.version
        ctx.has_x2, ctx.has_bias = x2 is not None, bias is not None
        ctx.wsink, ctx.bsink = _sink_of(weight), _sink_of(bias)
        ctx.save_for_backward(x1, x2, y, weight)
        if n_out == 1:
            return y
        # the activation has n_out consumers: hand each its own alias, so that backward() receives their gradients SEPARATELY and
        # sums them inside the activation-backward kernel (autograd would otherwise add them with n_out - 1 elementwise kernels)
        return tuple(y.view_as(y) for _ in range(n_out))

    @staticmethod
    def backward(ctx, *gs):
        x1, x2, y, weight = ctx.saved_tensors
        cfg, sn, d = ctx.cfg, ctx.sn, ctx.d
        gs = [g.contiguous() for g in gs if g is not None]
        if not gs:
            raise RuntimeError("conv backward without any output gradient")
        st = _stream()
        if len(gs) > 3:
            raise RuntimeError("conv: at most 3 consumers per activation")
        g = gs[0]
        if len(gs) > 1 or (cfg.act != ACT_NONE and not ctx.premasked):
            dz = torch.empty_like(g)
            act = ACT_NONE if ctx.premasked else cfg.act
            L.check(lib().uegan_act_bwd3(_dt(g), act, _p(g), _p(gs[1]) if len(gs) > 1 else None, _p(gs[2]) if len(gs) > 2 else None, _p(y),
                                         _p(dz), g.numel(), st))
        else:
            dz = g
        scale = None if sn is None else sn.sigma[1:]
        dx1 = dx2 = dw = db = None
        if ctx.needs_input_grad[0] or (ctx.has_x2 and ctx.needs_input_grad[1]):
            refuse_stale_pack(cfg.packed, ctx.ihwo, ctx.pack_version,
                              "conv backward: the layer's weight was updated by an optimizer step after this forward (the packed "
                              "copy saved for the data gradient has been rewritten in place); run backward() before step()")
            dx1 = torch.empty_like(x1)
            dx2 = torch.empty_like(x2) if ctx.has_x2 else None
            _dgrad(d, dz, ctx.ihwo, scale, dx1, dx2, cfg.in_act, x1)
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            finish = None
            if sn is not None:
                def finish(dw):      # the spectral-norm correction of this call's gradient, in place
                    wd = weight.detach()
                    rows, cols = wd.shape[0], wd[0].numel()
                    tmp = torch.empty((lib().uegan_specnorm_grad_workspace_floats(),), dtype=torch.float32, device=g.device)
                    L.check(lib().uegan_specnorm_grad(_p(dw), _p(wd), _p(sn.u), _p(sn.v), _p(sn.sigma), _p(dw), rows, cols, _p(tmp), st))
            dw, db = _wgrad(d, x1, x2, dz, scale, weight, ctx.wsink, ctx.bsink, ctx.has_bias, ctx.needs_input_grad[2], sn, cfg.cin_used, finish)
        return dx1, dx2, dw, db, None, None, None, None, None, None, None


class StatsHolder:
    """conv2d(..., stats=holder): after the call holder.value is a [2, B, C] fp32 tensor (mean, rstd of InstanceNorm: biased variance, eps 1e-5)
    of the conv's result when the kernel that took the layer emitted the moments on its way out (uegan_conv2d_fwd_stats), else None"""
    __slots__ = ("value",)

    def __init__(self):
        self.value = None


def conv2d(x1, x2, weight, bias, cfg, sn=None, wkey=None, n_out=1, stats=None, ex=None, premasked=None):
    """n_out > 1: returns n_out aliases of the output, one per consumer (their gradients are summed inside the activation backward);
    ex: a ConvExtras (hi + lo pairs, product / residual epilogue: uegan_conv2d_fwd_ex) -- its outputs are plain tensors outside the graph;
    premasked: this call's value of ConvCfg.premasked (None: the layer's)"""
    return _ConvFn.apply(x1, x2, weight, bias, cfg, sn, wkey, n_out, stats, ex, premasked)


def specnorm_sigma(weight_orig, u, v, do_iter):
    """One power iteration (in place on u, v when do_iter) and sigma; returns SNCall (torch spectral_norm)."""
    wd = weight_orig.detach()
    rows, cols = wd.shape[0], wd[0].numel()
    sigma = torch.empty((2,), dtype=torch.float32, device=wd.device)
    tmp = torch.empty((lib().uegan_specnorm_multi_workspace_floats(rows, cols),), dtype=torch.float32, device=wd.device)
    _chk(wd, u, v)
    L.check(lib().uegan_specnorm_sigma(_p(wd), _p(u), _p(v), rows, cols, 1 if do_iter else 0, SN_EPS, _p(sigma), _p(tmp), _stream()))
    need_grad = torch.is_grad_enabled() and weight_orig.requires_grad
    return SNCall(sigma, u.clone() if need_grad else u, v.clone() if need_grad else v)


def _sub_desc(d, nb):
    """the same convolution on the first nb images of the batch"""
    if nb is None or nb == d.B:
        return d
    d2 = L.ConvDesc.from_buffer_copy(d)
    d2.B = nb
    return d2


def raw_conv_fwd(x1, x2, weight, bias, cfg, scale=None, wkey=None, pool=False, n_full=None, n_idx=0, stats=None):
    """y = act(scale * conv(pad(cat[x1, x2]), W) + b) -> (y, desc, w_ihwo); pool=True: -> (y, desc, w_ihwo, maxpool2x2(y)) with the
    pooled tensor written by the convolution's epilogue where the kernel can (uegan_conv2d_fwd_pool).  n_full (with pool): only the first
    n_full images need y itself -- y[n_full:] is UNDEFINED afterwards (uegan_conv2d_fwd_pool_part), the pooled tensor is complete.
    n_idx > 0 (with pool): -> (y, desc, w_ihwo, pooled, idx) with idx (uint8, pooled shape) the window position of each maximum for the first
    n_idx images (uegan_conv2d_fwd_pool_idx): raw_maxpool_bwd_idx routes the gradient with it instead of with y"""
    d = _desc(x1, x2, weight, cfg)
    ohwi, ihwo = cfg.packed.get(weight, x1.dtype, d.C1 + d.C2, d.Cout, wkey, cfg.cin_used)
    y = torch.empty((d.B, d.Ho, d.Wo, d.Cout), dtype=x1.dtype, device=x1.device)
    biasc = None if bias is None else bias.detach()
    _chk(x1, x2, y, biasc)
    if pool:
        yp = torch.empty((d.B, d.Ho // 2, d.Wo // 2, d.Cout), dtype=x1.dtype, device=x1.device)
        nf = d.B if n_full is None else int(n_full)
        if n_idx:
            idx = torch.empty((d.B, d.Ho // 2, d.Wo // 2, d.Cout), dtype=torch.uint8, device=x1.device)
            L.check(lib().uegan_conv2d_fwd_pool_idx(C.byref(d), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), _p(yp), _p(idx), nf, int(n_idx), _stream()))
            return y, d, ihwo, yp, idx
        L.check(lib().uegan_conv2d_fwd_pool_part(C.byref(d), _p(x1), _p(x2), _p(ohwi), _p(biasc), _p(scale), _p(y), _p(yp), nf, _stream()))
        return y, d, ihwo, yp
    _fwd(d, x1, x2, ohwi, biasc, scale, y, stats)       # (stats: a StatsHolder, see conv2d)
    return y, d, ihwo


def raw_conv_dgrad(d, dz, ihwo, scale=None, in_act=ACT_NONE, x_act=None, nb=None, two=False):
    """data gradient on the first `nb` images (default: all): dx1 (, dx2) = dgrad(dz) [* act'(x_act)]"""
    d = _sub_desc(d, nb)
    dev = dz.device
    dx1 = torch.empty((d.B, d.H, d.W, d.C1), dtype=dz.dtype, device=dev)
    dx2 = torch.empty((d.B, d.H, d.W, d.C2), dtype=dz.dtype, device=dev) if two else None
    _dgrad(d, dz, ihwo, scale, dx1, dx2, in_act, x_act)
    return dx1, dx2


def raw_conv_wgrad(d, x1, x2, dz, weight, bias, scale=None, nb=None):
    """weight (and bias) gradient over the first `nb` images, written into the parameters' gradient sinks when they have one
    (beta = 1 after the first touch) -- returns (dw, db) tensors for autograd, None where the gradient went into a sink."""
    return _wgrad(_sub_desc(d, nb), x1, x2, dz, scale, weight, _sink_of(weight), _sink_of(bias), bias is not None, want_w=True, sn=None, cin_used=None)
