"""FusedAdamL2: Adam with L2 weight decay over every parameter of a network in one launch."""
import torch

from .. import _lib as L
from .conv import PackTable
from .core import GradSink, _p, _stream, invalidate_weight_caches, lib
from .elementwise import zero_


class FusedAdamL2:
    """torch.optim.Adam(lr, betas, eps, weight_decay) semantics (trainer.py:337-338) as ONE kernel launch over all
    tensors; gradients are read from a flat fp32 bucket (the RCCL all-reduce buffer) scaled by `grad_scale`.
    `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format (the reference checkpoint's `g_optimizer` /
    `d_optimizer` entries, trainer.py:199-207, 409-410)."""

    def __init__(self, params, lr, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-4):
        self.params = [p for p in params if p.requires_grad]
        self.before_access = None        # set by the Trainer: applies an update it left pending (data-parallel overlap) before the
                                         # optimizer's state or learning rate is read or changed from outside
        self._in_step = False
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.initial_lr = None           # set by trainer.LambdaLR (torch writes `initial_lr` into the param group)
        self.step_count = 0
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.flat_grad = torch.zeros((total,), dtype=torch.float32, device=dev)
        self.m = torch.zeros_like(self.flat_grad)
        self.v = torch.zeros_like(self.flat_grad)
        descs = (L.AdamTensor * len(self.params))()
        off = 0
        self.max_n = 0
        self._offsets = []
        for i, p in enumerate(self.params):
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("FusedAdamL2 expects contiguous float32 parameters")
            n = p.numel()
            p.grad = self.flat_grad[off:off + n].view_as(p)       # autograd accumulates in place into the bucket
            p._uegan_sink = GradSink(p.grad)                      # ... and the weight-gradient kernels write it directly
            descs[i].p = p.data_ptr()
            descs[i].g = self.flat_grad.data_ptr() + 4 * off
            descs[i].m = self.m.data_ptr() + 4 * off
            descs[i].v = self.v.data_ptr() + 4 * off
            descs[i].n = n
            self._offsets.append(off)
            off += n
            self.max_n = max(self.max_n, n)
        raw = bytes(descs)
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        self.desc_dev = host.to(dev)
        self._views = [p.grad for p in self.params]
        self._packs = PackTable()

    def _flush(self):
        if self.before_access is not None and not self._in_step:
            self._in_step = True
            try:
                self.before_access()
            finally:
                self._in_step = False

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._flush()                    # a pending update belongs to the OLD learning rate
        self._lr = value

    def zero_grad(self):
        zero_(self.flat_grad)
        for p, v in zip(self.params, self._views):
            p.grad = v
            p._uegan_sink.dirty = False

    def step(self, grad_scale=1.0):
        self.step_count += 1
        for p, v in zip(self.params, self._views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                raise RuntimeError("FusedAdamL2: a parameter's .grad no longer aliases the flat bucket")
        L.check(lib().uegan_adam_l2_step(_p(self.desc_dev), len(self.params), self.max_n, self.lr, self.betas[0], self.betas[1], self.eps,
                                         self.weight_decay, grad_scale, self.step_count, _stream()))
        invalidate_weight_caches(self.params)
        self._packs.repack(self.params)          # every packed copy of the updated weights, one launch

    # ---- torch.optim.Adam checkpoint format
    @property
    def param_groups(self):
        g = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
             "params": list(range(len(self.params)))}
        if self.initial_lr is not None:
            g["initial_lr"] = self.initial_lr
        return [g]

    def state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} exactly as torch.optim.Adam.state_dict():
        parameter index = position in the constructor's iterable, empty `state` before the first step.  `step` is a Python int
        (torch 1.4, the reference's version; current torch converts it on load)."""
        self._flush()
        state = {}
        if self.step_count > 0:
            for i, (p, off) in enumerate(zip(self.params, self._offsets)):
                n = p.numel()
                state[i] = {"step": self.step_count, "exp_avg": self.m[off:off + n].view_as(p).clone(),
                            "exp_avg_sq": self.v[off:off + n].view_as(p).clone()}
        return {"state": state, "param_groups": self.param_groups}

    def load_state_dict(self, sd):
        self._flush()
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        g = groups[0]
        if g.get("amsgrad", False):
            raise NotImplementedError("amsgrad checkpoints are not supported (the reference never sets it, trainer.py:337-338)")
        self.lr, self.betas, self.eps, self.weight_decay = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"])
        if "initial_lr" in g:
            self.initial_lr = float(g["initial_lr"])
        state = sd["state"]
        steps = set()
        self.m.zero_()
        self.v.zero_()
        for key, st in state.items():
            i = int(key)
            p, off = self.params[i], self._offsets[i]
            n = p.numel()
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("optimizer state %d has shape %s, parameter has %s" % (i, tuple(st["exp_avg"].shape), tuple(p.shape)))
            self.m[off:off + n].view_as(p).copy_(st["exp_avg"])
            self.v[off:off + n].view_as(p).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(state) not in (0, len(self.params)) or len(steps) > 1:
            raise ValueError("FusedAdamL2 keeps ONE step counter: every parameter must carry the same `step` (got %s)" % sorted(steps))
        self.step_count = steps.pop() if steps else 0
