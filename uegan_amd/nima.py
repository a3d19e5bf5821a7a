"""NIMA aesthetic score (metrics/NIMA/CalcNIMA.py) on the device: the metric the reference reports by default (config.py:80) and the
only one of its three that needs no label image.

    NIMA(pretrained_base_model=False)   MobileNetV2 trunk + ReLU -> Dropout -> Linear(1280, 10) -> Softmax head with the reference's
                                        state-dict keys, so `model.load_state_dict(torch.load('pretrain-model.pth'))` (CalcNIMA.py:66)
                                        works unchanged.  Eval mode only; forward(x): fp32 NCHW [B,3,224,224] in [0,1] -> [B,10]
    prepare_image(images_u8)            CalcNIMA.py:45-55 (Resize(256) -> CenterCrop(224) -> ToTensor) of uint8 BHWC images
    score(model, images_u8)             per-image mean score sum_j j*p_j and standard deviation (CalcNIMA.py:86-91)
    calc_nima(model, images)            their averages over a set (TRUE means)
    GraphedNIMA(model, batch)           the forward as one hipGraph launch for a fixed batch

The trunk runs as 53 convolution kernels (csrc/nima.h: first 3x3, depthwise 3x3, pointwise 1x1 on the matrix cores) with eval-mode BatchNorm
folded into a per-channel scale and shift, ReLU6 / ReLU as the clamp of the epilogue and the residual add in the projection's epilogue, plus
one head kernel (pool, ReLU, Linear, softmax, mean, std): 54 C-ABI calls per forward.  Storage and accumulation are fp32 whatever
ops.get_compute_dtype() says (a metric is a measuring instrument); that setting is left untouched.
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import data
from .ops import core
from .models import _InvalidatingModule

INPUT_SIZE = 224          # CenterCrop(224); the trunk's five stride-2 stages leave the 7x7 map AvgPool2d(7) expects
RESIZE = 256              # Resize(256): shorter side
CPAD = 16                 # channel padding of the scorer's NHWC tensors (csrc/nima.h NIMA_CPAD)
FIRST_CHANNELS, LAST_CHANNELS, N_SCORES = 32, 1280, 10
# MobileNetV2 (Sandler et al. 2018, table 2): expansion t, output channels c, repeats n, stride s of the first repeat
BLOCK_TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
INF = float("inf")


def _cp(c):
    return (c + CPAD - 1) // CPAD * CPAD


def _conv_bn(cin, cout, k, stride, groups=1):
    return [nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout)]


class _Block(nn.Module):
    """inverted residual: 1x1 expand (BN, ReLU6) -> depthwise 3x3 (BN, ReLU6) -> 1x1 project (BN), + input when the shapes allow.
    Parameter holder: the layers are run by NIMA.forward through the kernels, never called."""

    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hid = cin * t
        self.stride, self.residual = stride, stride == 1 and cin == cout
        self.conv = nn.Sequential(*(_conv_bn(cin, hid, 1, 1) + [nn.ReLU6(inplace=True)] + _conv_bn(hid, hid, 3, stride, groups=hid)
                                    + [nn.ReLU6(inplace=True)] + _conv_bn(hid, cout, 1, 1)))


def block_specs():
    """[(cin, cout, stride, t)] of the 17 blocks"""
    out, cin = [], FIRST_CHANNELS
    for t, c, n, s in BLOCK_TABLE:
        for i in range(n):
            out.append((cin, c, s if i == 0 else 1, t))
            cin = c
    return out


class NIMA(_InvalidatingModule):
    def __init__(self, pretrained_base_model=False):
        super().__init__()
        if pretrained_base_model:
            raise ValueError("no pretrained MobileNetV2 is bundled: load a NIMA checkpoint with load_state_dict")
        feats = [nn.Sequential(*(_conv_bn(3, FIRST_CHANNELS, 3, 2) + [nn.ReLU(inplace=True)]))]
        feats += [_Block(*spec) for spec in block_specs()]
        feats.append(nn.Sequential(*(_conv_bn(block_specs()[-1][1], LAST_CHANNELS, 1, 1) + [nn.ReLU(inplace=True)])))
        feats.append(nn.AvgPool2d(INPUT_SIZE // 32))
        self.base_model = nn.Sequential(nn.Sequential(*feats))
        self.head = nn.Sequential(nn.ReLU(inplace=True), nn.Dropout(p=0.75), nn.Linear(LAST_CHANNELS, N_SCORES), nn.Softmax(dim=1))
        for m in self.base_model.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
        self._packed = None
        self.eval()                     # the only mode the scorer runs in (CalcNIMA.py:68)

    # ---- folded, packed device copies of the weights ----
    def _apply(self, fn, *args, **kwargs):      # .to() / .cuda() / .float(): the packed copies live on the old device
        self._packed = None
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._packed = None

    def apply(self, fn):
        self._packed = None
        return super().apply(fn)

    def invalidate(self):
        """drop the folded weights (after editing parameters or BatchNorm statistics in place)"""
        self._packed = None

    @staticmethod
    def _fold(bn, cpad):
        """eval BatchNorm as y = x * scale + shift, in fp32 with running_var + eps under the root as F.batch_norm computes it"""
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
        pad = cpad - scale.numel()
        return nn.functional.pad(scale, (0, pad)).contiguous(), nn.functional.pad(shift, (0, pad)).contiguous()

    @staticmethod
    def _pack_pw(conv):
        w = conv.weight.detach().float()[:, :, 0, 0]
        out = torch.zeros((_cp(w.shape[0]), _cp(w.shape[1])), dtype=torch.float32, device=w.device)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    @staticmethod
    def _pack_taps(conv):
        """[Cout, Cin/groups, 3, 3] -> [(ky*3 + kx) * Cin/groups + ci][Cout padded]"""
        w = conv.weight.detach().float()
        co = w.shape[0]
        out = torch.zeros((9 * w.shape[1], _cp(co)), dtype=torch.float32, device=w.device)
        out[:, :co] = w.permute(2, 3, 1, 0).reshape(-1, co)
        return out

    def _plan(self):
        key = (core._weight_epoch[0], self.head[2].weight.device)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        feats = self.base_model[0]
        layers = []           # (kind, weight, scale, shift, lo, hi, stride, cout_pad, residual, block index or None)
        first = feats[0]
        layers.append(("first", self._pack_taps(first[0]), *self._fold(first[1], _cp(FIRST_CHANNELS)), 0.0, INF, 2, _cp(FIRST_CHANNELS), False, 0))
        for i in range(1, 18):
            blk = feats[i]
            c = blk.conv
            hid, cout = _cp(c[0].out_channels), _cp(c[6].out_channels)
            layers.append(("pw", self._pack_pw(c[0]), *self._fold(c[1], hid), 0.0, 6.0, 1, hid, False, None))
            layers.append(("dw", self._pack_taps(c[3]), *self._fold(c[4], hid), 0.0, 6.0, blk.stride, hid, False, None))
            layers.append(("pw", self._pack_pw(c[6]), *self._fold(c[7], cout), -INF, INF, 1, cout, blk.residual, i))
        last = feats[18]
        layers.append(("pw", self._pack_pw(last[0]), *self._fold(last[1], _cp(LAST_CHANNELS)), 0.0, INF, 1, _cp(LAST_CHANNELS), False, 18))
        fc = self.head[2]
        plan = (layers, fc.weight.detach().float().contiguous(), fc.bias.detach().float().contiguous())
        self._packed = (key, plan)
        return plan

    # ---- forward ----
    def _run(self, x, strides, B, taps=None):
        """x: device fp32 image batch [B, 3 channels, 224, 224] addressed by element `strides` (batch, channel, row, column).
        -> (pooled [B,1280], probs [B,10], mean [B], std [B]); taps: {feature index: None} filled with that layer's NHWC output."""
        if self.training:
            raise RuntimeError("NIMA runs in eval mode only (BatchNorm with batch statistics is not built): call model.eval()")
        layers, fw, fb = self._plan()
        lib, st, dev = core.lib(), core._stream(), x.device
        H = W = INPUT_SIZE
        cur, block_in = x, None
        for kind, w, scale, shift, lo, hi, stride, cout, residual, idx in layers:
            if kind == "first":
                H, W = (H - 1) // stride + 1, (W - 1) // stride + 1
                y = torch.empty((B, H, W, cout), dtype=torch.float32, device=dev)
                L.check(lib.uegan_nima_conv3x3_first(cur.data_ptr(), strides[0], strides[1], strides[2], strides[3], w.data_ptr(), scale.data_ptr(),
                                                     shift.data_ptr(), y.data_ptr(), B, INPUT_SIZE, INPUT_SIZE, cout, stride, lo, hi, st))
                block_in = y
            elif kind == "dw":
                Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                y = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=dev)
                L.check(lib.uegan_nima_dwconv3x3(cur.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), B, H, W, cout, stride,
                                                 lo, hi, st))
                H, W = Ho, Wo
            else:
                y = torch.empty((B, H, W, cout), dtype=torch.float32, device=dev)
                L.check(lib.uegan_nima_pwconv(cur.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), block_in.data_ptr() if residual else None,
                                              y.data_ptr(), B * H * W, cur.shape[3], cout, lo, hi, st))
                if idx is not None:
                    block_in = y
            if taps is not None and idx in taps:
                taps[idx] = y
            cur = y
        pooled = torch.empty((B, LAST_CHANNELS), dtype=torch.float32, device=dev)
        probs = torch.empty((B, N_SCORES), dtype=torch.float32, device=dev)
        mean = torch.empty((B,), dtype=torch.float32, device=dev)
        std = torch.empty((B,), dtype=torch.float32, device=dev)
        L.check(lib.uegan_nima_head(cur.data_ptr(), fw.data_ptr(), fb.data_ptr(), pooled.data_ptr(), probs.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                    B, H * W, cur.shape[3], LAST_CHANNELS, N_SCORES, st))
        return pooled, probs, mean, std

    @torch.no_grad()
    def forward_all(self, x, taps=None):
        """forward(x) with everything the head computes: (pooled features [B,1280], probabilities [B,10], mean [B], std [B])"""
        if self.training:
            raise RuntimeError("NIMA runs in eval mode only (BatchNorm with batch statistics is not built): call model.eval()")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise TypeError("NIMA expects a float32 [B,3,224,224] tensor")
        if x.shape[2] != INPUT_SIZE or x.shape[3] != INPUT_SIZE:
            raise ValueError("NIMA expects %dx%d inputs (prepare_image makes them), got %dx%d" % (INPUT_SIZE, INPUT_SIZE, x.shape[2], x.shape[3]))
        x = x.detach().contiguous()
        core._chk(x)
        hw = INPUT_SIZE * INPUT_SIZE
        return self._run(x, (3 * hw, hw, INPUT_SIZE, 1), x.shape[0], taps)

    def forward(self, x):
        return self.forward_all(x)[1]

    @torch.no_grad()
    def features(self, x, indices):
        """outputs of base_model[0][i] for i in indices (0: first layer, 1..17: blocks, 18: last 1x1), NCHW with the real channel counts"""
        taps = {int(i): None for i in indices}
        self.forward_all(x, taps)
        chans = [FIRST_CHANNELS] + [s[1] for s in block_specs()] + [LAST_CHANNELS]
        return {i: t[..., :chans[i]].permute(0, 3, 1, 2) for i, t in taps.items()}


# ---- preparation ----
_CROP_TABLES = {}


def resized_size(h, w):
    """torchvision Resize(256) on an h x w image: the shorter side becomes 256, the longer int(256 * long / short)"""
    if w <= h:
        return int(RESIZE * h / w), RESIZE
    return RESIZE, int(RESIZE * w / h)


def _crop_table(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _CROP_TABLES:
        tab, k = data._device_table(in_size, out_size, device)
        off = int(round((out_size - INPUT_SIZE) / 2.0))          # CenterCrop's offset
        _CROP_TABLES[key] = (tab[off:off + INPUT_SIZE].contiguous(), k)
    return _CROP_TABLES[key]


def _prepare(images_u8, cpad):
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise TypeError("prepare_image expects uint8 [B, h, w, 3] images (tester.to_uint8_image)")
    px = images_u8.contiguous()
    core._chk(px)
    B, h, w, _ = px.shape
    oh, ow = resized_size(h, w)
    if oh < INPUT_SIZE or ow < INPUT_SIZE:
        raise ValueError("image too small")
    dev = px.device
    htab, hk = _crop_table(w, ow, dev)
    vtab, vk = _crop_table(h, oh, dev)
    tmp = torch.empty((B, h, INPUT_SIZE, 3), dtype=torch.uint8, device=dev)
    shape = (B, 3, INPUT_SIZE, INPUT_SIZE) if cpad == 0 else (B, INPUT_SIZE, INPUT_SIZE, cpad)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    L.check(core.lib().uegan_nima_prepare(px.data_ptr(), B, h, w, INPUT_SIZE, INPUT_SIZE, htab.data_ptr(), hk, vtab.data_ptr(), vk, tmp.data_ptr(),
                                         out.data_ptr(), cpad, core._stream()))
    return out


def prepare_image(images_u8):
    """CalcNIMA.py:45-55 for a stack of decoded RGB images, uint8 [B,h,w,3] on the device -> fp32 [B,3,224,224] in [0,1]:
    Resize(256) (shorter side to 256, bilinear with antialiasing), CenterCrop(224), ToTensor.  The resize is Pillow's two-pass fixed-point
    resampler (uegan_amd.data.resample_table) and the result equals PIL.Image.resize(..., BILINEAR) + crop + /255 bit for bit.  torchvision
    is not a dependency of this project: as in uegan_amd/data.py the pin is against Pillow, which is what torchvision's Resize calls for a
    PIL image."""
    return _prepare(images_u8, 0)


@torch.no_grad()
def score(model, images_u8):
    """per-image NIMA of uint8 [B,h,w,3] device images (the bytes a saved PNG holds): (means, stds), two lists of B floats --
    mean = sum_j j * p_j, std = sqrt(sum_j p_j * (j - mean)^2), j = 1..10 (CalcNIMA.py:86-91)"""
    x = _prepare(images_u8, 4)                     # NHWC, read by the first layer through its strides: no layout pass
    _, _, mean, std = model._run(x, (INPUT_SIZE * INPUT_SIZE * 4, 1, INPUT_SIZE * 4, 4), x.shape[0])
    return mean.tolist(), std.tolist()


def calc_nima(model, images):
    """CalcNIMA.py:58-105 without the directory walk and the CSV files: (average mean score, average std) over `images`, a uint8 [B,h,w,3]
    stack or a list of uint8 [h,w,3] / [b,h,w,3] tensors of any sizes.  Like tester.mean_metric these are the TRUE means; the reference
    divides both totals by i = N - 1, the last index of its enumerate (CalcNIMA.py:99-100)."""
    stacks = [images] if torch.is_tensor(images) else list(images)
    means, stds = [], []
    for s in stacks:
        m, d = score(model, s.unsqueeze(0) if s.dim() == 3 else s)
        means += m
        stds += d
    return sum(means) / len(means), sum(stds) / len(stds)


class GraphedNIMA:
    """`model.forward_all` for a fixed batch as one hipGraph launch (cf. tester.GraphedGenerator): the 54 kernels are captured once on a side
    stream and replayed; nothing in the forward allocates outside the graph's pool or synchronises.  The folded weights are made at capture
    time: re-capture (`.capture()`) after the weights change."""

    def __init__(self, model, batch, device=None):
        self.model = model
        dev = device if device is not None else model.head[2].weight.device
        self.x = torch.zeros((batch, 3, INPUT_SIZE, INPUT_SIZE), dtype=torch.float32, device=dev)
        self.graph, self.out = None, None
        self.capture()

    @torch.no_grad()
    def capture(self):
        self.model.eval()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                       # warm-up: folds the weights, fills the allocator pool
                self.model.forward_all(self.x)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self.model.forward_all(self.x)

    @torch.no_grad()
    def forward_all(self, x):
        self.x.copy_(x)
        self.graph.replay()
        return self.out

    def __call__(self, x):
        return self.forward_all(x)[1]


# ---- seeded weights (fixtures and tests: no pretrained checkpoint exists offline) ----
def seeded_state_dict(seed, bn_stats=None):
    """A full NIMA state dict from one numpy generator: conv weights N(0, 2/fan_in), head.2 weight and bias N(0, 0.08^2), BatchNorm gamma
    U[0.5, 1.5] and beta U[-0.3, 0.3]; running statistics from `bn_stats` ({key: array}) where given, else 0 / 1."""
    rng = np.random.default_rng(seed)
    ref = NIMA().state_dict()
    out = OrderedDict()
    for k, v in ref.items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            t = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_mean") or k.endswith("running_var"):
            t = torch.from_numpy(np.asarray(bn_stats[k], dtype=np.float32)) if bn_stats is not None and k in bn_stats \
                else (torch.zeros(shape) if k.endswith("running_mean") else torch.ones(shape))
        elif k.startswith("head."):
            t = torch.from_numpy((rng.standard_normal(shape) * 0.08).astype(np.float32))
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            t = torch.from_numpy((rng.standard_normal(shape) * math.sqrt(2.0 / fan_in)).astype(np.float32))
        elif k.endswith("weight"):
            t = torch.from_numpy(rng.uniform(0.5, 1.5, shape).astype(np.float32))
        else:
            t = torch.from_numpy(rng.uniform(-0.3, 0.3, shape).astype(np.float32))
        out[k] = t
    return out


def tensor_checksum(t):
    """(sum, sum of squares) in float64: the fixture's per-tensor fingerprint of the seeded weights"""
    a = np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)
    return np.array([a.sum(), (a * a).sum()])
