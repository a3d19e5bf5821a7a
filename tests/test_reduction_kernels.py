"""Kernel-level parity of the per-(image, channel) reductions of norm.hip, in every regime of their work decomposition:

* `uegan_moments` and the statistics of `uegan_instnorm_fwd`
* `uegan_instnorm_fwd / _apply / _bwd` (direct calls and `ops.instnorm` with and without given moments), `uegan_instnorm_apply_pair`
* `uegan_affine_act_fwd / _bwd_sums / _bwd_apply`, every activation of `variants.ACT_CODES`, explicit and NULL coefficients
* `uegan_percep_tap_fwd / _fwd_given / _bwd / _bwd_act / _bwd_acc`

All of them run on `make_plan` -> RedPlan{V, CG, PL, ncg, S, chunk}.  `plan()` below restates it (cross-checked on every case against the one
thing the library exposes, `uegan_reduce_workspace_floats`), and every case carries the regime it exists for as values of that plan
(WITNESS); they are asserted for the backend and storage type a test runs on before any kernel runs, so a case cannot silently stop
covering its regime when a threshold of make_plan moves.

Every reference is plain PyTorch in float64 on the kernel's own operands (rounded to the storage type first), written from the formulas in
the header of norm.hip; none goes through a kernel or through `ops`.  Tolerances are test_ops.py's (what a kernel keeps in fp32 -- statistics,
sums, the loss -- is held to F32_TOL whatever the storage type, a stored tensor to the storage tolerance, the InstanceNorm gradient to 5 x
that, as test_resample_pool_norm_elementwise does) or derived where they stand; per tensor, max-abs error over max-abs reference
(helpers.rel).  Conventions (margins at activation kinks, NaN-filled workspaces, sentinel-filled outputs, `OBS|family|backend|what|error|
tolerance` lines, DESIGN.md section 4 records the largest) are test_loss_optim_kernels.py's.  A workspace this file owns additionally sits
between two guard bands that must come back untouched.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import BACKENDS, half_round, rel, use_backend
from test_loss_optim_kernels import DTYPE_IDS, DTYPES, MARGIN, NAN, held, held_scalar, storage_tol
from test_ops import F32_TOL
from uegan_amd import _lib, ops, variants

EPS = ops.IN_EPS
SENT = -32768.0          # sentinel of the output buffers: exact in every storage type, far outside every result here
GUARD = 12345.0          # the guard bands around a workspace
GUARD_N = 1024
GRID_TARGET = {"emu": 64, "gpu": 1024}       # make_plan's kGridTarget: UEGAN_EMU / the device


# --------------------------------------------------------------------------------------------------------------------
# make_plan, restated
# --------------------------------------------------------------------------------------------------------------------
def plan(B, HW, C, epc, grid_target):
    """RedPlan of a [B, HW, C] tensor whose 16-byte chunk holds `epc` elements (4: fp32, 8: 16-bit storage), plus what the witnesses read:
    last = pixels of the last split, live = channel lanes of the last group that own channels, trips / tail = how often the finalize wave
    strides over the splits and how many lanes take part in the last (partial) trip"""
    V = epc if C % epc == 0 else 1
    lanes = C // V
    CG = 1
    while CG < lanes and CG < 64:
        CG *= 2
    PL, ncg = 256 // CG, -(-lanes // CG)
    s, cap = -(-HW // 1024), 64
    while B * ncg * cap < 512 and cap < 512:
        cap *= 2
    s = max(1, min(s, cap))
    while B * ncg * s < grid_target and s < 2048 and HW // (2 * s) >= 128:
        s *= 2
    while HW <= 4096 and ncg * s < 128 and s < 2048 and HW // (2 * s) >= 16:
        s *= 2
    chunk = -(-HW // s)
    S = -(-HW // chunk)
    return dict(V=V, CG=CG, PL=PL, ncg=ncg, S=S, chunk=chunk, last=HW - (S - 1) * chunk, live=lanes - (ncg - 1) * CG,
                trips=-(-S // 64), tail=S % 64)


def epc_of(dtype):
    return 4 if dtype == torch.float32 else 8


def plan_of(backend, dtype, case):
    return plan(*case, epc_of(dtype), GRID_TARGET[backend])


def W(*where, **want):
    """one witness: plan values that hold where every tag of `where` applies ("emu" / "gpu": the backend, "f32" / "h16": the chunk width)"""
    return where, want


# (B, HW, C) -> the regime the case pins
WITNESS = {
    # one pixel: every pixel lane but one is empty; var = 0 -> rstd = 1 / sqrt(eps); the backward is exactly 0
    (1, 1, 8): [W(S=1, chunk=1), W("f32", V=4, PL=128), W("h16", V=8, PL=256)],
    # HW < PL: S = 1, Chan merges with nb = 0 partners
    (1, 9, 64): [W(S=1, chunk=9, ncg=1), W("f32", V=4, PL=16), W("h16", V=8, PL=32)],
    # V = 1, CG = 8 with 3 dead channel lanes, S = 2
    (2, 48, 5): [W(V=1, CG=8, live=5, S=2, chunk=24)],
    # V = 1, CG = 4, PL = 64 > HW
    (1, 17, 3): [W(V=1, CG=4, live=3, PL=64, S=1, chunk=17)],
    # V = 4 with CG = 32 (18 live lanes) / V = 8 with CG = 16 (9 live); S = 16, chunk 19, last split 15
    (1, 300, 72): [W(S=16, chunk=19, last=15, ncg=1), W("f32", V=4, CG=32, live=18), W("h16", V=8, CG=16, live=9)],
    # V = 1, two channel groups, the last with 6 live lanes of 64; S = 64 (the last size with one finalize trip), PL = 4
    (1, 1600, 70): [W(V=1, CG=64, ncg=2, live=6, S=64, PL=4, trips=1)],
    # ragged last group of several (2 / 1 live lanes); S = 32, last split 8 of 32
    (2, 1000, 520): [W(CG=64, PL=4, S=32, chunk=32, last=8), W("f32", V=4, ncg=3, live=2), W("h16", V=8, ncg=2, live=1)],
    # S = 93 > 64: the finalize wave's second trip on lanes 0..28 only; chunk 27, last split 16
    (1, 2500, 40): [W(S=93, trips=2, tail=29, chunk=27, last=16)],
    # S = 128 from the small-map loop; chunk 32 < PL = 128 / 256; last split 31
    (1, 4095, 8): [W(S=128, trips=2, chunk=32, last=31), W("f32", V=4, PL=128), W("h16", V=8, PL=256)],
    # just above the small-map loop: S = 20; fp32 V = 4 (3 live of 4 lanes), 16-bit falls to V = 1
    (1, 4097, 12): [W(S=20, chunk=205, last=202), W("f32", V=4, CG=4, live=3), W("h16", V=1, CG=16, live=12)],
    # HW > 4096, non-dividing chunk; the split count follows the grid target
    (1, 66000, 8): [W("emu", S=65, trips=2, tail=1, chunk=1016, last=976), W("gpu", S=260, trips=5, tail=4, chunk=254, last=214)],
    # the largest split count: 16 partials per finalize lane on the device
    (1, 131072, 8): [W("emu", S=128, trips=2, chunk=1024), W("gpu", S=1024, trips=16, tail=0, chunk=128)],
}
CASES = list(WITNESS)


def case_id(c):
    return "x".join(map(str, c))


def regime(backend, dtype, case):
    """asserts the case's witnesses for this backend and storage type -> its plan"""
    p = plan_of(backend, dtype, case)
    tags = {backend, "f32" if dtype == torch.float32 else "h16"}
    seen = 0
    for where, want in WITNESS[case]:
        if set(where) <= tags:
            seen += 1
            for k, v in want.items():
                assert p[k] == v, (case, backend, dtype, k, p[k], v)
    assert seen > 0, (case, backend)
    return p


def start(backend, dtype, case=None):
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    if case is not None:
        regime(backend, dtype, case)
    return dev, lib


def fam(name, dtype):
    return "%s %s" % (name, DTYPE_IDS[DTYPES.index(dtype)])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES + [(3, 4096, 8), (3, 1024, 72), (2, 8192, 4), (2, 131072, 8), (16, 1600, 70)], ids=case_id)
def test_plan_restatement_matches_the_workspace_size_and_every_case_keeps_its_regime(backend, case):
    dev, lib = start(backend, torch.float32)
    B, HW, Cc = case
    p4, p8 = plan(B, HW, Cc, 4, GRID_TARGET[backend]), plan(B, HW, Cc, 8, GRID_TARGET[backend])
    assert lib.uegan_reduce_workspace_floats(B, HW, Cc) == 3 * B * Cc * max(p4["S"], p8["S"]) + 8 * B * Cc
    for p in (p4, p8):
        assert p["CG"] * p["PL"] == 256 and (p["S"] - 1) * p["chunk"] < HW <= p["S"] * p["chunk"] and 0 < p["live"] <= p["CG"]
    if case in WITNESS:
        for dtype in (torch.float32, torch.bfloat16):
            regime(backend, dtype, case)


def test_restated_plan_splits_small_maps_per_image():
    """where make_plan's comment promises a split count per image: maps of at most 4096 pixels with fewer than 8 channel groups (on the restated
    plan, no kernel runs; the kernels' side of the promise is test_image_in_a_batch_equals_the_image_alone_up_to_4096_pixels)"""
    for target in GRID_TARGET.values():
        for epc in (4, 8):
            for HW in list(range(1, 4097, 7)) + [256, 1024, 2048, 4095, 4096]:
                for Cc in (3, 5, 8, 32, 64, 70, 72, 256, 512, 520, 1024):
                    ps = [plan(B, HW, Cc, epc, target) for B in (1, 2, 3, 8, 64, 512)]
                    assert ps[0]["ncg"] >= 8 or all(p == ps[0] for p in ps), (target, epc, HW, Cc)


# --------------------------------------------------------------------------------------------------------------------
# plumbing: operands, guarded workspaces, sentinel-filled outputs
# --------------------------------------------------------------------------------------------------------------------
class Workspace:
    """exactly n floats of NaN between two guard bands"""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD_N,), GUARD, dtype=torch.float32, device=dev)
        self.ws = self.buf[GUARD_N:GUARD_N + n]
        self.ws.fill_(NAN)

    def ptr(self):
        return self.ws.data_ptr()

    def intact(self):
        assert bool((self.buf[:GUARD_N] == GUARD).all()) and bool((self.buf[GUARD_N + self.n:] == GUARD).all())


def fresh(shape, dtype, dev):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def written(*ts):
    for t in ts:
        t = t.float()
        assert not bool(torch.isnan(t).any()) and not bool((t == SENT).any())


def seed_of(case, salt):
    B, HW, Cc = case
    return 1000 * salt + (7 * B + 3 * HW + Cc) % 997


def draw(case, dtype, salt, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed_of(case, salt))
    return half_round(torch.randn(*case, generator=g) * scale + shift, dtype)


def stats64(x):
    """[B, HW, C] float64 -> mean, biased variance, each [B, C]"""
    m = x.mean(1)
    return m, ((x - m[:, None]) ** 2).mean(1)


def in64(x):
    m, v = stats64(x)
    r = 1 / torch.sqrt(v + EPS)
    return (x - m[:, None]) * r[:, None], m, v, r


@functools.lru_cache(maxsize=None)
def instnorm_case(case, dtype):
    """operands (fp32 tensors holding storage-rounded values) and the float64 reference of one case, computed once"""
    x, dy = draw(case, dtype, 1, 2.0, 3.0), draw(case, dtype, 2)
    x64 = x.double().requires_grad_(True)
    y64, m, v, r = in64(x64)
    (dx64,) = torch.autograd.grad((y64 * dy.double()).sum(), x64)
    y64, m, v, r = y64.detach(), m.detach(), v.detach(), r.detach()
    # the operands of the direct calls: moments rounded to fp32, y rounded to the storage type
    m32, r32 = m.float(), r.float()
    y_apply = (x.double() - m32.double()[:, None]) * r32.double()[:, None]
    y_in = half_round(y64.float(), dtype)
    d64, yi64 = dy.double(), y_in.double()
    dx_direct = r32.double()[:, None] * (d64 - d64.mean(1, keepdim=True) - yi64 * (d64 * yi64).mean(1, keepdim=True))
    return dict(x=x, dy=dy, y=y64, mean=m, var=v, rstd=r, dx=dx64, m32=m32, r32=r32, y_apply=y_apply, y_in=y_in, dx_direct=dx_direct)


def grad_tol(dtype):
    return 5 * storage_tol(dtype)


# --------------------------------------------------------------------------------------------------------------------
# moments, InstanceNorm forward / apply / backward by direct call
# --------------------------------------------------------------------------------------------------------------------
def run_instnorm_direct(backend, dtype, case):
    dev, lib = start(backend, dtype, case)
    B, HW, Cc = case
    R = instnorm_case(case, dtype)
    tag, tol = case_id(case), storage_tol(dtype)
    xd, dyd = R["x"].to(dtype).to(dev), R["dy"].to(dtype).to(dev)
    dt = ops._dt(xd)
    n = lib.uegan_reduce_workspace_floats(B, HW, Cc)
    out = {}
    # uegan_moments: mean and the biased variance itself
    ws, mean, var = Workspace(n, dev), fresh((B, Cc), torch.float32, dev), fresh((B, Cc), torch.float32, dev)
    _lib.check(lib.uegan_moments(dt, xd.data_ptr(), mean.data_ptr(), var.data_ptr(), ws.ptr(), B, HW, Cc, None))
    ws.intact()
    written(mean, var)
    held(fam("moments", dtype), backend, tag + " mean", mean, R["mean"], F32_TOL)
    held(fam("moments", dtype), backend, tag + " var", var, R["var"], F32_TOL)
    out["mean"], out["var"] = mean.cpu(), var.cpu()
    # uegan_instnorm_fwd
    ws, mean, rstd, y = Workspace(n, dev), fresh((B, Cc), torch.float32, dev), fresh((B, Cc), torch.float32, dev), fresh(case, dtype, dev)
    _lib.check(lib.uegan_instnorm_fwd(dt, xd.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.ptr(), B, HW, Cc, EPS, None))
    ws.intact()
    written(mean, rstd, y)
    held(fam("instnorm", dtype), backend, tag + " fwd mean", mean, R["mean"], F32_TOL)
    held(fam("instnorm", dtype), backend, tag + " fwd rstd", rstd, R["rstd"], F32_TOL)
    held(fam("instnorm", dtype), backend, tag + " fwd y", y, R["y"], tol)
    out["fwd_mean"], out["fwd_rstd"], out["fwd_y"] = mean.cpu(), rstd.cpu(), y.cpu()
    # uegan_instnorm_apply on given moments
    y2 = fresh(case, dtype, dev)
    m32, r32 = R["m32"].to(dev), R["r32"].to(dev)
    _lib.check(lib.uegan_instnorm_apply(dt, xd.data_ptr(), y2.data_ptr(), m32.data_ptr(), r32.data_ptr(), B, HW, Cc, None))
    written(y2)
    held(fam("instnorm", dtype), backend, tag + " apply y", y2, R["y_apply"], tol)
    out["apply_y"] = y2.cpu()
    # uegan_instnorm_bwd on given y and rstd
    ws, dx, yin = Workspace(n, dev), fresh(case, dtype, dev), R["y_in"].to(dtype).to(dev)
    _lib.check(lib.uegan_instnorm_bwd(dt, dyd.data_ptr(), yin.data_ptr(), r32.data_ptr(), dx.data_ptr(), ws.ptr(), B, HW, Cc, None))
    ws.intact()
    written(dx)
    held(fam("instnorm", dtype), backend, tag + " bwd dx", dx, R["dx_direct"], grad_tol(dtype))
    out["bwd_dx"] = dx.cpu()
    if HW == 1:          # one pixel: x - mean and dy - mean(dy) are exactly 0
        assert bool((var == 0).all()) and bool((y.float() == 0).all()) and bool((y2.float() == 0).all()) and bool((dx.float() == 0).all())
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_moments_and_instnorm_by_direct_call(backend, dtype, case):
    run_instnorm_direct(backend, dtype, case)


def run_instnorm_ops(backend, dtype, case):
    dev, lib = start(backend, dtype, case)
    B, HW, Cc = case
    R = instnorm_case(case, dtype)
    tag = case_id(case)
    out = {}
    for how in ("computed", "given"):
        pre = None if how == "computed" else torch.stack([R["m32"], R["r32"]]).to(dev)
        xd = R["x"].to(dtype).to(dev).reshape(B, HW, 1, Cc).clone().requires_grad_(True)
        y = ops.instnorm(xd, pre)
        y.backward(R["dy"].to(dtype).to(dev).reshape(B, HW, 1, Cc))
        y, dx = y.detach().reshape(case), xd.grad.reshape(case)
        written(y, dx)
        held(fam("instnorm", dtype), backend, "%s ops(%s) y" % (tag, how), y, R["y"], storage_tol(dtype))
        held(fam("instnorm", dtype), backend, "%s ops(%s) dx" % (tag, how), dx, R["dx"], grad_tol(dtype))
        if HW == 1:
            assert bool((y.float() == 0).all()) and bool((dx.float() == 0).all())
        out[how + "_y"], out[how + "_dx"] = y.cpu(), dx.cpu()
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_instnorm_through_ops_with_computed_and_given_moments(backend, dtype, case):
    run_instnorm_ops(backend, dtype, case)


# --------------------------------------------------------------------------------------------------------------------
# InstanceNorm of a hi + lo pair of 16-bit planes
# --------------------------------------------------------------------------------------------------------------------
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def run_instnorm_pair(backend, dtype, case):
    dev, lib = start(backend, dtype, case)
    B, HW, Cc = case
    tag = case_id(case)
    g = torch.Generator().manual_seed(seed_of(case, 3))
    v = torch.randn(*case, generator=g) * 2 + 3
    hi = half_round(v, dtype)
    lo = half_round(v - hi, dtype)
    val = hi.double() + lo.double()
    _, m, _, r = in64(val)
    m32, r32 = m.float(), r.float()
    ref = (val - m32.double()[:, None]) * r32.double()[:, None]           # the value the kernel is given, on the moments it is given
    pre = torch.stack([m32, r32]).to(dev)
    y, ylo = ops.instnorm_pair(hi.to(dtype).to(dev).reshape(B, HW, 1, Cc), lo.to(dtype).to(dev).reshape(B, HW, 1, Cc), pre)
    y, ylo = y.detach().reshape(case).cpu(), ylo.reshape(case).cpu()
    written(y, ylo)
    # the hi plane is the storage rounding of the fp32 result, the lo plane the remainder rounded once more: hi + lo carries u^2
    held(fam("instnorm_pair", dtype), backend, tag + " hi", y, half_round(ref.float(), dtype), storage_tol(dtype))
    held(fam("instnorm_pair", dtype), backend, tag + " hi vs fp64", y, ref, storage_tol(dtype))
    e = float((y.double() + ylo.double() - ref).abs().max() / (ref.abs().max() + 1e-12))
    tol = F32_TOL + UNIT_ROUNDOFF[dtype] ** 2
    print("OBS|%s|%s|%s hi+lo|%.3e|%.1e" % (fam("instnorm_pair", dtype), backend, tag, e, tol))
    assert e < tol, (case, e, tol)
    return {"hi": y, "lo": ylo}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES[1:], ids=DTYPE_IDS[1:])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_instnorm_of_a_hi_lo_pair(backend, dtype, case):
    run_instnorm_pair(backend, dtype, case)


# --------------------------------------------------------------------------------------------------------------------
# affine normalisation + activation on explicit coefficients
# --------------------------------------------------------------------------------------------------------------------
ACTS = sorted(variants.ACT_CODES.items(), key=lambda kv: kv[1])


def act64(code, pre):
    if code == ops.ACT_LRELU:
        return F.leaky_relu(pre, 0.2)
    if code == ops.ACT_RELU:
        return F.relu(pre)
    if code == variants.ACT_SWISH:
        return pre * torch.sigmoid(pre)
    if code == variants.ACT_SELU:
        return F.selu(pre)
    assert code == ops.ACT_NONE
    return pre * 1.0


@functools.lru_cache(maxsize=None)
def affine_operands(case, dtype):
    """x, gy (storage-rounded) and per-(b, c) coefficients; ReLU, LeakyReLU and the derivative of SELU jump at 0, so x is resampled until the
    float64 pre-activation is MARGIN away from 0 with the coefficients (x * scale + shift) and without them (x itself)"""
    B, HW, Cc = case
    g = torch.Generator().manual_seed(seed_of(case, 4))
    coef = {k: torch.randn(B, Cc, generator=g) for k in ("shift", "ca", "cb", "cc")}
    coef["scale"] = (0.5 + torch.rand(B, Cc, generator=g)) * torch.where(torch.rand(B, Cc, generator=g) < 0.25, -1.0, 1.0)
    x = half_round(torch.randn(*case, generator=g) * 1.5 + 0.5, dtype)
    gy = half_round(torch.randn(*case, generator=g) + 0.25, dtype)
    for _ in range(50):
        bad = affine_band(x, coef)
        if not bool(bad.any()):
            break
        x[bad] = half_round(torch.randn(int(bad.sum()), generator=g) * 1.5 + 0.5, dtype)
    return x, gy, coef


def affine_band(x, coef):
    x64 = x.double()
    pre = x64 * coef["scale"].double()[:, None] + coef["shift"].double()[:, None]
    return (pre.abs() < MARGIN) | (x64.abs() < MARGIN)


def affine_ref(code, x, gy, coef):
    """float64: y, sums [B, C, 2] = {sum g, sum g * x}, gx = g * ca + x * cb + cc with g = gy * act'(x * scale + shift); NULL = 1 / 0 / 1 / 0 / 0"""
    x64, one = x.double(), torch.ones(x.shape[0], x.shape[2], dtype=torch.float64)
    k = {n: (coef[n].double() if coef else (one if n in ("scale", "ca") else 0 * one))[:, None] for n in ("scale", "shift", "ca", "cb", "cc")}
    pre = (x64 * k["scale"] + k["shift"]).requires_grad_(True)
    y = act64(code, pre)
    (gpre,) = torch.autograd.grad(y, pre, gy.double())
    return y.detach(), torch.stack([gpre.sum(1), (gpre * x64).sum(1)], -1), gpre * k["ca"] + x64 * k["cb"] + k["cc"]


def call_affine(lib, dev, dtype, code, x, gy, coef, case):
    """the three entry points on sentinel-filled outputs and a guarded workspace -> y, sums, gx"""
    B, HW, Cc = case
    xd, gyd = x.to(dtype).to(dev), gy.to(dtype).to(dev)
    dt = ops._dt(xd)
    cd = {n: t.to(dev) for n, t in coef.items()} if coef else {}
    P = lambda n: cd[n].data_ptr() if coef else None       # noqa: E731
    y, gx, sums = fresh(case, dtype, dev), fresh(case, dtype, dev), fresh((B, Cc, 2), torch.float32, dev)
    ws = Workspace(lib.uegan_reduce_workspace_floats(B, HW, Cc), dev)
    _lib.check(lib.uegan_affine_act_fwd(dt, code, xd.data_ptr(), P("scale"), P("shift"), y.data_ptr(), B, HW, Cc, None))
    _lib.check(lib.uegan_affine_act_bwd_sums(dt, code, gyd.data_ptr(), xd.data_ptr(), P("scale"), P("shift"), sums.data_ptr(), ws.ptr(), B, HW, Cc, None))
    _lib.check(lib.uegan_affine_act_bwd_apply(dt, code, gyd.data_ptr(), xd.data_ptr(), P("scale"), P("shift"), P("ca"), P("cb"), P("cc"), gx.data_ptr(),
                                              B, HW, Cc, None))
    ws.intact()
    written(y, sums, gx)
    return y.cpu(), sums.cpu(), gx.cpu()


def run_affine(backend, dtype, case, acts=ACTS):
    dev, lib = start(backend, dtype, case)
    x, gy, coef = affine_operands(case, dtype)
    assert not bool(affine_band(x, coef).any())              # the margin holds before a kernel sees the data; no element is left out below
    tag, out = case_id(case), {}
    for name, code in acts:
        for how, cf in (("coef", coef), ("null", None)):
            yr, sr, gr = affine_ref(code, x, gy, cf)
            y, sums, gx = call_affine(lib, dev, dtype, code, x, gy, cf, case)
            what = "%s %s %s" % (tag, name, how)
            held(fam("affine_act", dtype), backend, what + " y", y, yr, storage_tol(dtype))
            held(fam("affine_act", dtype), backend, what + " sums", sums, sr, F32_TOL)
            held(fam("affine_act", dtype), backend, what + " gx", gx, gr, storage_tol(dtype))
            out.update({what + " y": y, what + " sums": sums, what + " gx": gx})
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_affine_act_every_activation_with_and_without_coefficients(backend, dtype, case):
    run_affine(backend, dtype, case)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_affine_act_tie_follows_torch(backend, dtype):
    """x * scale + shift = 0 exactly (dyadic x, scale 2, shift -1; with NULL coefficients x = 0): torch takes the negative side's slope at 0
    (relu' = 0, leaky_relu' = 0.2, selu' = scale * alpha), and so must the kernels.  ReLU is compared bit for bit (every value is dyadic), the
    others to the storage tolerance ELEMENT-wise on the ties -- the other side's slope is 5 x / 0.6 x as large."""
    dev, lib = start(backend, dtype)
    case = (2, 48, 8)
    g = torch.Generator().manual_seed(6)
    vals = torch.tensor([0.5, 0.5, 0.0, -1.0, 1.0, 0.25, -0.5, 2.0])
    x = vals[torch.randint(0, len(vals), case, generator=g)]
    gy = torch.tensor([1.0, -2.0, 0.5, 4.0])[torch.randint(0, 4, case, generator=g)]
    B, HW, Cc = case
    coef = {"scale": torch.full((B, Cc), 2.0), "shift": torch.full((B, Cc), -1.0), "ca": torch.ones(B, Cc), "cb": torch.zeros(B, Cc),
            "cc": torch.zeros(B, Cc)}
    for how, cf, tie in (("coef", coef, x == 0.5), ("null", None, x == 0.0)):
        assert int(tie.sum()) > 50
        for name, code in ACTS:
            yr, sr, gr = affine_ref(code, x, gy, cf)
            y, sums, gx = call_affine(lib, dev, dtype, code, x, gy, cf, case)
            assert bool((y.float()[tie] == 0).all())
            if name in ("ReLU", "none"):
                assert torch.equal(y.float(), yr.float()) and torch.equal(gx.float(), gr.float()) and torch.equal(sums, sr.float())
                assert name == "none" or bool((gx.float()[tie] == 0).all())
            else:
                assert bool(((gx.double()[tie] - gr[tie]).abs() <= storage_tol(dtype) * gr[tie].abs()).all()), (name, how)
                held(fam("affine_act", dtype), backend, "tie %s %s gx" % (name, how), gx, gr, storage_tol(dtype))
                held(fam("affine_act", dtype), backend, "tie %s %s sums" % (name, how), sums, sr, F32_TOL)


# --------------------------------------------------------------------------------------------------------------------
# the fidelity-loss tap: weight * MSE(IN(x), IN(y)) and its gradient forms
# --------------------------------------------------------------------------------------------------------------------
TAP_WEIGHT = 0.7
LOSS0 = 1.25             # what the loss cell holds before the second forward: the kernels accumulate into it


def tap_operands(case, dtype):
    """x has exact zeros and both signs (the act forms mask on x > 0); y is another distribution"""
    g = torch.Generator().manual_seed(seed_of(case, 5))
    x = half_round(torch.randn(*case, generator=g) * 1.5 + 0.5, dtype)
    x[torch.rand(case, generator=g) < 0.05] = 0.0
    y = half_round(torch.randn(*case, generator=g) * 1.5 + 1.0, dtype)
    g0 = half_round(torch.randn(*case, generator=g), dtype)       # what gx holds before the accumulating form runs
    return x, y, g0


@functools.lru_cache(maxsize=None)
def tap_case(case, dtype, gscale):
    x, y, g0 = tap_operands(case, dtype)
    x64 = x.double().requires_grad_(True)
    xh, mx, _, rx = in64(x64)
    yh, my, _, ry = in64(y.double())
    loss = TAP_WEIGHT * ((xh - yh) ** 2).mean()
    (g,) = torch.autograd.grad(loss * gscale, x64)
    stats = [t.detach().float() for t in (mx, rx, my, ry)]
    return dict(x=x, y=y, g0=g0, loss=loss.detach(), g=g, stats=stats)


def tap_gscale(case):
    """k = 2 * weight * gscale / (B * HW * C) is 0.518 at every shape: the gradient is O(1), inside fp16's normal range"""
    B, HW, Cc = case
    return 0.37 * B * HW * Cc


def out_act_grad(code, x64):
    """derivative of the producer's activation read off its OUTPUT x (common.h: act_grad_from_out)"""
    if code == ops.ACT_RELU:
        return (x64 > 0).double()
    if code == ops.ACT_LRELU:
        return torch.where(x64 > 0, 1.0, 0.2).double()
    assert code == ops.ACT_NONE
    return torch.ones_like(x64)


def tap_forward(lib, dev, dtype, case, x, y, stats=None, loss0=0.0):
    """uegan_percep_tap_fwd (or _fwd_given on `stats`) on a guarded NaN workspace of 3 reduction workspaces -> loss cell, workspace"""
    B, HW, Cc = case
    ws = Workspace(3 * lib.uegan_reduce_workspace_floats(B, HW, Cc), dev)
    loss = torch.full((1,), loss0, dtype=torch.float32, device=dev)
    dt = ops._dt(x)
    if stats is None:
        _lib.check(lib.uegan_percep_tap_fwd(dt, x.data_ptr(), y.data_ptr(), TAP_WEIGHT, loss.data_ptr(), ws.ptr(), B, HW, Cc, EPS, None))
    else:
        st = [t.to(dev) for t in stats]
        _lib.check(lib.uegan_percep_tap_fwd_given(dt, x.data_ptr(), y.data_ptr(), TAP_WEIGHT, loss.data_ptr(), ws.ptr(), B, HW, Cc, st[0].data_ptr(),
                                                  st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), None))
    ws.intact()
    return loss, ws


def tap_backward(lib, dev, dtype, case, x, y, ws, gscale, form, code=ops.ACT_NONE, gx=None):
    B, HW, Cc = case
    gsc = torch.tensor([gscale], dtype=torch.float32, device=dev)
    acc = gx is not None
    if gx is None:
        gx = fresh(case, dtype, dev)
    dt = ops._dt(x)
    a = (x.data_ptr(), y.data_ptr(), TAP_WEIGHT, gsc.data_ptr(), gx.data_ptr(), ws.ptr(), B, HW, Cc, EPS)
    if form == "bwd":
        _lib.check(lib.uegan_percep_tap_bwd(dt, *a, None))
    elif form == "bwd_act":
        _lib.check(lib.uegan_percep_tap_bwd_act(dt, code, *a, None))
    else:
        _lib.check(lib.uegan_percep_tap_bwd_acc(dt, code, *a, 1 if acc else 0, None))
    ws.intact()
    written(gx)
    return gx


def run_tap(backend, dtype, case):
    dev, lib = start(backend, dtype, case)
    B, HW, Cc = case
    gscale = tap_gscale(case)
    R = tap_case(case, dtype, gscale)
    gmax = float(R["g"].abs().max())
    assert gmax >= 2.0 ** -10 or HW == 1, gmax               # (one pixel: IN(x) = IN(y) = 0, the loss and its gradient are exactly 0)
    tag, tol, fm = case_id(case), storage_tol(dtype), fam("percep_tap", dtype)
    xd, yd = R["x"].to(dtype).to(dev), R["y"].to(dtype).to(dev)
    x64 = R["x"].double()
    out = {}
    loss, ws = tap_forward(lib, dev, dtype, case, xd, yd)
    held_scalar(fm, backend, tag + " loss", loss, R["loss"], F32_TOL)
    # the forms of the gradient, each from the forward's workspace
    gx = tap_backward(lib, dev, dtype, case, xd, yd, ws, gscale, "bwd")
    held(fm, backend, tag + " bwd gx", gx, R["g"], tol)
    out["loss"], out["bwd"] = loss.cpu(), gx.cpu()
    for name, code in (("relu", ops.ACT_RELU), ("lrelu", ops.ACT_LRELU)):
        ref = R["g"] * out_act_grad(code, x64)
        ga = tap_backward(lib, dev, dtype, case, xd, yd, ws, gscale, "bwd_act", code)
        held(fm, backend, "%s bwd_act(%s) gx" % (tag, name), ga, ref, tol)
        assert bool((ga.float().cpu()[x64 <= 0] == 0).all()) or code != ops.ACT_RELU
        g0 = R["g0"].to(dtype).to(dev)
        gacc = tap_backward(lib, dev, dtype, case, xd, yd, ws, gscale, "bwd_acc", code, gx=g0.clone())
        held(fm, backend, "%s bwd_acc(%s) gx vs fp64" % (tag, name), gacc, ref + R["g0"].double(), tol)
        held(fm, backend, "%s bwd_acc(%s) gx vs prefill + bwd_act" % (tag, name), gacc, ga.double().cpu() + R["g0"].double(), tol)
        gset = tap_backward(lib, dev, dtype, case, xd, yd, ws, gscale, "bwd_acc", code)       # accumulate = 0: the same as _bwd_act, to the bit
        assert torch.equal(gset, ga)
        out.update({name + " act": ga.cpu(), name + " acc": gacc.cpu()})
    # the float64-correct statistics, rounded to fp32, give the same loss -- added to what the cell held -- and the same gradient
    loss2, ws2 = tap_forward(lib, dev, dtype, case, xd, yd, stats=R["stats"], loss0=LOSS0)
    held_scalar(fm, backend, tag + " fwd_given loss + preset", loss2, LOSS0 + R["loss"], F32_TOL)
    gx2 = tap_backward(lib, dev, dtype, case, xd, yd, ws2, gscale, "bwd")
    held(fm, backend, tag + " bwd gx after fwd_given", gx2, R["g"], tol)
    loss3, _ = tap_forward(lib, dev, dtype, case, xd, yd, loss0=LOSS0)
    held_scalar(fm, backend, tag + " loss + preset", loss3, LOSS0 + R["loss"], F32_TOL)
    out.update({"loss_given": loss2.cpu(), "bwd_given": gx2.cpu(), "loss_preset": loss3.cpu()})
    if HW == 1:
        assert float(loss) == 0 and float(loss2) == LOSS0 and all(bool((t.float() == 0).all()) for k, t in out.items() if k.startswith("bwd"))
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_percep_tap_loss_and_every_gradient_form(backend, dtype, case):
    run_tap(backend, dtype, case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_percep_tap_fp16_gradient_without_loss_scale_rounds_to_subnormals(backend):
    """FINDING: at (2, 1000, 520) with gscale 0.37 the tap gradient is about 1e-7, in fp16's subnormal range (step 2^-24 =
    6e-8), and is off by 2.5e-2 of the tensor's maximum against float64 (F16_TOL: 3e-3) -- through the format alone: every element is within
    one fp16 ulp (one subnormal step there) of the float64 gradient rounded to fp16, which is what is asserted.  Trainer(loss_scale=...)
    exists for this; with an O(1) gradient (test_percep_tap_loss_and_every_gradient_form) fp16 holds F16_TOL at every shape."""
    dtype, case, gscale = torch.float16, (2, 1000, 520), 0.37
    dev, lib = start(backend, dtype, case)
    R = tap_case(case, dtype, gscale)
    xd, yd = R["x"].to(dtype).to(dev), R["y"].to(dtype).to(dev)
    assert float(R["g"].abs().max()) < 2.0 ** -14            # the whole tensor is subnormal in fp16
    loss, ws = tap_forward(lib, dev, dtype, case, xd, yd)
    held_scalar(fam("percep_tap unscaled", dtype), backend, case_id(case) + " loss", loss, R["loss"], F32_TOL)
    for form, code in (("bwd", ops.ACT_NONE), ("bwd_act", ops.ACT_RELU)):
        ref = R["g"] * out_act_grad(code, R["x"].double())
        r16 = ref.to(torch.float16).double()
        got = tap_backward(lib, dev, dtype, case, xd, yd, ws, gscale, form, code).cpu()
        print("OBS|%s|%s|%s %s gx|%.3e|%.0e" % (fam("percep_tap unscaled", dtype), backend, case_id(case), form, rel(got, ref), storage_tol(dtype)))
        ulp = torch.clamp(2.0 ** (torch.floor(torch.log2(r16.abs().clamp_min(2.0 ** -30))) - 10), min=2.0 ** -24)
        assert bool(((got.double() - r16).abs() <= ulp).all())


# --------------------------------------------------------------------------------------------------------------------
# "the variance never suffers E[x^2] - E[x]^2 cancellation"
# --------------------------------------------------------------------------------------------------------------------
CANCEL_CASES = [(1, 9, 64), (2, 48, 5), (1, 1600, 70), (1, 2500, 40), (2, 1000, 520), (1, 66000, 8)]
CANCEL_MEAN = 100.0
CANCEL_SIGMA = {torch.float32: 0.1, torch.bfloat16: 0.5, torch.float16: 0.5}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CANCEL_CASES, ids=case_id)
def test_variance_of_data_far_from_zero_has_no_cancellation(backend, dtype, case):
    """Data at mean 100 with sigma 0.1 (fp32) / 0.5 (16-bit storage).  Bound on the relative error of a channel's variance: 8 * 2^-23 * |mean| / sigma
    -- the dominant term is the fp32 rounding of a partial mean (half an ulp of |mean|, 2^-24 |mean|), which enters a Chan merge as d^2 with
    d ~ sigma, i.e. 2 * 2^-24 * |mean| / sigma relative to sigma^2 per merge level; the factor 8 covers the depth of the merges.  The naive fp32
    formula on the same data (plain PyTorch; also with its sums taken exactly) must miss 10 x that bound, so the case separates the two algorithms."""
    dev, lib = start(backend, dtype, case)
    B, HW, Cc = case
    sigma = CANCEL_SIGMA[dtype]
    bound = 8 * 2.0 ** -23 * CANCEL_MEAN / sigma
    x = draw(case, dtype, 7, sigma, CANCEL_MEAN)
    m, v = stats64(x.double())
    assert float(v.min()) > 0
    naive = ((x * x).mean(1) - x.mean(1) ** 2).double()
    e_naive = float(((naive - v).abs() / v).max())
    # ... and the kindest fp32 evaluation of that formula: exact sums, only x * x, E[x^2] and E[x] rounded to fp32 (independent of torch's summation order)
    ex2, ex = (x * x).double().mean(1).float(), x.double().mean(1).float()
    e_kind = float((((ex2 - ex * ex).double() - v).abs() / v).max())
    xd = x.to(dtype).to(dev)
    ws = Workspace(lib.uegan_reduce_workspace_floats(B, HW, Cc), dev)
    mean, var = fresh((B, Cc), torch.float32, dev), fresh((B, Cc), torch.float32, dev)
    _lib.check(lib.uegan_moments(ops._dt(xd), xd.data_ptr(), mean.data_ptr(), var.data_ptr(), ws.ptr(), B, HW, Cc, None))
    ws.intact()
    written(mean, var)
    e = float(((var.double().cpu() - v).abs() / v).max())
    print("OBS|%s|%s|%s var, per channel (must EXCEED 10 x the bound)|%.3e|%.1e" % (fam("naive E[x^2]-E[x]^2 in fp32", dtype), backend, case_id(case), e_naive, bound))
    print("OBS|%s|%s|%s var, per channel|%.3e|%.1e" % (fam("moments cancellation", dtype), backend, case_id(case), e, bound))
    print("OBS|%s|%s|%s var, per channel, sums exact (must EXCEED 10 x the bound)|%.3e|%.1e" % (fam("naive E[x^2]-E[x]^2 in fp32", dtype), backend, case_id(case), e_kind,
                                                                                                  bound))
    assert e_naive > 10 * bound and e_kind > 10 * bound, (e_naive, e_kind, bound)
    assert e < bound, (e, bound)
    held(fam("moments cancellation", dtype), backend, case_id(case) + " mean", mean, m, F32_TOL)


# --------------------------------------------------------------------------------------------------------------------
# batch composition
# --------------------------------------------------------------------------------------------------------------------
def instnorm_fwd_bwd(lib, dev, dtype, x, dy):
    """uegan_instnorm_fwd then _bwd on the y it wrote -> mean, rstd, y, dx"""
    B, HW, Cc = x.shape
    xd, dyd = x.to(dtype).to(dev), dy.to(dtype).to(dev)
    dt = ops._dt(xd)
    n = lib.uegan_reduce_workspace_floats(B, HW, Cc)
    ws, mean, rstd = Workspace(n, dev), fresh((B, Cc), torch.float32, dev), fresh((B, Cc), torch.float32, dev)
    y, dx = fresh(tuple(x.shape), dtype, dev), fresh(tuple(x.shape), dtype, dev)
    _lib.check(lib.uegan_instnorm_fwd(dt, xd.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.ptr(), B, HW, Cc, EPS, None))
    ws.ws.fill_(NAN)
    _lib.check(lib.uegan_instnorm_bwd(dt, dyd.data_ptr(), y.data_ptr(), rstd.data_ptr(), dx.data_ptr(), ws.ptr(), B, HW, Cc, None))
    ws.intact()
    written(mean, rstd, y, dx)
    return mean.cpu(), rstd.cpu(), y.cpu(), dx.cpu()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("hwc", [(4096, 8), (1024, 72)], ids=lambda s: "%dx%d" % s)
def test_image_in_a_batch_equals_the_image_alone_up_to_4096_pixels(backend, dtype, hwc):
    """what make_plan promises for maps of at most 4096 pixels: the split count does not depend on how many images share the launch, so an
    image's statistics, y and dx are the same bits alone and as image 0 of three"""
    dev, lib = start(backend, dtype)
    p3, p1 = plan_of(backend, dtype, (3,) + hwc), plan_of(backend, dtype, (1,) + hwc)
    assert p3 == p1 and hwc[0] <= 4096
    x, dy = draw((3,) + hwc, dtype, 8, 2.0, 3.0), draw((3,) + hwc, dtype, 9)
    together = instnorm_fwd_bwd(lib, dev, dtype, x, dy)
    alone = instnorm_fwd_bwd(lib, dev, dtype, x[:1], dy[:1])
    for a, b in zip(together, alone):
        assert torch.equal(a[:1], b)


ABOVE_RANGE = {"emu": (8192, 4), "gpu": (131072, 8)}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_image_in_a_batch_agrees_with_the_image_alone_above_4096_pixels(backend, dtype):
    """FINDING: above 4096 pixels the split count follows B * ncg (make_plan's first grow loop and `cap`), so the two launches
    sum in different orders: the results agree to the kernels' tolerances; neither bit equality nor inequality is promised or asserted."""
    dev, lib = start(backend, dtype)
    hwc = ABOVE_RANGE[backend]
    p2, p1 = plan_of(backend, dtype, (2,) + hwc), plan_of(backend, dtype, (1,) + hwc)
    assert p2["S"] != p1["S"], (p1, p2)
    x, dy = draw((2,) + hwc, dtype, 10, 2.0, 3.0), draw((2,) + hwc, dtype, 11)
    together = instnorm_fwd_bwd(lib, dev, dtype, x, dy)
    alone = instnorm_fwd_bwd(lib, dev, dtype, x[:1], dy[:1])
    tag = "B=1 vs B=2 %dx%d" % hwc
    for name, a, b, tol in zip(("mean", "rstd", "y", "dx"), together, alone, (F32_TOL, F32_TOL, storage_tol(dtype), grad_tol(dtype))):
        held(fam("instnorm batch composition", dtype), backend, "%s %s" % (tag, name), a[:1], b, tol)


# --------------------------------------------------------------------------------------------------------------------
# repeatability: fixed-order merges and finalize
# --------------------------------------------------------------------------------------------------------------------
FAMILIES = {"instnorm_direct": run_instnorm_direct, "instnorm_ops": run_instnorm_ops, "instnorm_pair": run_instnorm_pair, "affine_act": run_affine,
            "percep_tap": run_tap}
# (hi + lo pairs exist for the 16-bit storage formats only)
REPEATS = [(f, d) for f in FAMILIES for d in DTYPES if not (f == "instnorm_pair" and d == torch.float32)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", [(1, 2500, 40), (1, 131072, 8)], ids=case_id)
@pytest.mark.parametrize("family_dtype", REPEATS, ids=lambda fd: "%s-%s" % (fd[0], DTYPE_IDS[DTYPES.index(fd[1])]))
def test_two_identical_calls_give_identical_bits(backend, case, family_dtype):
    """no atomics anywhere: block trees, the per-lane merge and the butterfly of the finalize wave all run in a fixed order (S = 93: a partial second
    trip; S = 1024 on the device: 16 partials per lane)"""
    family, dtype = family_dtype
    a = FAMILIES[family](backend, dtype, case)
    b = FAMILIES[family](backend, dtype, case)
    assert a.keys() == b.keys() and len(a) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
