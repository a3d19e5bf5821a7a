"""Kernel-level parity of everything between the discriminator's maps and the optimizer step, in every launch regime:

* the relativistic losses (`ops.rahinge`, `variants.rals`) and the one-list terms (`variants.pred_loss`)          -- loss.hip
* the head-map form of the relativistic hinge (`uegan_rahinge_heads_fwd / _bwd`, fp32 / bf16 / fp16 storage)     -- loss.hip
* the multiscale reconstruction loss (`ops.multiscale_rec`)                                                      -- loss.hip
* the spectral-norm power iteration and gradient (`uegan_specnorm_*`)                                            -- optim_sn.hip
* `uegan_sn_act_bwd` -> `uegan_sn_grad_finish` (unpadded form; the padded form keeps its test in test_ops.py)    -- act_bwd.hip
* the multi-tensor Adam / RMSprop steps (`ops.FusedAdamL2`, `variants.FusedRMSprop`)                             -- optim_sn.hip

Every reference is a few lines of plain PyTorch in float64 on the kernel's own operands (rounded to the storage type first where
the storage is 16-bit), written from the reference's formulas (losses.py:219-231, 312-409; torch spectral_norm / Adam / RMSprop);
none goes through a kernel or through `ops`.  The sizes are taken from the launchers' constants (named next to each case list) so
that every block cap, fixed-order fold and grid-stride loop runs with more work than one pass holds.

Tolerances are test_ops.py's: what a kernel keeps in fp32 (losses, sigma, u, v, dw, db, optimizer state) is held to F32_TOL whatever
the storage type, a tensor stored in 16 bits to BF16_TOL / F16_TOL; per tensor, max-abs error over max-abs reference (helpers.rel).
Structurally zero or untouched regions are asserted exactly.

The hinge and (smooth-)L1 gradients jump at a threshold.  Random inputs are therefore built so that the fp64 reference sees every
such argument at least MARGIN away from its threshold (the offending elements are resampled and the margin is asserted before the
kernel runs; no element is left out of a comparison), and the ties themselves are tested with dyadic values whose sums are exact
in fp32, bit for bit against torch's convention.

Where a test owns a workspace it fills it with NaN (the contracts promise that no zero-initialisation is needed) and every output
buffer with a sentinel; the autograd wrappers allocate theirs themselves.  Each comparison prints an `OBS|family|backend|what|error|
tolerance` line (pytest -rP shows them): DESIGN.md section 4 records the largest per family and backend.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from helpers import BACKENDS, half_round, rel, use_backend
from test_ops import BF16_TOL, F16_TOL, F32_TOL
from uegan_amd import _lib, ops, variants

GPU_ONLY = BACKENDS[1:]
NAN = float("nan")
SENT = 3.0               # sentinel of the output buffers (exact in every storage type)
MARGIN = 1e-4            # > 20 x the worst fp32 error of a mean over these sizes
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DTYPE_IDS = ["f32", "bf16", "f16"]


def storage_tol(dtype):
    return {torch.float32: F32_TOL, torch.bfloat16: BF16_TOL, torch.float16: F16_TOL}[dtype]


def held(family, backend, what, got, ref, tol):
    e = rel(got, ref)
    print("OBS|%s|%s|%s|%.3e|%.0e" % (family, backend, what, e, tol))
    assert e < tol, (family, what, e, tol)


def held_scalar(family, backend, what, got, ref, tol):
    e = abs(float(got) - float(ref)) / (abs(float(ref)) + 1e-12)
    print("OBS|%s|%s|%s|%.3e|%.0e" % (family, backend, what, e, tol))
    assert e < tol, (family, what, float(got), float(ref), e, tol)


# --------------------------------------------------------------------------------------------------------------------
# relativistic losses: rahinge / rals (losses.py:348-376, summed over the scales :393-409)
# --------------------------------------------------------------------------------------------------------------------
# loss.hip: RB = 64 block partials per scale and quantity, 256 threads x 4 = 1024 elements per block (ra_fill: nbx = min(RB,
# ceil(max n / 1024))); the gradient kernel caps at 256 blocks.  8 192 -> 8 partials, 65 536 -> 64, 65 537 -> 64 and a second trip of
# the grid-stride loop, 300 000 -> several trips of the reduction and of the gradient kernel.
RA_SIZES = [1, 700, 8192, 65536, 65537, 300000]
RA_FIVE_SCALES = [300000, 1, 700, 65537, 8192]        # one call: the block count follows the largest, the others' blocks run dry


def ref_relativistic(kind, reals, fakes, for_d):
    s = 1.0 if for_d else -1.0
    loss = 0
    for r, f in zip(reals, fakes):
        rf, fr = r - f.mean(), f - r.mean()
        if kind == "rahinge":
            loss = loss + (torch.relu(1 - s * rf).mean() + torch.relu(1 + s * fr).mean()) / 2
        else:
            loss = loss + (((rf - s) ** 2).mean() + ((fr + s) ** 2).mean()) / 2
    return loss


def hinge_band(r, f):
    """elements of r / f whose hinge argument (either direction of the loss) is within MARGIN of 0 in fp64"""
    r64, f64 = r.double(), f.double()
    rb, fb = r64.mean(), f64.mean()
    bad_r, bad_f = torch.zeros(r.shape, dtype=torch.bool), torch.zeros(f.shape, dtype=torch.bool)
    for s in (1.0, -1.0):
        bad_r |= (1 - s * (r64 - fb)).abs() < MARGIN
        bad_f |= (1 + s * (f64 - rb)).abs() < MARGIN
    return bad_r, bad_f


def relativistic_maps(sizes, seed, rnd=lambda t: t, shift=0.3):
    g = torch.Generator().manual_seed(seed)
    reals = [rnd(torch.tanh(torch.randn(n, generator=g))) for n in sizes]
    fakes = [rnd(torch.tanh(torch.randn(n, generator=g) - shift)) for n in sizes]
    for r, f in zip(reals, fakes):
        for _ in range(50):
            bad_r, bad_f = hinge_band(r, f)
            if not (bool(bad_r.any()) or bool(bad_f.any())):
                break
            r[bad_r] = rnd(torch.tanh(torch.randn(int(bad_r.sum()), generator=g)))
            f[bad_f] = rnd(torch.tanh(torch.randn(int(bad_f.sum()), generator=g) - shift))
    return reals, fakes


def run_relativistic(kind, backend, dev, reals, fakes, for_d, want, gscale, tag):
    for r, f in zip(reals, fakes):                       # the margin holds before the kernel sees the data
        bad_r, bad_f = hinge_band(r, f)
        assert kind != "rahinge" or not (bool(bad_r.any()) or bool(bad_f.any()))
    r64 = [t.double().requires_grad_("r" in want) for t in reals]
    f64 = [t.double().requires_grad_("f" in want) for t in fakes]
    leaves = (r64 if "r" in want else []) + (f64 if "f" in want else [])
    l = ref_relativistic(kind, r64, f64, for_d)
    gs = torch.autograd.grad(l * gscale, leaves)
    rd = [t.clone().to(dev).requires_grad_("r" in want) for t in reals]
    fd = [t.clone().to(dev).requires_grad_("f" in want) for t in fakes]
    fn = ops.rahinge if kind == "rahinge" else variants.rals
    l2 = fn(rd, fd, for_d)
    assert tuple(l2.shape) == (1,)
    (l2 * gscale).sum().backward()
    held_scalar(kind, backend, tag + " loss", l2, l, F32_TOL)
    got = ([t.grad for t in rd] if "r" in want else []) + ([t.grad for t in fd] if "f" in want else [])
    for i, (a, b) in enumerate(zip(got, gs)):
        held(kind, backend, "%s grad %d" % (tag, i), a, b, F32_TOL)
    for t in (fd if want == "r" else rd if want == "f" else []):
        assert t.grad is None


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["rahinge", "rals"])
@pytest.mark.parametrize("n", RA_SIZES)
def test_relativistic_loss_every_block_count(backend, kind, n):
    dev = use_backend(backend)
    reals, fakes = relativistic_maps([n], 100 + n % 97)
    for for_d in (True, False):
        run_relativistic(kind, backend, dev, reals, fakes, for_d, "rf", 0.37, "n=%d d=%d" % (n, for_d))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["rahinge", "rals"])
def test_relativistic_loss_five_uneven_scales_and_partial_gradients(backend, kind):
    dev = use_backend(backend)
    reals, fakes = relativistic_maps(RA_FIVE_SCALES, 11)
    for for_d in (True, False):
        for want, gscale in (("rf", 1.0), ("r", -2.5), ("f", 0.37)):       # both lists, only the real lists, only the fake lists
            run_relativistic(kind, backend, dev, reals, fakes, for_d, want, gscale, "5 scales d=%d %s" % (for_d, want))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", [4096, 131072])
def test_rahinge_tie_takes_relu_zero_gradient(backend, n):
    """A = 0 (or B = 0) exactly: one map constant, the other made of dyadic values, so both means and every hinge argument are exact in
    fp32.  torch's relu has gradient 0 at 0; every factor of the gradient is a power of two here, so the comparison is bit for bit."""
    dev = use_backend(backend)
    pat = torch.tensor([0.5, 0.25, -0.75, 0.5]).repeat(n // 4)            # mean 0.125; the 0.5 entries are the ties
    for for_d, tie_on_real in ((True, True), (True, False), (False, True), (False, False)):
        s = 1.0 if for_d else -1.0
        if tie_on_real:          # A = 1 - s (r - fbar) = 0 at r = s / 2 with fbar = -s / 2
            real, fake = s * pat, torch.full((n,), -0.5 * s)
        else:                    # B = 1 + s (f - rbar) = 0 at f = -s / 2 with rbar = s / 2
            real, fake = torch.full((n,), 0.5 * s), -s * pat
        r64, f64 = real.double().requires_grad_(True), fake.double().requires_grad_(True)
        l = ref_relativistic("rahinge", [r64], [f64], for_d)
        arg = (1 - s * (r64 - f64.mean())) if tie_on_real else (1 + s * (f64 - r64.mean()))
        assert int((arg == 0).sum()) == n // 2                            # the ties are really there
        gr, gf = torch.autograd.grad(l * 0.5, [r64, f64])
        rd, fd = real.clone().to(dev).requires_grad_(True), fake.clone().to(dev).requires_grad_(True)
        l2 = ops.rahinge([rd], [fd], for_d)
        (l2 * 0.5).sum().backward()
        assert float(l2) == float(l)
        assert torch.equal(rd.grad.cpu(), gr.float()) and torch.equal(fd.grad.cpu(), gf.float())


# --------------------------------------------------------------------------------------------------------------------
# non-relativistic terms on one prediction list (losses.py:312-347, 377-392)
# --------------------------------------------------------------------------------------------------------------------
# pred_loss_fwd: bx = min(RB, ceil(max n / 1024)); pred_grad_kernel caps at 256 blocks -- the same regimes as above
PRED_TERMS = [("bce1", variants.PRED_BCE, 1.0), ("bce0", variants.PRED_BCE, 0.0), ("ls1", variants.PRED_LS, 1.0), ("ls0", variants.PRED_LS, 0.0),
              ("hinge_real", variants.PRED_HINGE_REAL, 0.0), ("hinge_fake", variants.PRED_HINGE_FAKE, 0.0),
              ("neg_mean", variants.PRED_NEG_MEAN, 0.0), ("pos_mean", variants.PRED_POS_MEAN, 0.0)]
PRED_SIZE_CASES = [[n] for n in RA_SIZES] + [RA_FIVE_SCALES]
PLANTED = [1.0, -1.0, 50.0, -50.0, 100.0, -100.0]      # the hinge terms exactly at their threshold; BCE where exp() leaves fp32's range


def ref_pred(term, target, preds):
    loss = 0
    for p in preds:
        if term == variants.PRED_BCE:
            l = F.binary_cross_entropy_with_logits(p, torch.full_like(p, target))
        elif term == variants.PRED_LS:
            l = F.mse_loss(p, torch.full_like(p, target))
        elif term == variants.PRED_HINGE_REAL:
            l = -torch.min(p - 1, torch.zeros_like(p)).mean()
        elif term == variants.PRED_HINGE_FAKE:
            l = -torch.min(-p - 1, torch.zeros_like(p)).mean()
        elif term == variants.PRED_NEG_MEAN:
            l = -p.mean()
        else:
            l = p.mean()
        loss = loss + l
    return loss


def pred_maps(sizes, seed):
    """1.5 randn (both sides of both hinge thresholds), no element within MARGIN of +-1 except the planted ones, which sit exactly ON it"""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for n in sizes:
        p = 1.5 * torch.randn(n, generator=g)
        for _ in range(50):
            bad = ((p.double().abs() - 1).abs() < MARGIN)
            if not bool(bad.any()):
                break
            p[bad] = 1.5 * torch.randn(int(bad.sum()), generator=g)
        if n >= 2 * len(PLANTED):
            p[:len(PLANTED)] = torch.tensor(PLANTED)
        ps.append(p)
    return ps


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("sizes", PRED_SIZE_CASES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("term", PRED_TERMS, ids=lambda t: t[0])
def test_pred_loss_every_term_and_block_count(backend, term, sizes):
    dev = use_backend(backend)
    name, fid, target = term
    ps = pred_maps(sizes, 7 + len(sizes))
    for p in ps:
        d = (p.double().abs() - 1).abs()
        assert bool(((d >= MARGIN) | (d == 0)).all())
    p64 = [p.double().requires_grad_(True) for p in ps]
    l = ref_pred(fid, target, p64)
    gs = torch.autograd.grad(l * 0.37, p64)
    pd = [p.clone().to(dev).requires_grad_(True) for p in ps]
    l2 = variants.pred_loss(pd, fid, target)
    assert tuple(l2.shape) == (1,)
    (l2 * 0.37).sum().backward()
    held_scalar("pred_loss", backend, name + " loss", l2, l, F32_TOL)
    for i, (a, b) in enumerate(zip(pd, gs)):
        held("pred_loss", backend, "%s grad %d" % (name, i), a.grad, b, F32_TOL)
        if fid in (variants.PRED_HINGE_REAL, variants.PRED_HINGE_FAKE) and a.numel() >= 2 * len(PLANTED):
            # the planted tie: torch.min(x, 0) hands half of the gradient to each argument where the two are equal
            tie = 0 if fid == variants.PRED_HINGE_REAL else 1
            assert float(b[tie]) != 0 and abs(float(a.grad[tie]) - float(b[tie])) < F32_TOL * abs(float(b[tie]))


# --------------------------------------------------------------------------------------------------------------------
# relativistic hinge on the batched head maps (uegan_rahinge_heads_fwd / _bwd)
# --------------------------------------------------------------------------------------------------------------------
# RH_MAXG = 4 groups, RH_MAXP = 4 pairs; forward: bx = min(RB = 64, ceil(max pixels per group / 1024)); backward: min(1024, ceil(max / 256))
# blocks.  nb = 2: 70 x 70 maps -> 9 800 pixels per group (10 partials), 200 x 170 -> 68 000 (64 partials and a second trip).
# (id, ngroups, pairs, group_mask, for_discriminator, map sizes)
HEAD_BIG = [(200, 170), (70, 70), (9, 7), (1, 1)]
HEAD_CASES = [
    ("trainer_d", 3, [(0, 1), (0, 2)], 0b111, True, HEAD_BIG),                       # trainer.py:92+95, every group's gradient
    ("trainer_g", 2, [(0, 1)], 0b10, False, HEAD_BIG),                               # trainer.py:104: only the fake group's gradient
    ("four_pairs", 4, [(0, 1), (0, 2), (3, 1), (2, 3)], 0b0101, True, [(70, 70), (3, 5)]),      # groups that are real in one pair and fake in another
    ("three_pairs", 3, [(1, 0), (2, 0), (1, 2)], 0b110, False, [(70, 70), (33, 31), (2, 2)]),
    ("one_pair_swapped", 2, [(1, 0)], 0b01, True, [(70, 70), (5, 3)]),
]


def head_gscale(dtype):
    """The factor the backward sweep starts from.  fp16 storage cannot hold the raw gradient of a mean over tens of thousands of pixels
    (0.5 / 68 000 = 7e-6 is below fp16's smallest normal number 2^-14 = 6.1e-5: half a subnormal step of 2^-24 is already 0.4 % of it), which
    is why the Trainer refuses fp16 storage without a loss scale and names 2^14; the scale reaches this kernel through gscale.  The
    unscaled fp16 gradient has its own test below."""
    return 0.37 * (2.0 ** 14 if dtype == torch.float16 else 1.0)


def run_head_case(backend, dtype, case, gscale):
    """-> per scale (gradient of the groups in the mask [live][nb][h][w][cp] as fp32, its fp64 reference [live][nb][h][w]); the loss, the
    padding channels, the groups outside the mask and the agreement with the unfused loss are asserted here"""
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    name, ng, pairs, mask, for_d, sizes = case
    nb = 2
    cp = 4 if dtype == torch.float32 else 8                  # one 16-byte chunk per pixel: channel 0 is the prediction, the rest is padding
    gen = torch.Generator().manual_seed(len(name))

    def rnd(t):
        return half_round(t, dtype)

    def draw(shape, grp):
        return rnd(torch.tanh(torch.randn(shape, generator=gen) - 0.3 * grp))

    Ps = []
    for h, w in sizes:
        P = torch.stack([draw((nb, h, w), grp) for grp in range(ng)])               # [group][nb][h][w]
        for _ in range(50):
            bad = torch.zeros(P.shape, dtype=torch.bool)
            for gr, gf in pairs:
                br, bf = hinge_band(P[gr], P[gf])
                bad[gr] |= br
                bad[gf] |= bf
            if not bool(bad.any()):
                break
            for grp in range(ng):
                P[grp][bad[grp]] = draw((int(bad[grp].sum()),), grp)
        for gr, gf in pairs:                                 # asserted before the kernel runs
            br, bf = hinge_band(P[gr], P[gf])
            assert not (bool(br.any()) or bool(bf.any()))
        Ps.append(P)
    # fp64 reference: sum over the pairs of the list loss; d loss / d(pre-tanh) = d loss / dP * (1 - P^2)
    P64 = [P.double().requires_grad_(True) for P in Ps]
    l = 0
    for gr, gf in pairs:
        l = l + ref_relativistic("rahinge", [P[gr].reshape(-1) for P in P64], [P[gf].reshape(-1) for P in P64], for_d)
    gz = [gp * (1 - P.detach() ** 2) for gp, P in zip(torch.autograd.grad(l * gscale, P64), P64)]
    # the kernel's operands: padding channels hold a non-zero value that must never be read
    maps = []
    for P in Ps:
        m = torch.full(tuple(P.reshape(ng * nb, *P.shape[2:]).shape) + (cp,), 7.0)
        m[..., 0] = P.reshape(ng * nb, *P.shape[2:])
        maps.append(m.to(dtype).to(dev).contiguous())
    ns = len(maps)
    tmp = torch.full((lib.uegan_rahinge_heads_workspace_floats(ns),), NAN, dtype=torch.float32, device=dev)
    loss = torch.full((1,), NAN, dtype=torch.float32, device=dev)
    pix = (C.c_int64 * ns)(*[h * w for h, w in sizes])
    pr = (C.c_int32 * (2 * len(pairs)))(*[v for pq in pairs for v in pq])
    tab = (C.c_void_p * ns)(*[m.data_ptr() for m in maps])
    dt = ops._dt(maps[0])
    _lib.check(lib.uegan_rahinge_heads_fwd(dt, ns, tab, pix, nb, cp, ng, len(pairs), pr, 1 if for_d else 0, loss.data_ptr(), tmp.data_ptr(), None))
    fam = "rahinge_heads " + DTYPE_IDS[DTYPES.index(dtype)]
    held_scalar(fam, backend, name + " loss", loss, l, F32_TOL)
    gmaps = [torch.full_like(m, SENT) for m in maps]
    gtab = (C.c_void_p * ns)(*[m.data_ptr() for m in gmaps])
    gsc = torch.tensor([gscale], dtype=torch.float32, device=dev)
    _lib.check(lib.uegan_rahinge_heads_bwd(dt, ns, tab, pix, nb, cp, ng, len(pairs), pr, 1 if for_d else 0, tmp.data_ptr(), gsc.data_ptr(), gtab, mask,
                                           None))
    live = [grp for grp in range(ng) if (mask >> grp) & 1]
    dead = [grp for grp in range(ng) if not (mask >> grp) & 1]
    got0, out = [], []
    for k, (gm, ref) in enumerate(zip(gmaps, gz)):
        gm = gm.float().cpu().reshape(ng, nb, *gm.shape[1:])
        got0.append(gm[..., 0])
        out.append((gm[live][..., 0], ref[live]))
        assert bool((gm[live][..., 1:] == 0).all())          # padding channels of a written group: zeros
        assert bool((gm[dead] == SENT).all())                # groups outside the mask: memory untouched
    # ... and against the unfused list loss on the extracted channel (fp32 operands holding the same values)
    Pl = [P.clone().to(dev).requires_grad_(True) for P in Ps]
    lu = 0
    for gr, gf in pairs:
        lu = lu + ops.rahinge([P[gr].reshape(-1) for P in Pl], [P[gf].reshape(-1) for P in Pl], for_d)
    (lu * gscale).sum().backward()
    held_scalar(fam, backend, name + " loss vs unfused", loss, lu, F32_TOL)
    unfused = [(P.grad * (1 - P.detach() ** 2)).cpu()[live] for P in Pl]
    return out, unfused


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: c[0])
def test_rahinge_on_head_maps(backend, dtype, case):
    out, unfused = run_head_case(backend, dtype, case, head_gscale(dtype))
    fam = "rahinge_heads " + DTYPE_IDS[DTYPES.index(dtype)]
    for k, ((got, ref), gu) in enumerate(zip(out, unfused)):
        held(fam, backend, "%s dz scale %d" % (case[0], k), got, ref, storage_tol(dtype))
        held(fam, backend, "%s dz vs unfused scale %d" % (case[0], k), got, gu, storage_tol(dtype))


@pytest.mark.parametrize("backend", BACKENDS)
def test_rahinge_on_head_maps_fp16_without_loss_scale_rounds_to_subnormals(backend):
    """FINDING: with gscale of order 1 the fp16 head gradient of a 68 000-pixel group is about 5e-6, a subnormal fp16
    number, and misses F16_TOL through the format alone: measured 5.5e-3 of the tensor's maximum on the emulator (bound 3e-3).  This is the
    number format, not the kernel: every element is the correctly rounded fp16 value of the fp64 reference to within half a subnormal
    step (2^-25) or half an ulp (2^-11 relative), which is what is asserted here; the scaled gradient above holds F16_TOL."""
    out, _ = run_head_case(backend, torch.float16, HEAD_CASES[1], 0.37)
    for k, (got, ref) in enumerate(out):
        print("OBS|rahinge_heads f16 unscaled|%s|trainer_g dz scale %d|%.3e|%.0e" % (backend, k, rel(got, ref), F16_TOL))
        err = (got.double() - ref).abs()
        assert bool((err <= 2.0 ** -25 + 2.0 ** -11 * ref.abs() + F32_TOL * float(ref.abs().max())).all())


# --------------------------------------------------------------------------------------------------------------------
# multiscale reconstruction loss (losses.py:219-231)
# --------------------------------------------------------------------------------------------------------------------
REC_KINDS = ["l1", "smoothl1", "l2"]
# msrec_kernel takes 4-aligned maps, msrec_ragged_kernel the rest (one thread per 4 x 4 block of the ceil grid), rec_flat_kernel one scale
REC_SHAPES = [(2, 3, 16, 24),      # 4-aligned
              (1, 2, 7, 12),       # odd H
              (1, 2, 8, 13),       # odd W
              (1, 3, 12, 10),      # W % 4 == 2
              (2, 1, 3, 9),        # H < 4 (and odd W): two scales at most
              (1, 2, 5, 6),        # odd H, W % 4 == 2, second pooling floors both
              (1, 2, 4, 4)]        # one 4 x 4 block per plane


def rec_criterion(kind, a, b):
    return {"l1": F.l1_loss, "smoothl1": F.smooth_l1_loss, "l2": F.mse_loss}[kind](a, b)


def ref_msrec(kind, nscales, pred, gt):
    loss = 0
    for i in range(nscales):
        loss = loss + 0.5 ** i * rec_criterion(kind, pred, gt)
        if i != nscales - 1:
            pred, gt = F.avg_pool2d(pred, 2, stride=2, count_include_pad=False), F.avg_pool2d(gt, 2, stride=2, count_include_pad=False)
    return loss


def rec_band(pred, gt, nscales):
    """pixels of the full-size map behind a difference (at any of the scales) within MARGIN of the L1 kink |d| = 0 or smooth-L1's |d| = 1"""
    d = pred.double() - gt.double()
    H, W = d.shape[2:]
    bad = torch.zeros(d.shape, dtype=torch.bool)
    for i in range(nscales):
        near = (d.abs() < MARGIN) | ((d.abs() - 1).abs() < MARGIN)
        up = near.repeat_interleave(1 << i, 2).repeat_interleave(1 << i, 3)
        bad[:, :, :up.shape[2], :up.shape[3]] |= up[:, :, :H, :W]
        if i != nscales - 1:
            d = F.avg_pool2d(d, 2, stride=2)
    return bad


def rec_maps(shape, nscales, seed):
    g = torch.Generator().manual_seed(seed)
    pred, gt = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1      # differences on both sides of |d| = 1
    for _ in range(50):
        bad = rec_band(pred, gt, nscales)
        if not bool(bad.any()):
            break
        pred[bad] = torch.rand(int(bad.sum()), generator=g) * 2 - 1
    return pred, gt


def run_msrec(backend, dev, kind, nscales, pred, gt, gscale, tag):
    assert not bool(rec_band(pred, gt, nscales).any())
    p64 = pred.double().requires_grad_(True)
    l = ref_msrec(kind, nscales, p64, gt.double())
    (gr,) = torch.autograd.grad(l * gscale, p64)
    pd = pred.clone().to(dev).requires_grad_(True)
    l2 = ops.multiscale_rec(pd, gt.to(dev), kind, nscales)
    assert l2.dim() == 0
    (l2 * gscale).backward()
    held_scalar("msrec", backend, tag + " loss", l2, l, F32_TOL)
    held("msrec", backend, tag + " grad", pd.grad, gr, F32_TOL)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", REC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("nscales", [1, 2, 3])
@pytest.mark.parametrize("kind", REC_KINDS)
def test_multiscale_rec_aligned_and_ragged(backend, kind, nscales, shape):
    dev = use_backend(backend)
    H, W = shape[2:]
    if min(H, W) >> (nscales - 1) == 0:                      # AvgPool2d would raise "Output size is too small": so does the launcher
        z = torch.zeros(shape, device=dev)
        with pytest.raises(RuntimeError, match="too small"):
            ops.multiscale_rec(z, z, kind, nscales)
        return
    pred, gt = rec_maps(shape, nscales, 3 * H + W + nscales)
    run_msrec(backend, dev, kind, nscales, pred, gt, 0.37, "%s %d %s" % (kind, nscales, "x".join(map(str, shape))))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", REC_KINDS)
def test_multiscale_rec_refuses_maps_that_pool_to_nothing(backend, kind):
    dev = use_backend(backend)
    for shape, nscales in (((1, 1, 1, 8), 2), ((1, 2, 8, 1), 2), ((1, 1, 3, 8), 3), ((2, 1, 8, 2), 3), ((1, 1, 1, 1), 3)):
        z = torch.zeros(shape, device=dev)
        with pytest.raises(RuntimeError, match="too small"):
            ops.multiscale_rec(z, z, kind, nscales)
        assert float(ops.multiscale_rec(z, z, kind, 1)) == 0.0            # one scale never pools


# power-of-two element counts at every scale: the coefficients 2^-i / n_i are exact.  (shape, scales): aligned, H % 4 = 2, W % 4 = 2
REC_TIE_CASES = [((2, 1, 8, 8), 1), ((2, 1, 8, 8), 2), ((2, 1, 8, 8), 3), ((1, 2, 8, 16), 3), ((2, 2, 2, 8), 1), ((2, 2, 2, 8), 2), ((2, 2, 8, 2), 2),
                 ((1, 2, 8, 4), 3)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", REC_TIE_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-%d" % c[1])
@pytest.mark.parametrize("kind", ["l1", "smoothl1"])
def test_multiscale_rec_ties_follow_torch(backend, kind, case):
    """d = 0 and d = +-1 exactly, at every scale: differences that are multiples of 1/4 keep every pooled difference, every coefficient and
    every term of the gradient exact in fp32, so the gradient is compared bit for bit with torch's: sign(0) = 0, and smooth-L1 takes the
    quadratic branch only for |d| < 1."""
    dev = use_backend(backend)
    shape, nscales = case
    H, W = shape[2:]
    g = torch.Generator().manual_seed(5)
    vals = torch.tensor([0.0, 0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 0.25, 1.5])
    d = vals[torch.randint(0, len(vals), shape, generator=g)]
    d[..., :2, :2] = 1.0                                     # ties at the pooled scales too: a 2 x 2 block of ones ...
    if W >= 4:
        d[..., :2, 2:4] = torch.tensor([[1.0, -1.0], [-1.0, 1.0]])      # ... and one of +-1 that pools to 0
    if H >= 4:
        d[..., 2:4, :2] = 0.0
    assert bool((d == 0).any()) and bool((d.abs() == 1).any())
    gt = torch.randint(-4, 5, shape, generator=g) * 0.25
    pred = gt + d
    assert torch.equal(pred - gt, d)                         # exact: multiples of 1/4 of small magnitude
    p64 = pred.double().requires_grad_(True)
    l = ref_msrec(kind, nscales, p64, gt.double())
    (gr,) = torch.autograd.grad(l * 0.5, p64)
    pd = pred.clone().to(dev).requires_grad_(True)
    l2 = ops.multiscale_rec(pd, gt.to(dev), kind, nscales)
    (l2 * 0.5).backward()
    held_scalar("msrec", backend, "tie loss", l2, l, F32_TOL)
    assert torch.equal(pd.grad.cpu(), gr.float())


# MSREC_MAXB = 2048 blocks of 256 threads: 16 x 3 x 128 x 128 = 786 432 4 x 4 blocks > 524 288, so the grid-stride loop takes a second trip
# and msrec_final_kernel folds all 2048 partials; one scale: 12.6 M elements through rec_flat_kernel
@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("kind", REC_KINDS)
def test_multiscale_rec_more_blocks_than_the_grid(backend, kind):
    dev = use_backend(backend)
    shape = (16, 3, 512, 512)
    assert shape[0] * shape[1] * (shape[2] // 4) * (shape[3] // 4) > 2048 * 256
    pred, gt = rec_maps(shape, 3, 21)
    for nscales in (3, 1):
        run_msrec(backend, dev, kind, nscales, pred, gt, 0.37, "%s %d 16x3x512x512" % (kind, nscales))


# --------------------------------------------------------------------------------------------------------------------
# spectral norm (torch.nn.utils.spectral_norm: one power iteration, eps 1e-12, sigma = u^T W v)
# --------------------------------------------------------------------------------------------------------------------
# optim_sn.hip: SN_SLAB = 128 rows per slab of snm_wt_u_kernel (256 columns per block), snm_norm_v_kernel is ONE block of 1024 threads per
# layer (block-stride loop over the columns), snm_w_v_kernel one block per row, the grid of a multi-layer call is sized by the largest layer.
SN_SHAPES = [(128, 1024), (129, 1025), (300, 1500),
             (32, 147), (64, 1568), (128, 3136), (256, 3200), (512, 6400)]       # the cd32 discriminator's five trunk layers (7x7, 7x7, 7x7, 5x5, 5x5)
SN_EPS = 1e-12


def power_iteration(w, u):
    """one round in fp64: (u', v', sigma)"""
    v = F.normalize(w.t() @ u, dim=0, eps=SN_EPS)
    s = w @ v
    u2 = F.normalize(s, dim=0, eps=SN_EPS)
    return u2, v, u2 @ s


def sn_operands(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, cols, generator=g) * 0.05
    return w, F.normalize(torch.randn(rows, generator=g), dim=0), F.normalize(torch.randn(cols, generator=g), dim=0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_specnorm_sigma_slabs_and_wide_rows(backend, shape):
    dev = use_backend(backend)
    rows, cols = shape
    w, u, v = sn_operands(rows, cols, rows + cols)
    ur, vr, sr = power_iteration(w.double(), u.double())
    wd, ud, vd = w.to(dev), u.clone().to(dev), v.clone().to(dev)
    sn = ops.specnorm_sigma(wd, ud, vd, True)
    tag = "%dx%d" % shape
    held("specnorm", backend, tag + " u", ud, ur, F32_TOL)
    held("specnorm", backend, tag + " v", vd, vr, F32_TOL)
    held_scalar("specnorm", backend, tag + " sigma", sn.sigma[0], sr, F32_TOL)
    held_scalar("specnorm", backend, tag + " 1/sigma", sn.sigma[1], 1 / sr, F32_TOL)
    # eval mode: nothing moves, sigma is u^T W v of the vectors as they are
    u0, v0 = ud.clone(), vd.clone()
    sn2 = ops.specnorm_sigma(wd, ud, vd, False)
    assert torch.equal(ud, u0) and torch.equal(vd, v0)
    held_scalar("specnorm", backend, tag + " sigma no-iter", sn2.sigma[0], u0.double().cpu() @ (w.double() @ v0.double().cpu()), F32_TOL)


def sn_layers(lib, dev, shapes, n_rounds, seed):
    arr = (_lib.SnLayer * len(shapes))()
    keep = []
    for i, (rows, cols) in enumerate(shapes):
        w, u, v = sn_operands(rows, cols, seed + i)
        t = {"w": w.to(dev), "u": u.to(dev), "v": v.to(dev), "w64": w.double(),
             "sigma": torch.full((n_rounds,), SENT, device=dev), "inv": torch.full((n_rounds,), SENT, device=dev),
             "uh": torch.full((n_rounds, rows), SENT, device=dev), "vh": torch.full((n_rounds, cols), SENT, device=dev),
             "tmp": torch.full((lib.uegan_specnorm_multi_workspace_floats(rows, cols),), NAN, device=dev)}
        arr[i].w, arr[i].u, arr[i].v = t["w"].data_ptr(), t["u"].data_ptr(), t["v"].data_ptr()
        arr[i].sigma, arr[i].inv_sigma = t["sigma"].data_ptr(), t["inv"].data_ptr()
        arr[i].u_hist, arr[i].v_hist, arr[i].tmp = t["uh"].data_ptr(), t["vh"].data_ptr(), t["tmp"].data_ptr()
        arr[i].rows, arr[i].cols = rows, cols
        keep.append(t)
    return arr, keep


# layers of different shape in one call: the grid is (ceil(1568 / 256), ceil(300 / 128), layers) -- most blocks of the small layers return at once
SN_MULTI = [(300, 1500), (32, 147), (129, 1025), (64, 1568), (1, 5), (7, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_specnorm_multi_layers_and_rounds(backend):
    dev = use_backend(backend)
    lib = _lib.load()
    n_rounds = 3
    arr, keep = sn_layers(lib, dev, SN_MULTI, n_rounds, 40)
    u0 = [t["u"].clone() for t in keep]
    _lib.check(lib.uegan_specnorm_multi(arr, len(SN_MULTI), n_rounds, 1, SN_EPS, None))
    for (rows, cols), t, ustart in zip(SN_MULTI, keep, u0):
        tag = "multi %dx%d" % (rows, cols)
        uprev = ustart.double().cpu()
        for r in range(n_rounds):                            # each round is one more fp64 power iteration from the vectors the round before left
            ur, vr, sr = power_iteration(t["w64"], uprev)
            held("specnorm", backend, "%s u round %d" % (tag, r), t["uh"][r], ur, F32_TOL)
            held("specnorm", backend, "%s v round %d" % (tag, r), t["vh"][r], vr, F32_TOL)
            held_scalar("specnorm", backend, "%s sigma round %d" % (tag, r), t["sigma"][r], sr, F32_TOL)
            held_scalar("specnorm", backend, "%s 1/sigma round %d" % (tag, r), t["inv"][r], 1 / sr, F32_TOL)
            uprev = t["uh"][r].double().cpu()
        assert torch.equal(t["u"], t["uh"][n_rounds - 1]) and torch.equal(t["v"], t["vh"][n_rounds - 1])
        # against three fp64 iterations from the start as well (the error does not build up: the iteration contracts)
        uu = ustart.double().cpu()
        for r in range(n_rounds):
            uu, vv, ss = power_iteration(t["w64"], uu)
        held("specnorm", backend, tag + " u after 3", t["u"], uu, F32_TOL)
        held_scalar("specnorm", backend, tag + " sigma after 3", t["sigma"][n_rounds - 1], ss, F32_TOL)


@pytest.mark.parametrize("backend", BACKENDS)
def test_specnorm_multi_without_iteration_fills_histories(backend):
    dev = use_backend(backend)
    lib = _lib.load()
    n_rounds = 3
    shapes = [(300, 1500), (32, 147), (129, 1025)]
    arr, keep = sn_layers(lib, dev, shapes, n_rounds, 50)
    u0, v0 = [t["u"].clone() for t in keep], [t["v"].clone() for t in keep]
    _lib.check(lib.uegan_specnorm_multi(arr, len(shapes), n_rounds, 0, SN_EPS, None))
    for (rows, cols), t, a, b in zip(shapes, keep, u0, v0):
        assert torch.equal(t["u"], a) and torch.equal(t["v"], b)
        sr = a.double().cpu() @ (t["w64"] @ b.double().cpu())
        for r in range(n_rounds):
            assert torch.equal(t["uh"][r], a) and torch.equal(t["vh"][r], b)
            held_scalar("specnorm", backend, "no-iter %dx%d sigma round %d" % (rows, cols, r), t["sigma"][r], sr, F32_TOL)
            held_scalar("specnorm", backend, "no-iter %dx%d 1/sigma round %d" % (rows, cols, r), t["inv"][r], 1 / sr, F32_TOL)
        assert torch.equal(t["sigma"], t["sigma"][:1].expand(n_rounds))          # fixed summation order: the same bits every round


# dot_kernel: SN_DOTB = 256 blocks of 256 threads (one element per thread and trip: it strides beyond 65 536 elements, and its block count
# stops following ceil(n / 1024) at 256 x 1024); the rank-1 kernels cap at 512 blocks of 256 threads, 1024 elements per block: 512 x 1024
SN_GRAD_SHAPES = [(24, 200), (129, 1025), (300, 1500), (512, 1100)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SN_GRAD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_specnorm_gradient_and_accumulating_form(backend, shape):
    dev = use_backend(backend)
    lib = _lib.load()
    rows, cols = shape
    assert shape != (300, 1500) or 256 * 1024 < rows * cols < 512 * 1024
    assert shape != (512, 1100) or rows * cols > 512 * 1024
    gen = torch.Generator().manual_seed(rows)
    w, u, v = sn_operands(rows, cols, rows * 3)
    g = 0.5 * w + 0.05 * torch.randn(rows, cols, generator=gen)               # <g, w> far from 0: the rank-1 term is as large as g
    sigma = 1.7
    sig = torch.tensor([sigma, 1 / sigma], dtype=torch.float32)
    k = (g.double() * w.double()).sum() * float(sig[1])
    ref = g.double() - k * torch.outer(u.double(), v.double())
    assert float((k * torch.outer(u.double(), v.double())).abs().max()) > 0.1 * float(g.abs().max())
    gd, wd, ud, vd, sd = g.to(dev), w.to(dev), u.to(dev), v.to(dev), sig.to(dev)
    tag = "%dx%d" % shape
    tmp = torch.full((lib.uegan_specnorm_grad_workspace_floats(),), NAN, device=dev)
    dw = torch.full_like(gd, SENT)
    _lib.check(lib.uegan_specnorm_grad(gd.data_ptr(), wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd.data_ptr(), dw.data_ptr(), rows, cols,
                                       tmp.data_ptr(), None))
    held("specnorm_grad", backend, tag + " dw", dw, ref, F32_TOL)
    inplace = gd.clone()                                     # dw == g is allowed
    tmp.fill_(NAN)
    _lib.check(lib.uegan_specnorm_grad(inplace.data_ptr(), wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd.data_ptr(), inplace.data_ptr(), rows, cols,
                                       tmp.data_ptr(), None))
    assert torch.equal(inplace, dw)
    dw0 = torch.randn(rows, cols, generator=gen)
    for acc in (0, 1):
        out = dw0.clone().to(dev) if acc else torch.full_like(gd, SENT)
        tmp.fill_(NAN)
        _lib.check(lib.uegan_specnorm_grad_acc(gd.data_ptr(), wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), sd[1:].data_ptr(), out.data_ptr(), rows,
                                               cols, tmp.data_ptr(), acc, None))
        held("specnorm_grad", backend, "%s dw acc=%d" % (tag, acc), out, ref + dw0.double() if acc else ref, F32_TOL)


# --------------------------------------------------------------------------------------------------------------------
# sn_act_bwd -> sn_grad_finish (unpadded form)
# --------------------------------------------------------------------------------------------------------------------
# act_bwd.hip: a block holds pl = 256 / (C / chunk) pixels per trip, UNR = 4 trips in flight; bx = min(SNB / 2 = 128, ceil(pixels / (4 pl)))
# partial blocks per group.  sn_grad_finish folds the c_r partials 64 lanes at a time and the bias partials over 16 interleaved rows.
# (C, 0 = one chunk; groups; pixels per group; activation; second gradient; C - nbias; cols)
SNACT_CASES = [
    (0, 1, 9, ops.ACT_NONE, False, 3, 20),
    (32, 2, 3001, ops.ACT_LRELU, True, 0, 75),
    (512, 3, 2500, ops.ACT_RELU, False, 12, 40),            # 128 (fp32) / 64 (16-bit) chunks per pixel: 2 / 4 pixels per block trip, 128 partials
    (16, 4, 70001, ops.ACT_LRELU, True, 5, 147),            # 128 partials per group: more than one 64-lane fold
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", SNACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sn_act_bwd_then_grad_finish(backend, dtype, case):
    dev = use_backend(backend)
    ops.set_compute_dtype(dtype)
    lib = _lib.load()
    Cc, ng, ppg, act, use_g2, deficit, cols = case
    epc = 4 if dtype == torch.float32 else 8
    Cc = Cc or epc
    nbias = rows = Cc - deficit
    gen = torch.Generator().manual_seed(ppg + Cc)

    def rnd(t):
        return half_round(t, dtype)

    g = rnd(torch.randn(ng, ppg, Cc, generator=gen) + 0.25)
    g2 = rnd(torch.randn(ng, ppg, Cc, generator=gen)) if use_g2 else None
    y = rnd(torch.randn(ng, ppg, Cc, generator=gen))
    y[torch.rand(y.shape, generator=gen) < 0.05] = 0.0       # exact zeros: act'(0) is the negative side's slope, as in torch
    bias = torch.randn(nbias, generator=gen)
    inv = 1.0 / (1.0 + torch.rand(ng, generator=gen))
    uh = F.normalize(torch.randn(ng, rows, generator=gen), dim=1)
    vh = F.normalize(torch.randn(ng, cols, generator=gen), dim=1)
    dw0 = torch.randn(rows, cols, generator=gen)
    db0 = torch.randn(Cc, generator=gen)
    # fp64 reference on the same operands
    gs, y64 = g.double() + (g2.double() if use_g2 else 0), y.double()
    if act == ops.ACT_LRELU:
        slope, z = torch.where(y64 > 0, torch.ones_like(y64), torch.full_like(y64, 0.2)), torch.where(y64 > 0, y64, 5 * y64)
    elif act == ops.ACT_RELU:
        slope, z = (y64 > 0).double(), y64
    else:
        slope, z = torch.ones_like(y64), y64
    raw = gs * slope
    dz_ref = raw * inv.double()[:, None, None]
    b64 = torch.zeros(Cc, dtype=torch.float64)
    b64[:nbias] = bias.double()
    c_ref = (dz_ref * (z - b64)).sum((1, 2))                 # from the unrounded dz
    db_ref = raw.sum((0, 1))[:rows]
    dw_ref = dw0.double() - torch.einsum("r,ri,rj->ij", c_ref, uh.double(), vh.double())
    # the kernels
    gd, yd = g.to(dtype).to(dev), y.to(dtype).to(dev)
    g2d = g2.to(dtype).to(dev) if use_g2 else None
    bd, invd = bias.to(dev), inv.to(dev)
    ws = torch.full((lib.uegan_sn_act_bwd_workspace_floats(ng, Cc),), NAN, dtype=torch.float32, device=dev)
    dz = torch.full_like(gd, NAN)
    nbx = lib.uegan_sn_act_bwd(ops._dt(gd), act, gd.data_ptr(), ops._p(g2d), yd.data_ptr(), bd.data_ptr(), nbias, invd.data_ptr(), dz.data_ptr(),
                               ws.data_ptr(), ppg, Cc, ng, None)
    pl = 256 // (Cc // epc)
    assert nbx == min(128, (ppg + 4 * pl - 1) // (4 * pl)), nbx
    if ppg == 70001 or Cc == 512:
        assert nbx == 128
    fam = "sn_act_bwd " + DTYPE_IDS[DTYPES.index(dtype)]
    tag = "x".join(map(str, case))
    held(fam, backend, tag + " dz", dz, dz_ref, storage_tol(dtype))
    uhd, vhd = uh.to(dev), vh.to(dev)
    for mode in ("set", "acc", "null"):
        dw = dw0.clone().to(dev)
        db = torch.full((Cc,), SENT, device=dev) if mode == "set" else db0.clone().to(dev)
        _lib.check(lib.uegan_sn_grad_finish(dw.data_ptr(), None if mode == "null" else db.data_ptr(), ws.data_ptr(), nbx, ng, uhd.data_ptr(),
                                            vhd.data_ptr(), rows, cols, Cc, 1 if mode == "acc" else 0, None))
        held(fam, backend, "%s dw (%s)" % (tag, mode), dw, dw_ref, F32_TOL)
        if mode == "set":
            held(fam, backend, tag + " db", db[:rows], db_ref, F32_TOL)
            assert bool((db[rows:] == SENT).all())           # channels beyond the layer's own: untouched
        elif mode == "acc":
            held(fam, backend, tag + " db acc", db[:rows], db_ref + db0[:rows].double(), F32_TOL)
            assert torch.equal(db[rows:].cpu(), db0[rows:])
        else:
            assert torch.equal(db.cpu(), db0)


# --------------------------------------------------------------------------------------------------------------------
# multi-tensor Adam / RMSprop
# --------------------------------------------------------------------------------------------------------------------
# adam_kernel / rmsprop_kernel: grid (min(128, ceil(max n / 1024)), tensors), 256 threads: 128 x 1024 = 131 072 elements is the last size
# every block covers with four trips; one more element and the cap shows
OPT_SIZES = [1, 131072, 131073, 300000]


def run_optimizer(backend, dev, which, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) for n in sizes]
    params = [torch.nn.Parameter(p.clone().to(dev)) for p in ps]
    refp = [torch.nn.Parameter(p.double()) for p in ps]
    if which == "adam":
        opt = ops.FusedAdamL2(params, 1e-2, (0.5, 0.999), 1e-8, 1e-4)
        topt = torch.optim.Adam(refp, lr=1e-2, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-4)
    else:
        opt = variants.FusedRMSprop(params, 1e-3, 0.99, 1e-8)
        topt = torch.optim.RMSprop(refp, lr=1e-3, alpha=0.99, eps=1e-8)
    for _ in range(3):
        opt.zero_grad()
        topt.zero_grad()
        for p, q in zip(params, refp):
            gr = torch.randn(q.shape, generator=g)
            p.grad.add_((4 * gr).to(dev))                    # the kernel's grad_scale takes the factor out again
            q.grad = gr.double()
        opt.step(grad_scale=0.25)
        topt.step()
    off = 0
    for p, q in zip(params, refp):
        n = q.numel()
        held(which, backend, "param %d" % n, p, q, F32_TOL)
        st = topt.state[q]
        if which == "adam":
            held(which, backend, "exp_avg %d" % n, opt.m[off:off + n], st["exp_avg"], F32_TOL)
            held(which, backend, "exp_avg_sq %d" % n, opt.v[off:off + n], st["exp_avg_sq"], F32_TOL)
        else:
            held(which, backend, "square_avg %d" % n, opt.v[off:off + n], st["square_avg"], F32_TOL)
        off += n


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("which", ["adam", "rmsprop"])
def test_optimizer_step_across_the_block_cap(backend, which):
    dev = use_backend(backend)
    run_optimizer(backend, dev, which, OPT_SIZES, 9)


@pytest.mark.parametrize("backend", GPU_ONLY)
@pytest.mark.parametrize("which", ["adam", "rmsprop"])
def test_optimizer_step_one_large_tensor(backend, which):
    dev = use_backend(backend)
    run_optimizer(backend, dev, which, [3300000], 10)
