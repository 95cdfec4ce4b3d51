"""Inputs and CPU references of tests/test_loss_ops_gpu.py, shared with tests/test_loss_inputs_cpu.py (which checks, from the
float64 oracle alone, that every case is what its name claims and that no data-dependent branch sits where float32 could flip it).

Everything here is plain torch on the CPU: the references are oracle/loss_ref.py or a dense restatement, evaluated in the dtype
they are asked for from the same float32 inputs.  Nothing in this file touches a kernel."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_ref as O

# ------------------------------------------------------------------------------------------------
# voxel losses.  The kernels' constants: 256 threads, 2048 elements per forward workgroup and at most 1024 of them; the backward
# has 256 elements per workgroup and at most 4096.
# ------------------------------------------------------------------------------------------------
RAGGED = 5 * 2048 + 77                        # several ragged workgroups
BIG = 1024 * 2048 + 3 * 2048 + 5              # past both caps: both grid-stride loops run a second, ragged time
N_SIZES = [1, 255, 257, 2049, RAGGED, BIG]
MIX_SIZES = [257, RAGGED, BIG]
UPSTREAM = -3.5                               # d(result)/d(loss) of every voxel-loss backward in these tests
P_LO, P_HI = float(np.float32(1e-4)), float(np.float32(1 - 1e-4))     # the trainer's clamp ends, as float32 holds them

# mix -> which of (positive, soft, unlabeled) voxels it holds.  "soft" is the kernels' and the reference's class -1 < g < 1: it
# includes the labelled negatives (g = 0), so a mix without soft voxels is positives and unlabeled only - two of them, with a few
# and with half of the voxels positive.
MIXES = {"standard": (1, 1, 1), "no_pos": (0, 1, 1), "no_soft": (1, 0, 1), "pos_unl": (1, 0, 1), "soft_edges": (1, 1, 1),
         "all_soft": (0, 1, 0)}
FOCAL_MIXES = list(MIXES)
PU_MIXES = [m for m, (p, _, u) in MIXES.items() if p and u]
PRED_KINDS = ["uniform", "clamp_ends", "confident"]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _share(n, frac):
    return max(2, int(frac * n))


@functools.lru_cache(maxsize=None)
def voxel_labels(mix, n):
    """(n,) float32 labels: 1 positive, -1 unlabeled, anything between soft.  Class sizes are fixed shares of n (at least 2)."""
    g = gen("labels", mix, n)
    perm = torch.randperm(n, generator=g)
    gt = torch.full((n,), -1.0)
    at = [0]

    def put(frac, values):
        k = _share(n, frac)
        idx = perm[at[0]:at[0] + k]
        at[0] += k
        gt[idx] = values(k) if callable(values) else values
    rand = lambda k: torch.rand(k, generator=g)
    if mix in ("standard", "no_pos"):                      # the losses_inputs mix: 30 % zeros, 10 % soft in [0, 0.9), 3 % positive
        put(0.30, 0.0)
        put(0.10, lambda k: rand(k) * 0.9)
        put(0.03, 1.0 if mix == "standard" else 0.0)
    elif mix == "no_soft":
        put(0.03, 1.0)
    elif mix == "pos_unl":
        put(0.50, 1.0)
    elif mix == "soft_edges":
        put(0.03, 1.0)
        put(0.10, 0.0)
        put(0.10, lambda k: -(0.001 + 0.998 * rand(k)))                       # in (-1, 0)
        put(0.10, lambda k: 1.0 - (1e-6 + 0.99e-3 * rand(k)))                 # within 1e-3 of 1, below it
        put(0.10, lambda k: rand(k) * 0.9)
    elif mix == "all_soft":
        gt[:] = (2.0 * rand(n) - 1.0) * 0.999
        gt[perm[:_share(n, 0.10)]] = 0.0
    else:
        raise KeyError(mix)
    assert at[0] <= n
    return gt


def label_classes(gt):
    """(positive, soft, unlabeled) boolean masks, as the kernels and the reference define them"""
    return gt == 1, (gt > -1) & (gt < 1), gt == -1


@functools.lru_cache(maxsize=None)
def voxel_pred(kind, mix, n):
    from cet_pick_amd.synthetic import confident_pred
    g = gen("pred", kind, mix, n)
    if kind == "confident":
        return confident_pred(voxel_labels(mix, n), seed=zlib.crc32(repr((mix, n)).encode()))
    p = (1e-4 + torch.rand(n, generator=g) * (1 - 2e-4)).clamp(P_LO, P_HI)
    if kind == "clamp_ends":                               # a tenth of the voxels exactly at each clamp end
        perm, k = torch.randperm(n, generator=g), max(1, n // 10)
        p[perm[:k]] = P_LO
        p[perm[k:2 * k]] = P_HI
    return p


def voxel_case(n, mix, kind):
    return voxel_pred(kind, mix, n), voxel_labels(mix, n)


def _with_grad(fn, pred, dtype):
    p = pred.to(dtype).clone().requires_grad_(True)
    loss = fn(p)
    (UPSTREAM * loss).backward()
    return loss.detach(), p.grad


@functools.lru_cache(maxsize=None)
def focal_reference(n, mix, kind):
    """{dtype: (loss, d(UPSTREAM x loss)/d pred)} by the oracle and autograd"""
    pred, gt = voxel_case(n, mix, kind)
    return {dt: _with_grad(lambda p: O.neg_loss(p, gt.to(dt)), pred, dt) for dt in (torch.float32, torch.float64)}


def pu_terms(pred, gt, tau):
    """(pos_risk, neg_total) of the PU risk in the dtype of the arguments: what the branch `neg_total < -beta` decides on"""
    pos, soft, unl = (m.to(pred.dtype) for m in label_classes(gt))
    a = torch.log(pred) * (1 - pred) ** 2
    b = torch.log(1 - pred) * pred ** 2
    pos_tot, negpos_tot = -(a * pos).sum() / pos.sum(), -(b * pos).sum() / pos.sum()
    if soft.sum() > 0:
        pos_tot = pos_tot - (b * (1 - gt) ** 4 * soft).sum() / soft.sum()
        negpos_tot = negpos_tot - (a * gt ** 4 * soft).sum() / soft.sum()
    return pos_tot * tau, -tau * negpos_tot - (b * unl).sum() / unl.sum()


@functools.lru_cache(maxsize=None)
def pu_reference(n, mix, kind, tau, beta):
    pred, gt = voxel_case(n, mix, kind)
    return {dt: _with_grad(lambda p: O.pu_neg_loss(p, gt.to(dt), tau, beta), pred, dt) for dt in (torch.float32, torch.float64)}


# By the float64 oracle the one small case whose clamped predictions fall on the soft labels next to 1 has neg_total = -0.33 at
# tau = 0.6: it is a case of the dropped branch, and says so.
DROPPED = {(257, "soft_edges", "clamp_ends", 0.6)}


def pu_settings(n, mix, kind):
    """(tau, beta, the branch the case expects: True = the negative risk is kept).  Random and clamped predictions keep it, the
    confident ones (low on everything but the positives) drive it below -beta.  tau = 0.05 with beta = 0.1 is left to the kept
    side: the confident predictions put neg_total at about -0.14 there, too close to -0.1 to call it a clear case."""
    if kind == "confident":
        full = [(0.05, 0.0, False), (0.6, 0.0, False), (0.6, 0.1, False)]
        return [full[0], full[2]] if n == BIG else full
    full = [(tau, beta, (n, mix, kind, tau) not in DROPPED) for tau in (0.05, 0.6) for beta in (0.0, 0.1)]
    return [full[1], full[2]] if n == BIG else full


def big_kind(mix):
    """the largest size takes each mix with ONE kind of prediction (its float64 autograd is the suite's time)"""
    return PRED_KINDS[list(MIXES).index(mix) % 3]


FOCAL_CASES = [(n, m, k) for n in MIX_SIZES for m in FOCAL_MIXES for k in PRED_KINDS if n != BIG or k == big_kind(m)]
PU_CASES = [(n, m, k) for n in MIX_SIZES for m in PU_MIXES for k in PRED_KINDS if n != BIG or k == big_kind(m)]


SIZE_PU = (0.05, 0.1)                         # (tau, beta) of the size sweep: the kept branch, by a wide margin


def size_case(n):
    """the size sweep: the standard mix, or - one voxel - a single positive (focal and MSE only)"""
    if n == 1:
        return torch.tensor([0.3]), torch.tensor([1.0])
    return voxel_case(n, "standard", "uniform")


@functools.lru_cache(maxsize=None)
def mse_case(n, offset):
    g = gen("mse", n, offset)
    a = torch.rand(n, generator=g) + offset
    b = (a + 0.1 * torch.randn(n, generator=g)).float()
    return a, b


def mse_reference(a, b):
    out = {}
    for dt in (torch.float32, torch.float64):
        x, y = a.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True)
        loss = O.mse(x, y)
        (UPSTREAM * loss).backward()
        out[dt] = (loss.detach(), x.grad, y.grad)
    return out


# ------------------------------------------------------------------------------------------------
# contrastive row sums
# ------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634
UCL_SIZES = [2, 6, 32, 34, 62, 64, 66, 130, 1554]          # 66, 130: N = 33, 65 - a row and its pair in different 32-wide tiles
UCL_DIMS = [32, 64]
INV_TS = [float(np.float32(1 / 0.07)), float(np.float32(1 / 0.5))]      # what the kernel gets: a float
FEATURE_KINDS = ["normalised", "spread", "twin", "same_views", "zero_row"]
CLASS_KINDS = ["random", "all0", "all3", "bit0_first_half"]
UCL_SCALES = (1.0, 0.7, 0.5, 0.3)                          # upstream gradients of s_all, s_pos, s_other, e_pair


def ucl_features(kind, n2, dim, key=0):
    g = gen("ucl", kind, n2, dim, key)
    f = F.normalize(torch.randn(n2, dim, generator=g), dim=1)
    h = n2 // 2
    if kind == "spread":                                   # row norms over [0.5, 2]: the general backward kernel
        f = f * torch.linspace(0.5, 2.0, n2)[torch.randperm(n2, generator=g)][:, None]
    elif kind == "twin":                                   # rows 0 and 1 identical and no pair: S[0][1] ties the row maximum
        assert h > 1
        f[1] = f[0]
    elif kind == "same_views":                             # f_cr == f: the pair element is exp(0)
        f[h:] = f[:h]
    elif kind == "zero_row":
        f[n2 - 1] = 0.0
    elif kind != "normalised":
        raise KeyError(kind)
    return f.contiguous()


def ucl_classes(kind, n2, key=0):
    g = gen("cls", kind, n2, key)
    if kind == "random":
        c = torch.randint(0, 4, (n2,), generator=g)
    elif kind == "all0":
        c = torch.zeros(n2, dtype=torch.long)
    elif kind == "all3":
        c = torch.full((n2,), 3)
    elif kind == "bit0_first_half":
        c = 2 * torch.randint(0, 2, (n2,), generator=g) + (torch.arange(n2) < n2 // 2).long()
    else:
        raise KeyError(kind)
    return c.to(torch.uint8)


def ucl_combos(n2):
    """(feature kind, class kind, inv_T) of one size: every feature kind at both temperatures, the class kinds in turn"""
    out = []
    for i, fk in enumerate(FEATURE_KINDS):
        if fk == "twin" and n2 < 6:                        # (2N = 2: the only other row is the pair)
            continue
        for j, inv_T in enumerate(INV_TS):
            out.append((fk, CLASS_KINDS[(2 * i + j) % 4], inv_T))
    return out


@functools.lru_cache(maxsize=None)
def ucl_gouts(n2):
    g = gen("gouts", n2)
    return tuple(torch.randn(n2, generator=g) * s for s in UCL_SCALES)


def ucl_dense(f, cls, inv_T, gouts, dtype):
    """The dense evaluation: E = exp(S - rowmax) with the diagonal masked to exp(0), its row sums under the class masks and the
    pair element; the gradient of sum_k <out_k, gouts[k]> (None: that output takes no part).  Returns
    (rowmax, s_all, s_pos, s_other, e_pair, dfeat) in `dtype`."""
    x = f.to(dtype).clone().requires_grad_(True)
    n2 = x.shape[0]
    S = (x @ x.t()) * inv_T
    m = S.max(1, keepdim=True)[0].detach()
    X = torch.exp(S - m)
    E = X * (1 - torch.eye(n2, dtype=dtype))
    pos, oth = (cls & 1).to(dtype), ((cls >> 1) & 1).to(dtype)
    ar = torch.arange(n2)
    outs = (E.sum(1) + 1, (E * pos).sum(1) + pos, (E * oth).sum(1) + oth, X[ar, (ar + n2 // 2) % n2])
    total = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gouts) if g is not None)
    total.backward()
    return (m[:, 0],) + tuple(o.detach() for o in outs) + (x.grad,)


@functools.lru_cache(maxsize=None)
def ucl_reference(n2, dim, fkind, ckind, inv_T):
    f, cls = ucl_features(fkind, n2, dim), ucl_classes(ckind, n2)
    return f, cls, {dt: ucl_dense(f, cls, inv_T, ucl_gouts(n2), dt) for dt in (torch.float32, torch.float64)}


# the range decision: row maxima (base-2 units) spread clearly below and clearly above the kernel's 16
RANGE_SIZES = [66, 1554]
RANGE_INV_T = INV_TS[0]
RANGE_NORMS = {"near": (1.0, 1.25), "far": (1.0, 1.42)}    # (b^2 - a^2) log2(e) / T = 11.6 and 20.9
RANGE_BOUND = {"near": lambda s: 8.0 <= s <= 12.0, "far": lambda s: 20.0 <= s <= 24.0}


@functools.lru_cache(maxsize=None)
def range_case(side, n2):
    g = gen("range", side, n2)
    lo, hi = RANGE_NORMS[side]
    f = F.normalize(torch.randn(n2, 32, generator=g), dim=1) * torch.linspace(lo, hi, n2)[torch.randperm(n2, generator=g)][:, None]
    f, cls = f.contiguous(), ucl_classes("random", n2, key=1)
    return f, cls, {dt: ucl_dense(f, cls, RANGE_INV_T, ucl_gouts(n2), dt) for dt in (torch.float32, torch.float64)}


def rowmax_spread(rowmax):
    return float((rowmax.max() - rowmax.min()) * LOG2E)


# ------------------------------------------------------------------------------------------------
# UnbiasedConLoss
# ------------------------------------------------------------------------------------------------
TAIL_T, TAIL_TAU_PLUS = 0.1, 0.05
TAIL_NS, TAIL_DIMS, TAIL_THRESH = [5, 33, 777], [16, 32, 48, 64], [1.0, 0.4]
TAIL_SETS = ["standard", "no_hi", "no_lo", "no_mid", "one_pos"]
# every combination at the two small sizes; at N = 777 (a 1554^2 dense float64 graph) each set with both thresholds, widths in turn
TAIL_CASES = [(n, d, t, s) for n in TAIL_NS[:2] for d in TAIL_DIMS for t in TAIL_THRESH for s in TAIL_SETS] + \
             [(777, TAIL_DIMS[(2 * i + j) % 4], t, s) for i, s in enumerate(TAIL_SETS) for j, t in enumerate(TAIL_THRESH)]


@functools.lru_cache(maxsize=None)
def tail_case(n, dim, kind):
    """labels (1 positive, 0.5 soft, 0 negative, -1 unlabeled), the two views' predictions and features.  The predictions of the
    unlabeled voxels fall into three sets - above 0.99, below 0.01 and between - of which `kind` leaves one empty."""
    g = gen("tail", n, dim, kind)
    lab = torch.full((n,), -1.0)
    perm = torch.randperm(n, generator=g)
    n_pos = 1 if kind == "one_pos" or n < 10 else max(2, n // 20)
    n_soft, n_zero = max(1, n // 10), max(0, n // 4 - 1)
    lab[perm[:n_pos]] = 1.0
    lab[perm[n_pos:n_pos + n_soft]] = 0.5
    lab[perm[n_pos + n_soft:n_pos + n_soft + n_zero]] = 0.0
    f = F.normalize(torch.randn(n, dim, generator=g), dim=1)
    f_cr = F.normalize(f + 0.3 * torch.randn(n, dim, generator=g), dim=1)
    levels = {"hi": 0.995, "lo": 0.004, "mid": None}
    keep = [k for k in levels if kind != "no_" + k]
    which = torch.randint(0, len(keep), (2, n), generator=g)
    which[:, perm[-len(keep):]] = torch.arange(len(keep))[None, :]            # every kept set holds an unlabeled voxel of each view
    mid = 0.05 + 0.9 * torch.rand(2, n, generator=g)
    o = mid.clone()
    for i, k in enumerate(keep):
        if levels[k] is not None:
            o[which == i] = levels[k]
    return lab, o[0].contiguous(), o[1].contiguous(), f, f_cr


def tail_sets(lab, o1, o2):
    """sizes of the three prediction sets over the unlabeled voxels of both views"""
    un = torch.cat([lab, lab]) < 0
    p = torch.cat([o1, o2])
    return {"hi": int((un & (p > 0.99)).sum()), "lo": int((un & (p < 0.01)).sum()),
            "mid": int((un & (p > 0.01) & (p < 0.99)).sum())}


@functools.lru_cache(maxsize=None)
def tail_reference(n, dim, thresh, kind):
    """{dtype: (sup, unsup, [d(sup + 0.1 unsup) / d f, f_cr, o1, o2])} by the dense oracle"""
    lab, o1, o2, f, f_cr = tail_case(n, dim, kind)
    out = {}
    for dt in (torch.float32, torch.float64):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in (f, f_cr, o1, o2)]
        sup, unsup = O.unbiased_con_loss(lab.to(dt), leaves[2], leaves[3], leaves[0], leaves[1], TAIL_T, TAIL_TAU_PLUS, thresh)
        (sup + 0.1 * unsup).backward()
        out[dt] = (sup.detach(), unsup.detach(), [t.grad for t in leaves])
    return out
