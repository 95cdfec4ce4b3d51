"""Inputs and CPU references of tests/test_ge_loss_gpu.py, shared with tests/test_ge_cases_cpu.py (which checks the references
against central differences and every case against what its name claims, from float64 alone).

The GE-binomial heat-map loss (reference cet_pick/models/loss.py:215-253, `PUGELoss`), restated: with U the voxels where gt == -1,
N = |U|, mu = sum_U p, v = sum_U p (1 - p), w = v + 1e-7,
    s_k = -(mu - k)^2 / (2 w),  q = softmax(s) over k = 0 .. N,  b_k = log Binom(k; N, tau),  B = sum_k q_k b_k
    pen = -B  (+ entropy_penalty / 2 (log v + log 2 pi + 1) when entropy_penalty > 0)
    loss = focal(voxels with gt >= 0) + slack pen
    g_mu = -sum_k q_k (b_k - B)(k - mu) / w,  g_v = -sum_k q_k (b_k - B)(k - mu)^2 / (2 w^2)  (+ entropy_penalty / (2 v))
    d loss / d p_i = slack (g_mu + g_v (1 - 2 p_i)) on U, the focal gradient elsewhere.
Everything here is numpy, scipy and torch on the CPU; nothing in this file touches a kernel."""
import functools
import math
import zlib

import numpy as np
import torch
from scipy.special import gammaln
from scipy.stats import binom

UPSTREAM = -3.5                               # d(result)/d(loss) of every backward in these tests
W_FLOOR = 1e-7
CUT = 746.0                                   # the kernel's window: exp(-x) of a double is 0 for x > 745.2

# the kernels' constants (csrc/loss_ge.hip): 256 threads, 2048 voxels per workgroup of the partial pass and at most 1024 of them;
# the count stage has 256 counts per workgroup and at most 32 of them
WG, VOX_PER_WG, VOX_WGS, COUNT_WGS = 256, 256 * 8, 1024, 32
COUNT_GRID = COUNT_WGS * WG
BIG = VOX_WGS * VOX_PER_WG + 5                # past the partial pass's grid cap
SIZES = [37, 256, 257, VOX_PER_WG + 3, BIG]
MIXES = ["no_unl", "one_unl", "all_unl", "train"]
REGIMES = ["at_tau", "far", "tiny", "near_tie"]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def labels(mix, n):
    """(n,) float32 labels: 1 positive, -1 unlabeled, anything between soft"""
    g = gen("ge labels", mix, n)
    r = torch.rand(n, generator=g)
    soft = torch.rand(n, generator=g) * 0.9
    perm = torch.randperm(n, generator=g)
    if mix == "all_unl":
        return torch.full((n,), -1.0)
    if mix == "train":                        # the trainer tests' mix: 60 % unlabeled, 30 % zeros, soft values, a few exact 1s
        gt = torch.full((n,), -1.0)
        gt[r < 0.3] = 0.0
        m = (r >= 0.3) & (r < 0.4)
        gt[m] = soft[m]
        gt[r > 0.96] = 1.0
        gt[perm[0]] = 1.0
        gt[perm[1:3]] = -1.0
        return gt
    gt = torch.zeros(n)                       # labelled only ...
    gt[r < 0.2] = soft[r < 0.2]
    gt[perm[:max(1, n // 30)]] = 1.0
    if mix == "one_unl":                      # ... but for one voxel
        gt[perm[-1]] = -1.0
    elif mix != "no_unl":
        raise KeyError(mix)
    return gt


@functools.lru_cache(maxsize=None)
def preds(regime, mix, n, tau):
    """(n,) float32 heat-map: uniform over the trainer's clamp range on the labelled voxels, `regime` on the unlabeled ones"""
    g = gen("ge pred", regime, mix, n, tau)
    p = (1e-4 + torch.rand(n, generator=g) * (1 - 2e-4)).clamp(1e-4, 1 - 1e-4)
    u = torch.rand(n, generator=g)
    unl = labels(mix, n) == -1
    N = int(unl.sum())
    if regime == "at_tau":                    # mu / N at tau
        pu = tau * (0.8 + 0.4 * u)
    elif regime == "far":                     # p about 0.5 whatever tau is
        pu = 0.45 + 0.1 * u
    elif regime == "tiny":                    # v tiny: the 1e-7 floor is part of w, q is nearly one-hot
        pu = 1e-6 + 9e-6 * u
    elif regime == "near_tie":                # mu within 1e-3 of k + 1/2: moved there over (up to) eight voxels
        pu = (0.3 + 0.4 * u).double()
        idx = torch.nonzero(unl)[:8, 0]
        if N:
            mu = float(pu[unl].sum())
            pu[idx] += (math.floor(mu) + 0.5 + 5e-4 - mu) / idx.numel()
    else:
        raise KeyError(regime)
    p[unl] = pu.float()[unl]
    return p


def case_inputs(case):
    return preds(case.regime, case.mix, case.n, case.tau), labels(case.mix, case.n)


class Case:
    def __init__(self, n, mix, regime, tau, slack=1.0, entropy_penalty=0.0, walked=None):
        self.n, self.mix, self.regime, self.tau, self.slack, self.entropy_penalty = n, mix, regime, tau, slack, entropy_penalty
        self.walked = walked                  # what the case claims about the number of counts the count stage walks

    @property
    def id(self):
        s = "n%d-%s-%s-tau%g" % (self.n, self.mix, self.regime, self.tau)
        s += "-slack%g" % self.slack if self.slack != 1.0 else ""
        return s + ("-ent%g" % self.entropy_penalty if self.entropy_penalty else "")


RAG = VOX_PER_WG + 3
CASES = (
    # the size sweep: the training-like mix at every voxel count
    [Case(n, "train", "at_tau", 0.1) for n in SIZES] +
    # label mixes x regimes
    [Case(37, "no_unl", "at_tau", 0.1), Case(RAG, "no_unl", "at_tau", 0.5),
     Case(257, "one_unl", "far", 0.01), Case(257, "one_unl", "tiny", 0.1), Case(RAG, "one_unl", "near_tie", 0.5),
     Case(RAG, "all_unl", "at_tau", 0.5), Case(RAG, "all_unl", "far", 0.01), Case(RAG, "all_unl", "tiny", 0.01),
     Case(RAG, "all_unl", "near_tie", 0.1), Case(37, "all_unl", "at_tau", 0.1),
     Case(RAG, "train", "far", 0.01), Case(RAG, "train", "tiny", 0.1), Case(257, "train", "near_tie", 0.5),
     Case(RAG, "train", "at_tau", 0.5), Case(37, "train", "near_tie", 0.01), Case(256, "train", "tiny", 0.5)] +
    # the count stage against its own geometry: p about 0.5 on N unlabeled voxels puts all N + 1 counts inside the window up to
    # N = 1490, and about 39 sqrt(N) of them beyond
    [Case(WG - 2, "all_unl", "far", 0.01, walked="below_wg"), Case(WG - 1, "all_unl", "far", 0.1, walked="at_wg"),
     Case(WG, "all_unl", "far", 0.5, walked="past_wg"), Case(8 * COUNT_GRID, "all_unl", "far", 0.5, walked="past_grid"),
     Case(BIG, "all_unl", "far", 0.01, walked="past_grid")] +
    [Case(RAG, "train", "at_tau", 0.1, slack=0.5), Case(RAG, "train", "far", 0.1, entropy_penalty=0.3)]
)
WALKED = {"below_wg": lambda c: c == WG - 1, "at_wg": lambda c: c == WG, "past_wg": lambda c: c == WG + 1,
          "past_grid": lambda c: c > COUNT_GRID}


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def log_binom_lgamma(k, N, tau):
    """b_k in the form the kernel uses"""
    k = np.asarray(k, np.float64)
    return gammaln(N + 1.0) - gammaln(k + 1.0) - gammaln(N - k + 1.0) + k * math.log(tau) + (N - k) * math.log1p(-tau)


def window(N, mu, w):
    """(k_lo, k_hi) as csrc/loss_ge.hip takes them: the counts whose term can be non-zero next to the largest one, at k*"""
    ks = min(max(float(np.rint(mu)), 0.0), float(N))
    R = math.sqrt((ks - mu) ** 2 + 2.0 * CUT * w)
    return int(max(0.0, math.floor(mu - R))), int(min(float(N), math.ceil(mu + R)))


def count_stage64(N, mu, v, tau, entropy_penalty=0.0, k_range=None, log_binom=None):
    """float64: (pen, B, g_mu, g_v, q) over the counts k_range = (lo, hi), all N + 1 of them when None"""
    w = v + W_FLOOR
    lo, hi = (0, N) if k_range is None else k_range
    k = np.arange(lo, hi + 1, dtype=np.float64)
    s = -0.5 * (mu - k) ** 2 / w
    e = np.exp(s - s.max())
    q = e / e.sum()
    b = (binom.logpmf(np.arange(lo, hi + 1), N, tau) if log_binom is None else log_binom(k, N, tau)).astype(np.float64)
    # b_k - B is taken as (b_k - b_k*) - sum_j q_j (b_j - b_k*), k* the count of the largest term: where q is nearly one-hot B
    # rounds to b_k* and b_k* - B to 0, which loses the k* term of the two gradient sums - 1.1e-2 of g_mu at mu = 0.011
    # (tests/test_ge_cases_cpu.py holds both forms against 400-digit arithmetic)
    ks = int(np.argmax(s))
    bs = b - b[ks]
    Bs = float((q * bs).sum())
    B = float(b[ks]) + Bs
    pen = -B
    g_mu = -float((q * (bs - Bs) * (k - mu)).sum()) / w
    g_v = -float((q * (bs - Bs) * (k - mu) ** 2).sum()) / (2.0 * w * w)
    if entropy_penalty > 0:
        with np.errstate(divide="ignore"):
            pen += entropy_penalty * 0.5 * (float(np.log(v)) + math.log(2.0 * math.pi) + 1.0)
            g_v += entropy_penalty / (2.0 * v) if v > 0 else math.inf
    return pen, B, g_mu, g_v, q


def classes(gt):
    """(positive, soft, unlabeled) boolean arrays"""
    gt = np.asarray(gt)
    return gt == 1, (gt > -1) & (gt < 1), gt == -1


def reference64(pred, gt, tau, slack=1.0, entropy_penalty=0.0, k_range=None):
    """The float64 restatement from float32 inputs: (loss, d loss / d pred, info) - the full, unwindowed softmax unless k_range"""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    pos, soft, unl = classes(g)
    n_pos = int(pos.sum())
    a, b = np.log(p) * (1 - p) ** 2, np.log1p(-p) * p ** 2
    da, db = (1 - p) ** 2 / p - 2 * (1 - p) * np.log(p), -p ** 2 / (1 - p) + 2 * p * np.log1p(-p)
    wgt = (1 - g) ** 4
    grad = np.zeros_like(p)
    if n_pos == 0:
        focal = -float((b * wgt)[soft].sum())
        grad[soft] = -(db * wgt)[soft]
    else:
        focal = -float(a[pos].sum() + (b * wgt)[soft].sum()) / n_pos
        grad[pos] = -da[pos] / n_pos
        grad[soft] = -(db * wgt)[soft] / n_pos
    pu = p[unl]
    N, mu, v = int(unl.sum()), float(pu.sum()), float((pu * (1 - pu)).sum())
    pen, B, g_mu, g_v, q = count_stage64(N, mu, v, tau, entropy_penalty, k_range if k_range != "window" else window(N, mu, v + W_FLOOR))
    grad[unl] = slack * (g_mu + g_v * (1 - 2 * pu))
    info = dict(N=N, mu=mu, v=v, pen=pen, B=B, g_mu=g_mu, g_v=g_v, focal=focal, q=q, counts=(n_pos, int(soft.sum()), N))
    return focal + slack * pen, grad, info


def evaluate32(pred, gt, tau, slack=1.0, entropy_penalty=0.0):
    """The same formula in float32 torch with autograd: (loss, d(UPSTREAM x loss)/d pred) - the yardstick of conftest.f32_equivalent"""
    p = pred.float().clone().requires_grad_(True)
    g = gt.float()
    pos, soft, unl = g == 1, (g > -1) & (g < 1), g == -1
    zero = torch.zeros_like(p)
    a, b = torch.log(p) * (1 - p) ** 2, torch.log(1 - p) * p ** 2
    pos_sum, soft_sum = torch.where(pos, a, zero).sum(), torch.where(soft, b * (1 - g) ** 4, zero).sum()
    focal = -soft_sum if int(pos.sum()) == 0 else -(pos_sum + soft_sum) / pos.sum()
    pu = p[unl]
    N = pu.numel()
    mu, v = pu.sum(), (pu * (1 - pu)).sum()
    k = torch.arange(N + 1, dtype=torch.float32)
    q = torch.softmax(-0.5 * (mu - k) ** 2 / (v + W_FLOOR), dim=0)
    pen = -(torch.from_numpy(binom.logpmf(np.arange(N + 1), N, tau)).float() * q).sum()
    if entropy_penalty > 0:
        pen = pen + entropy_penalty * 0.5 * (torch.log(v) + math.log(2.0 * math.pi) + 1.0)
    loss = focal + slack * pen
    (UPSTREAM * loss).backward()
    return loss.detach(), p.grad


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(loss64, UPSTREAM x gradient64, info, loss32, UPSTREAM x gradient32) of a case, computed once"""
    pred, gt = case_inputs(case)
    loss, grad, info = reference64(pred, gt, case.tau, case.slack, case.entropy_penalty)
    l32, g32 = evaluate32(pred, gt, case.tau, case.slack, case.entropy_penalty)
    return loss, UPSTREAM * grad, info, l32, g32
