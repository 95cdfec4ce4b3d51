"""The references and inputs of tests/test_ge_loss_gpu.py, checked from float64 alone (no GPU): the restated gradient against central
differences, the lgamma form of log Binom against scipy, the windowed count sum against the full one, and every case against what
its name claims (class counts, regime of the predictions, number of counts the count stage walks).  Last, the binding and the built
library carry the two entry points."""
import math
import os
import re

import numpy as np
import pytest
from scipy.stats import binom

import ge_loss_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in C.CASES if c.n <= C.RAG]
IDS = lambda cases: [c.id for c in cases]


def test_case_constants_are_the_kernels():
    src = open(os.path.join(REPO, "cet_pick_amd", "csrc", "loss_ge.hip")).read()
    assert int(re.search(r"GE_COUNT_BLOCKS = (\d+);", src).group(1)) == C.COUNT_WGS
    assert re.search(r"\(n \+ 256 \* 8 - 1\) / \(256 \* 8\), 1024\)", src) and (C.VOX_PER_WG, C.VOX_WGS) == (256 * 8, 1024)
    assert float(re.search(r"GE_CUT = ([0-9.]+);", src).group(1)) == C.CUT
    assert C.SIZES == [37, 256, 257, 256 * 8 + 3, 1024 * 256 * 8 + 5]
    assert {c.n for c in C.CASES if c.mix == "train" and c.regime == "at_tau" and c.tau == 0.1} >= set(C.SIZES)
    assert {c.mix for c in C.CASES} == set(C.MIXES) and {c.tau for c in C.CASES} == {0.01, 0.1, 0.5}
    for mix in ("one_unl", "all_unl", "train"):
        assert {c.regime for c in C.CASES if c.mix == mix} >= {"far", "tiny", "near_tie"}, mix
    assert {c.regime for c in C.CASES if c.mix in ("all_unl", "train")} == set(C.REGIMES)
    assert {c.walked for c in C.CASES} == {None} | set(C.WALKED)
    assert sum(c.slack == 0.5 for c in C.CASES) == 1 and sum(c.entropy_penalty == 0.3 for c in C.CASES) == 1


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_gradient_against_central_differences(case):
    pred, gt = C.case_inputs(case)
    p = pred.numpy().astype(np.float64)
    loss, grad, _ = C.reference64(p, gt, case.tau, case.slack, case.entropy_penalty)
    rng = np.random.RandomState(case.n)
    picks = []
    for m in C.classes(gt.numpy()):
        where = np.nonzero(m)[0]
        picks += list(rng.choice(where, size=min(4, where.size), replace=False))
    for i in picks:
        h = min(1e-6, 0.01 * p[i])
        hi, lo = p.copy(), p.copy()
        hi[i] += h
        lo[i] -= h
        fd = (C.reference64(hi, gt, case.tau, case.slack, case.entropy_penalty)[0] -
              C.reference64(lo, gt, case.tau, case.slack, case.entropy_penalty)[0]) / (2 * h)
        # six digits, above the rounding of the two losses themselves
        assert abs(fd - grad[i]) <= 1e-5 * abs(grad[i]) + 64 * np.finfo(np.float64).eps * abs(loss) / h, (i, fd, grad[i])


@pytest.mark.parametrize("N", [0, 1, 37, 5000, C.BIG])
@pytest.mark.parametrize("tau", [0.01, 0.1, 0.5])
def test_lgamma_form_of_log_binom(N, tau):
    k = np.arange(N + 1) if N <= 5000 else np.unique(np.concatenate([np.arange(0, N + 1, 997), [N // 2, N - 1, N]]))
    want = binom.logpmf(k, N, tau)
    got = C.log_binom_lgamma(k, N, tau)
    assert np.isfinite(want).all()
    # three lgamma values of up to N log N each, a few roundings apiece
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=32 * np.finfo(np.float64).eps * (N + 2) * math.log(N + 2))


@pytest.mark.parametrize("case", C.CASES, ids=IDS(C.CASES))
def test_windowed_sum_is_the_full_sum(case):
    info = C.case_reference(case)[2]
    N, mu, v = info["N"], info["mu"], info["v"]
    lo, hi = C.window(N, mu, v + C.W_FLOOR)
    q = info["q"]
    assert 0 <= lo <= hi <= N and q.size == N + 1
    assert not q[:lo].any() and not q[hi + 1:].any(), "a count outside the window has a non-zero term"
    full = C.count_stage64(N, mu, v, case.tau, case.entropy_penalty)[:4]
    part = C.count_stage64(N, mu, v, case.tau, case.entropy_penalty, k_range=(lo, hi))[:4]
    # the same non-zero terms in another summation order: equal to 1e-12 of the sum of their magnitudes (g_mu is a sum that
    # cancels: it vanishes where mu sits at the prior's mode)
    k, w = np.arange(N + 1, dtype=np.float64), v + C.W_FLOOR
    t = q * np.abs(binom.logpmf(np.arange(N + 1), N, case.tau) - info["B"])
    mags = [float((q * np.abs(binom.logpmf(np.arange(N + 1), N, case.tau))).sum()), None, float((t * np.abs(k - mu)).sum()) / w,
            float((t * (k - mu) ** 2).sum()) / (2 * w * w)]
    mags[1] = mags[0]
    for a, b, m in zip(part, full, mags):
        assert abs(a - b) <= 1e-12 * m + 1e-300, (a, b, m)
    # ... and with b_k in the kernel's lgamma form: the penalty, to the accuracy of that form (test_lgamma_form_of_log_binom)
    pen_lg = C.count_stage64(N, mu, v, case.tau, case.entropy_penalty, k_range=(lo, hi), log_binom=C.log_binom_lgamma)[0]
    assert abs(pen_lg - full[0]) <= 1e-13 * abs(full[0]) + 32 * np.finfo(np.float64).eps * (N + 2) * math.log(N + 2)
    if case.walked:
        assert C.WALKED[case.walked](hi - lo + 1), (case.walked, hi - lo + 1)


NARROW = [c for c in C.CASES if c.n <= 257 or c.regime == "tiny"]


@pytest.mark.parametrize("case", NARROW, ids=IDS(NARROW))
def test_count_stage_against_400_digit_arithmetic(case):
    """The restated count stage, as written (b_k relative to b_k*), against the same sums in 400-digit arithmetic (a term of 1e-298
    next to 1 has to survive in B).  Where q is nearly one-hot the plain float64 form - b_k - B with B = sum q b - is off by about
    mu in g_mu: shown on the tiny cases."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.dps = 400
    info = C.case_reference(case)[2]
    N, mu, v = info["N"], info["mu"], info["v"]
    lo, hi = C.window(N, mu, v + C.W_FLOOR)
    assert hi - lo < 300
    m_mu, m_w, m_tau = mp.mpf(mu), mp.mpf(v) + mp.mpf(C.W_FLOOR), mp.mpf(case.tau)
    ks = range(lo, hi + 1)
    s = [-(m_mu - k) ** 2 / (2 * m_w) for k in ks]
    e = [mp.exp(x - max(s)) for x in s]
    q = [x / mp.fsum(e) for x in e]
    b = [mp.loggamma(N + 1) - mp.loggamma(k + 1) - mp.loggamma(N - k + 1) + k * mp.log(m_tau) + (N - k) * mp.log(1 - m_tau) for k in ks]
    B = mp.fsum(x * y for x, y in zip(q, b))
    g_mu = -mp.fsum(x * (y - B) * (k - m_mu) for x, y, k in zip(q, b, ks)) / m_w
    g_v = -mp.fsum(x * (y - B) * (k - m_mu) ** 2 for x, y, k in zip(q, b, ks)) / (2 * m_w * m_w)
    pen, _, got_mu, got_v, _ = C.count_stage64(N, mu, v, case.tau)
    # scipy's b_k: a few roundings of values up to N log N; the sums: of their terms' magnitudes
    b_err = 32 * np.finfo(np.float64).eps * (N + 2) * math.log(N + 2)
    mag_mu = float(mp.fsum(abs(x * (y - B) * (k - m_mu)) for x, y, k in zip(q, b, ks)) / m_w)
    mag_v = float(mp.fsum(abs(x * (y - B)) * (k - m_mu) ** 2 for x, y, k in zip(q, b, ks)) / (2 * m_w * m_w))
    assert abs(pen + float(B)) <= 1e-13 * abs(float(B)) + b_err
    if N:
        # b_k - b_k* is exact at k* and carries b_err elsewhere: every count but k* brings b_err times its own weight into the sums,
        # once through its own term and once, through B, into the term at k*
        star = max(range(len(s)), key=lambda i: s[i])
        d = [abs(k - m_mu) for k in ks]
        lost_mu = 2 * b_err * float(mp.fsum(q[i] * (d[i] + d[star]) for i in range(len(d)) if i != star) / m_w)
        lost_v = 2 * b_err * float(mp.fsum(q[i] * (d[i] ** 2 + d[star] ** 2) for i in range(len(d)) if i != star) / (2 * m_w * m_w))
        assert abs(got_mu - float(g_mu)) <= 1e-12 * mag_mu + lost_mu + 1e-300, (got_mu, float(g_mu))
        assert abs(got_v - float(g_v)) <= 1e-12 * mag_v + lost_v + 1e-300, (got_v, float(g_v))
    if case.regime == "tiny" and N > 1:
        kk = np.arange(N + 1, dtype=np.float64)
        bb = binom.logpmf(np.arange(N + 1), N, case.tau)
        qq = info["q"]
        plain = -float((qq * (bb - float((qq * bb).sum())) * (kk - mu)).sum()) / (v + C.W_FLOOR)
        assert 0.5 * mu <= abs(plain / float(g_mu) - 1.0) <= 2.0 * mu, (plain, float(g_mu), mu)


@pytest.mark.parametrize("case", C.CASES, ids=IDS(C.CASES))
def test_cases_hold_what_they_claim(case):
    pred, gt = C.case_inputs(case)
    loss, grad, info, l32, g32 = C.case_reference(case)
    n_pos, n_soft, N = info["counts"]
    assert pred.shape == gt.shape == (case.n,) and n_pos + n_soft + N == case.n
    assert float(pred.min()) > 0 and float(pred.max()) < 1
    assert {"no_unl": N == 0 and n_pos >= 1 and n_soft >= 2, "one_unl": N == 1 and n_pos >= 1 and n_soft >= 2,
            "all_unl": N == case.n, "train": N >= 2 and n_pos >= 1 and n_soft >= 2 and int(((gt > 0) & (gt < 1)).sum()) >= 1}[case.mix]
    mu, v, q = info["mu"], info["v"], info["q"]
    if N == 0:
        assert info["pen"] == 0.0 and loss == info["focal"]
    elif case.regime == "at_tau":             # the penalty sits at the binomial's mode: -b_mode + 1/2 for a Gaussian q of the binomial's width
        mode = binom.logpmf(int(round(N * case.tau)), N, case.tau)
        # (p = tau (0.8 + 0.4 u): the mean of N of them is tau to 0.115 tau / sqrt(N), four of those allowed)
        assert abs(mu / N - case.tau) <= 0.5 * case.tau / math.sqrt(N) and -mode <= info["pen"] <= -mode + 1.0, (mu / N, info["pen"], mode)
    elif case.regime == "far":
        assert abs(mu / N - 0.5) <= 0.05
        if case.tau == 0.01 and N >= 100:
            assert info["pen"] >= 100.0, info["pen"]
    elif case.regime == "tiny":
        assert v <= 1e-5 * N and float(q.max()) >= 1 - 1e-12
        if N == 1:
            assert C.W_FLOOR >= 0.01 * (v + C.W_FLOOR)
    elif case.regime == "near_tie":
        assert abs(mu - (math.floor(mu) + 0.5)) <= 1e-3, mu
    if case.entropy_penalty == 0 or N > 0:
        assert np.isfinite(loss) and np.isfinite(grad).all()
        assert bool(np.isfinite(float(l32))) and bool(np.isfinite(g32.numpy()).all())


def test_binding_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    for name in ("mi_pu_ge_loss_fwd", "mi_pu_ge_loss_bwd", "mi_pu_ge_loss_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), "missing export " + name
    size = _lib.lib().mi_pu_ge_loss_workspace_bytes
    assert size(0) == 0 and size(1) == 8 * (7 + 6)
    assert size(C.BIG) == 8 * (7 * C.VOX_WGS + 6 * C.COUNT_WGS)
