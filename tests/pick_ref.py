"""Host arbiter and fixtures of the pick grouping and tracing (csrc/pick_groups.hip): scipy's connected components mapped to
smallest-member labels, and the intermediate values of utils/post_process.tomo_fiber_postprocess recomputed with numpy
(numpy.polyfit in float64), component by component.  Nothing here touches the device."""
import warnings

import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components

CUTOFF = 15


def labels_scipy(pts, cutoff):
    """(label, size) int32: the smallest index of each point's component of the graph sqrt(d2) <= cutoff, and its member count."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    lab = connected_components(sparse.csr_matrix(np.sqrt(d2) <= cutoff), directed=False)[1]
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab].astype(np.int32), np.bincount(lab)[lab].astype(np.int32)


def chain(n, seed):
    """n integer points on a line, 10 apart (only consecutive ones are within 15), in a shuffled index order: the graph's
    diameter is n - 1, the long case for label propagation."""
    order = np.random.default_rng(seed).permutation(n)
    pts = np.zeros((n, 3))
    pts[:, 0] = 10.0 * order
    pts[:, 1] = 7.0
    pts[:, 2] = 3.0
    return pts


def blobs(seed=5):
    """three blobs of 8, 3 and 6 integer points (each within a ball of radius 6, centres 100 apart), indices interleaved"""
    rng = np.random.default_rng(seed)
    parts = [np.array(c) + rng.integers(-3, 4, (k, 3)) for c, k in (((50, 60, 40), 8), ((150, 60, 40), 3), ((50, 160, 40), 6))]
    pts = np.concatenate(parts).astype(np.float64)
    return pts[rng.permutation(len(pts))]


# ---- fibre fixtures: integer coordinates [t, u, v], as the detector produces them ------------------------------------------------

def _fibre(t, fu, fv, rng, jitter):
    t = np.asarray(t, np.float64)
    ju = rng.integers(-jitter, jitter + 1, len(t)) if jitter else 0
    jv = rng.integers(-jitter, jitter + 1, len(t)) if jitter else 0
    return np.stack([t, np.rint(fu(t)) + ju, np.rint(fv(t)) + jv], 1)


def fibre_scenes(seed=11):
    """name -> (n, 3) float64 with integer values.  Components of different fibres are more than 15 apart."""
    rng = np.random.default_rng(seed)
    s = {}
    s["line"] = _fibre(30 + 5 * np.arange(20), lambda t: 100.37 + 0.513 * t, lambda t: 60.21 + 0.197 * t, rng, 0)
    s["parabola"] = _fibre(40 + 4 * np.arange(40), lambda t: 200.3 + 0.31 * (t - 118) + 0.0011 * (t - 118) ** 2,
                           lambda t: 90.4 - 0.12 * (t - 118) - 0.0007 * (t - 118) ** 2, rng, 1)
    s["arc"] = _fibre(60 + 2 * np.arange(41), lambda t: 300.2 + 0.021 * (t - 100) ** 2, lambda t: 50.3 + 0.1 * t, rng, 0)
    s["six"] = _fibre(20 + 6 * np.arange(6), lambda t: 40.3 + 0.4 * t, lambda t: 30.1 + 0.1 * t, rng, 1)
    s["seven"] = _fibre(20 + 6 * np.arange(7), lambda t: 40.3 + 0.4 * t, lambda t: 30.1 + 0.1 * t, rng, 1)
    s["two_values"] = np.array([[50 + 6 * (i % 2), 100 + 5 * (i // 2), 30 + (i % 3)] for i in range(8)], np.float64)
    s["flat_span"] = np.array([[80 + (i % 2), 100 + 4 * i, 30 + (i % 2)] for i in range(8)], np.float64)
    a = _fibre(25 + 5 * np.arange(30), lambda t: 120.4 + 0.25 * t, lambda t: 40.2 - 0.05 * t, rng, 1)
    b = _fibre(300 + 6 * np.arange(18), lambda t: 400.6 - 0.3 * (t - 350), lambda t: 140.1 + 0.2 * (t - 350), rng, 1)
    noise = np.array([[600, 20, 20], [640, 300, 90], [10, 500, 200], [700, 700, 10], [333, 30, 222]], np.float64)
    both = np.concatenate([a, b, noise])
    s["two_fibres_noise"] = both[rng.permutation(len(both))]
    # everything in one call, each scene moved 300 further along v
    s["all"] = np.concatenate([p + np.array([0, 0, 300.0 * k]) for k, p in enumerate(s.values())])
    return s


def k_x(y, a, b):
    return np.max((2 * a) / ((1 + (2 * a * y + b) ** 2)) ** (2 / 3))


def fiber_reference(pts, distance_cutoff=CUTOFF, res_cutoff=30, curvature_cutoff=0.03, scale=2):
    """The values tomo_fiber_postprocess computes on its way, one dict per component of more than 6 members in ascending label
    order: label, members, idx (member indices), lo, hi, skipped (m2 == 0), degenerate (t has fewer than 3 distinct values),
    fit_u, fit_v (numpy.polyfit coefficients), res_u, res_v, k_u, k_v, tot, accepted, y_out, u_fit, v_fit, kappa."""
    pts = np.asarray(pts, np.float64)
    label, size = labels_scipy(pts, distance_cutoff)
    out = []
    for lb in np.unique(label):
        idx = np.flatnonzero(label == lb)
        if len(idx) <= 6:
            continue
        t, u, v = pts[idx, 0], pts[idx, 1], pts[idx, 2]
        lo, hi = t.min(), t.max()
        span = hi - lo
        y_range = np.linspace(lo - 1, hi + 1, int(span // 2))
        y_out = np.linspace(lo - 1, hi + 1, int(span // scale))
        c = dict(label=int(lb), members=len(idx), idx=idx, lo=lo, hi=hi, skipped=len(y_range) == 0,
                 degenerate=len(np.unique(t)) < 3, accepted=False, y_out=y_out[:0], u_fit=y_out[:0], v_fit=y_out[:0])
        out.append(c)
        if c["skipped"]:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")            # RankWarning of the degenerate fixture
            fu, fv = np.polyfit(t, u, 2, full=True), np.polyfit(t, v, 2, full=True)
        c["fit_u"], c["fit_v"] = fu[0], fv[0]
        c["res_u"] = fu[1][0] / len(idx) if fu[1].shape[0] > 0 else 10000
        c["res_v"] = fv[1][0] / len(idx) if fv[1].shape[0] > 0 else 10000
        c["k_u"], c["k_v"] = k_x(y_range, fu[0][0], fu[0][1]), k_x(y_range, fv[0][0], fv[0][1])
        tot = c["tot"] = c["res_u"] + c["res_v"]
        ku, kv = abs(c["k_u"]), abs(c["k_v"])
        c["accepted"] = bool((tot < res_cutoff and ku < curvature_cutoff and kv < curvature_cutoff) or
                             (res_cutoff <= tot < res_cutoff * 3 and ku < curvature_cutoff / 10 and kv < curvature_cutoff / 10))
        A = np.vander(t, 3)
        c["kappa"] = np.linalg.cond(A / np.sqrt((A * A).sum(0)))
        if c["accepted"]:
            c["y_out"], c["u_fit"], c["v_fit"] = y_out, np.polyval(fu[0], y_out), np.polyval(fv[0], y_out)
    return out


def assert_margins(comps, res_cutoff=30, curvature_cutoff=0.03):
    """The condition on a fixture: the reference's own values stay clear of every decision they feed - no polyval output within
    1e-6 of an integer, none of tot, |k_u|, |k_v| within a relative 1e-6 of a cutoff it is compared with."""
    for c in comps:
        if c["skipped"]:
            continue
        for val, cuts in ((c["tot"], (res_cutoff, res_cutoff * 3)), (abs(c["k_u"]), (curvature_cutoff, curvature_cutoff / 10)),
                          (abs(c["k_v"]), (curvature_cutoff, curvature_cutoff / 10))):
            for cut in cuts:
                assert abs(val - cut) > 1e-6 * abs(cut), (c["label"], val, cut)
        for f in (c["u_fit"], c["v_fit"]):
            assert (np.abs(f - np.rint(f)) > 1e-6).all(), (c["label"], f[np.abs(f - np.rint(f)) <= 1e-6])
