"""The arbiter of the k-means tests: Lloyd's iteration in numpy float64 (expanded-form distances, lowest-index ties, means,
the empty-cluster rule restated from include/cetpick_hip.h) and the maker of the test inputs.  Nothing here calls the code
under test."""
import numpy as np

EPS = 1.0 / 1024.0
CASES = {            # name: (N, d, k, spread)
    "A": (20000, 128, 256, 0.15),
    "B": (20000, 100, 256, 0.15),
    "C": (4099, 32, 48, 0.15),
    "D": (20000, 128, 256, 0.05),
}
BAND_CAP = 0.002     # at most 0.2 % of a case's points may lie in the tie band


def make(N, d, seed=7, spread=0.15, n_dir=48, return_classes=False):
    """48 unit-norm Gaussian directions mu; x = mu[randint(48)] + spread * randn(d), fp32."""
    rs = np.random.RandomState(seed)
    mu = rs.randn(n_dir, d)
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    cls = rs.randint(n_dir, size=N)
    x = (mu[cls] + spread * rs.randn(N, d)).astype(np.float32)
    return (x, cls, mu) if return_classes else x


def init_rows(N, k, seed=1234):
    return np.random.RandomState(seed).permutation(N)[:k]


def band(d):
    """Relative gap below which fp32 cannot be asked for the float64 label: (d + 8) 2^-24."""
    return (d + 8) * 2.0 ** -24


def assign64(x, c, block=8192):
    """float64, expanded form.  -> labels (lowest index on ties), dist (clamped at 0), second (index of the second-best
    centroid), relgap = (second-smallest - smallest) / (|x|^2 + |c_best|^2), scale = |x|^2 + |c_best|^2."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    cn = (c * c).sum(1)
    n = x.shape[0]
    labels, second = np.empty(n, np.int64), np.empty(n, np.int64)
    dist, gap, scale = np.empty(n), np.empty(n), np.empty(n)
    for s in range(0, n, block):
        xb = x[s:s + block]
        xn = (xb * xb).sum(1)
        D = xn[:, None] + (cn[None, :] - 2.0 * (xb @ c.T))
        l = np.argmin(D, axis=1)                     # the first minimum: lowest index
        r = np.arange(len(l))
        best = D[r, l]
        D2 = D.copy()
        D2[r, l] = np.inf
        l2 = np.argmin(D2, axis=1)
        labels[s:s + block], second[s:s + block] = l, l2
        dist[s:s + block] = np.maximum(best, 0.0)
        scale[s:s + block] = xn + cn[l]
        gap[s:s + block] = (D2[r, l2] - best) / np.maximum(xn + cn[l], 1e-300)
    return labels, dist, second, gap, scale


def means64(x, labels, k, prev):
    """Per-cluster count and float64 mean; an empty cluster keeps its row of `prev`."""
    x = np.asarray(x, np.float64)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, labels, x)
    cent = np.array(prev, dtype=np.float64, copy=True)
    nz = counts > 0
    cent[nz] = sums[nz] / counts[nz, None]
    return cent, counts


def split_rule(cent, counts, eps=EPS):
    """Empty clusters in ascending index; donor = most points at that moment (lowest index on ties); the empty cluster takes
    the donor's centroid, component m times 1 + eps (m even) / 1 - eps (m odd), the donor the opposite; of the donor's n
    points the empty cluster takes n // 2, the donor keeps n - n // 2.  -> cent, counts, [(empty, donor), ...]"""
    cent, counts = np.array(cent, dtype=np.float64, copy=True), np.array(counts, dtype=np.int64, copy=True)
    sign = np.where(np.arange(cent.shape[1]) % 2 == 0, 1.0, -1.0)
    served = []
    for e in range(len(counts)):
        if counts[e] != 0:
            continue
        donor = int(np.argmax(counts))               # the first maximum: lowest index
        c = cent[donor].copy()
        cent[e] = c * (1.0 + eps * sign)
        cent[donor] = c * (1.0 - eps * sign)
        n = int(counts[donor])
        counts[e], counts[donor] = n // 2, n - n // 2
        served.append((e, donor))
    return cent, counts, served


def lloyd_step(x, c):
    """One iteration from centroids c: -> new centroids (float64), counts after the splits, labels, dist, served."""
    labels, dist, _, _, _ = assign64(x, c)
    cent, counts = means64(x, labels, len(c), c)
    cent, counts, served = split_rule(cent, counts)
    return cent, counts, labels, dist, served


def lloyd(x, c, niter):
    c = np.asarray(c, np.float64)
    objs = []
    for _ in range(niter):
        c, counts, labels, dist, _ = lloyd_step(x, c)
        objs.append(dist.sum())
    return c, np.array(objs)


def check_assign(x, c, got_labels, got_dist, what="", cap=BAND_CAP):
    """Check 1 of the issue.  x (N, d) fp32 and c (k, d) fp32 are what the device was given.  Prints the figures, then asserts:
    the tie band holds <= cap of the points (on the float64 data, before the device's labels are looked at); outside the band
    the label is the float64 argmin exactly, inside it is the best or the second-best; dist within
    2 (d + 8) 2^-24 (|x|^2 + |c|^2) of float64."""
    d = x.shape[1]
    labels, dist, second, gap, scale = assign64(x, c)
    inband = gap < band(d)
    share = float(inband.mean())
    assert share <= cap, "%s: %.4f %% of the points in the tie band (cap %.2f %%)" % (what, 100 * share, 100 * cap)
    got_labels = np.asarray(got_labels).astype(np.int64).ravel()
    got_dist = np.asarray(got_dist, np.float64).ravel()
    wrong_out = int((got_labels[~inband] != labels[~inband]).sum())
    differ_in = int((got_labels[inband] != labels[inband]).sum())
    bad_in = int(((got_labels != labels) & (got_labels != second) & inband).sum())
    derr = np.abs(got_dist - dist) / np.maximum(scale, 1e-300)
    print("%s: N=%d d=%d k=%d band share %.4f %% (%d points, %d differ), outside band wrong %d, dist err max %.3e (bound %.3e)"
          % (what, x.shape[0], d, c.shape[0], 100 * share, int(inband.sum()), differ_in, wrong_out, float(derr.max()),
             2 * band(d)))
    assert wrong_out == 0, "%s: %d labels outside the tie band differ from float64" % (what, wrong_out)
    assert bad_in == 0, "%s: %d labels inside the tie band are neither best nor second-best" % (what, bad_in)
    assert float(derr.max()) <= 2 * band(d), "%s: dist error %.3e of |x|^2+|c|^2, bound %.3e" % (what, float(derr.max()), 2 * band(d))
    return labels, dist
