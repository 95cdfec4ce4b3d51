"""The arbiter of the UMAP tests, in float64 numpy, written from the text of DESIGN.md 4.14 (umap-learn is not a dependency):
the smooth-distance search, the fuzzy union kept on the directed graph, the incident-pair lists, one epoch-synchronous step
with its per-vertex term counts and error scale, the whole fit, the sequential in-place loop the synchronous form stands in
for (used by the golden generator only), and the curve fit.  Nothing here calls the code under test."""
import numpy as np

import augment_ref as A

NEGATIVES = 5
CLIP = 4.0


def band64(n_terms):
    """(n_terms + 64) 2^-53: one rounding per term of a double sum, and 64 for the ~20 double operations of one term plus
    an allowance for a device `pow` / `exp` that is a few ulp off numpy's."""
    return (n_terms + 64) * 2.0 ** -53


def n_epochs_for(n):
    return 500 if n <= 10000 else 200


def find_ab(min_dist, spread=1.0):
    """umap-learn's find_ab_params: 1 / (1 + a x^(2b)) fitted to 1 below min_dist, exp(-(x - min_dist) / spread) above."""
    from scipy.optimize import curve_fit
    x = np.linspace(0, spread * 3, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    p, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    return float(p[0]), float(p[1])


def distances(dist2):
    """d = sqrt of the squared distances, rounded to float32 as the device holds it, as float64."""
    return np.sqrt(np.asarray(dist2, np.float64)).astype(np.float32).astype(np.float64)


def smooth64(dist2, mean_all=None):
    """dist2 (N, K - 1) squared distances to the K - 1 nearest other points (n_neighbors = K counts the point itself).
    -> (rho (N,), sigma (N,), w (N, K - 1)), float64."""
    d = distances(dist2)
    n, k1 = d.shape
    K = k1 + 1
    target = np.log2(K)
    if mean_all is None:
        mean_all = d.sum() / (n * K)
    rho, sigma = np.zeros(n), np.zeros(n)
    for i in range(n):
        row = d[i]
        pos = row[row > 0]
        r = pos.min() if len(pos) else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        for _ in range(64):
            g = row - r
            with np.errstate(over="ignore"):                   # g / mid past the largest double: exp(-inf) = 0
                s = np.where(g > 0, np.exp(-g / mid), 1.0).sum()
            if abs(s - target) < 1e-5:
                break
            if s > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        floor = 1e-3 * (row.sum() / K if r > 0 else mean_all)
        rho[i], sigma[i] = r, max(mid, floor)
    w = np.exp(-np.maximum(0.0, d - rho[:, None]) / sigma[:, None])
    return rho, sigma, w


def reverse_lists(index):
    """(rev_ptr (N + 1,), rev_edge (N K,)): the ids of the edges that end in row r, ascending."""
    index = np.asarray(index, np.int64)
    n = index.shape[0]
    dest = index.reshape(-1)
    order = np.argsort(dest, kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(dest, minlength=n))
    return ptr, order


def union64(index, w, n_epochs, wmax=None):
    """Per directed edge: wsym = a + b - a b (a the edge's weight, b the opposite edge's or 0), mutual, and the spacing
    eps = wmax / wsym, +inf where wsym < wmax / n_epochs.  wmax: the largest wsym unless given."""
    index = np.asarray(index, np.int64)
    w = np.asarray(w, np.float64)
    n, k = index.shape
    opp = {}
    for i in range(n):
        for c in range(k):
            opp[(i, int(index[i, c]))] = w[i, c]
    wsym, mutual = np.zeros((n, k)), np.zeros((n, k), bool)
    for i in range(n):
        for c in range(k):
            j = int(index[i, c])
            b = opp.get((j, i))
            mutual[i, c] = b is not None
            a = w[i, c]
            b = 0.0 if b is None else b
            wsym[i, c] = a + b - a * b
    if wmax is None:
        wmax = wsym.max()
    return wsym, mutual, spacing64(wsym, wmax, n_epochs), wmax


def spacing64(wsym, wmax, n_epochs):
    wsym = np.asarray(wsym, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = float(wmax) / wsym
    return np.where(wsym < float(wmax) / n_epochs, np.inf, eps)


def incident(index, mutual):
    """The incident pairs of every vertex as flat arrays (vertex, slot, other, edge), vertex-major: the vertex's forward
    edges in column order, then the edges that end in it and have no opposite edge, in ascending edge id; slot counts
    from 0 within the vertex.  A pair {i, j} is in the list of i once and in the list of j once."""
    index = np.asarray(index, np.int64)
    n, k = index.shape
    ptr, rev = reverse_lists(index)
    mflat = np.asarray(mutual, bool).reshape(-1)
    vert, slot, other, edge = [], [], [], []
    for i in range(n):
        s = 0
        for c in range(k):
            vert.append(i); slot.append(s); other.append(int(index[i, c])); edge.append(i * k + c)
            s += 1
        for e in rev[ptr[i]:ptr[i + 1]]:
            if not mflat[e]:
                vert.append(i); slot.append(s); other.append(int(e) // k); edge.append(int(e))
                s += 1
    return tuple(np.array(v, np.int64) for v in (vert, slot, other, edge))


def fires(n, eps):
    """An incident pair with spacing eps fires at epoch n (from 1) iff floor(n / eps) > floor((n - 1) / eps)."""
    eps = np.asarray(eps, np.float64)
    return np.floor(n / eps) > np.floor((n - 1) / eps)


def negatives(vert, slot, n, n_points, seed):
    """(len(vert), 5) int64: the negative samples of (vertex, slot, epoch n)."""
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    v, s = np.asarray(vert, np.uint64), np.asarray(slot, np.uint64)
    words = []
    for q in range((NEGATIVES + 3) // 4):
        words += list(A.philox4x32_10(v, s, np.uint64(n), np.uint64(q), k0, k1))
    words = np.stack(words[:NEGATIVES], 1)
    return ((words * np.uint64(n_points)) >> np.uint64(32)).astype(np.int64)


def _attraction(d2, a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        c = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
    return np.where(d2 > 0, c, 0.0)


def _repulsion(d2, a, b):
    return 2.0 * b / ((0.001 + d2) * (a * d2 ** b + 1.0))


def epoch_terms64(Y, inc, eps, n, n_epochs, a, b, seed):
    """One synchronous epoch from the positions Y (N, 2).  -> (y_new (N, 2) float64 = Y + alpha acc, not rounded,
    n_terms (N,) the number of terms added into the vertex's accumulator, abs_terms (N, 2) the sum of their magnitudes)."""
    Y = np.asarray(Y, np.float64)
    N = len(Y)
    vert, slot, other, edge = inc
    f = fires(n, np.asarray(eps, np.float64).reshape(-1)[edge])
    vert, slot, other = vert[f], slot[f], other[f]
    acc, abs_terms, n_terms = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N, np.int64)
    diff = Y[vert] - Y[other]
    d2 = (diff ** 2).sum(1)
    t = 2.0 * np.clip(_attraction(d2, a, b)[:, None] * diff, -CLIP, CLIP)
    np.add.at(acc, vert, t)
    np.add.at(abs_terms, vert, np.abs(t))
    np.add.at(n_terms, vert, 1)
    neg = negatives(vert, slot, n, N, seed)
    for q in range(NEGATIVES):
        k = neg[:, q]
        diff = Y[vert] - Y[k]
        d2 = (diff ** 2).sum(1)
        t = np.clip(_repulsion(d2, a, b)[:, None] * diff, -CLIP, CLIP)
        t = np.where((d2 == 0)[:, None], CLIP, t)
        live = k != vert
        np.add.at(acc, vert[live], t[live])
        np.add.at(abs_terms, vert[live], np.abs(t[live]))
        np.add.at(n_terms, vert[live], 1)
    alpha = 1.0 - (n - 1.0) / n_epochs
    return Y + alpha * acc, n_terms, abs_terms


def epoch64(Y, inc, eps, n, n_epochs, a, b, seed):
    return epoch_terms64(Y, inc, eps, n, n_epochs, a, b, seed)[0]


def start(n, seed):
    """umap-learn's init="random"."""
    return np.random.RandomState(seed).uniform(-10, 10, (n, 2)).astype(np.float32)


def graph64(index, dist2, n_epochs):
    """(inc, eps) of the first K - 1 columns of a search for K neighbours."""
    w = smooth64(dist2)[2]
    wsym, mutual, eps, _ = union64(index, w.astype(np.float32), n_epochs)
    return incident(index, mutual), spacing64(wsym.astype(np.float32), np.float32(wsym.max()), n_epochs)


def fit64(index, dist2, a, b, seed, n_epochs=None):
    """The epoch-synchronous fit; positions are rounded to float32 at the end of every epoch, as the device stores them."""
    n = len(index)
    n_epochs = n_epochs or n_epochs_for(n)
    inc, eps = graph64(index, dist2, n_epochs)
    Y = start(n, seed)
    for e in range(1, n_epochs + 1):
        Y = epoch64(Y, inc, eps, e, n_epochs, a, b, seed).astype(np.float32)
    return Y


def sequential_fit64(index, dist2, a, b, seed, n_epochs=None):
    """umap-learn's loop: the entries (vertex, slot) in order, every firing moves both ends of its pair in place, then the
    vertex by its five negatives, each from the positions as they are at that moment.  Same schedule, same negatives."""
    n = len(index)
    n_epochs = n_epochs or n_epochs_for(n)
    inc, eps = graph64(index, dist2, n_epochs)
    vert, slot, other, edge = inc
    eps = eps.reshape(-1)[edge]
    Y = start(n, seed).astype(np.float64)
    ys = [[float(p[0]), float(p[1])] for p in Y]
    clip = lambda v: 4.0 if v > 4.0 else (-4.0 if v < -4.0 else v)                   # noqa: E731
    for e in range(1, n_epochs + 1):
        alpha = 1.0 - (e - 1.0) / n_epochs
        f = np.nonzero(fires(e, eps))[0]
        neg = negatives(vert[f], slot[f], e, n, seed).tolist()
        for (i, j), ks in zip(zip(vert[f].tolist(), other[f].tolist()), neg):
            yi, yj = ys[i], ys[j]
            dx, dy = yi[0] - yj[0], yi[1] - yj[1]
            d2 = dx * dx + dy * dy
            if d2 > 0:
                c = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
                gx, gy = clip(c * dx) * alpha, clip(c * dy) * alpha
                yi[0] += gx; yi[1] += gy; yj[0] -= gx; yj[1] -= gy
            for k in ks:
                if k == i:
                    continue
                yk = ys[k]
                dx, dy = yi[0] - yk[0], yi[1] - yk[1]
                d2 = dx * dx + dy * dy
                if d2 > 0:
                    c = 2.0 * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                    yi[0] += clip(c * dx) * alpha; yi[1] += clip(c * dy) * alpha
                else:
                    yi[0] += 4.0 * alpha; yi[1] += 4.0 * alpha
    return np.array(ys)
