"""Float64 numpy restatement of label spreading as csrc/label_spread.hip computes it (Zhou et al. 2004), the named
inputs of its tests and the bounds those tests hold the device to.  Nothing here runs on a GPU or reads the product's code.

    knn_exact      the directed k-NN graph of an embedding, float64, ties by index; dist rounded to fp32 as knn_graph.npz holds it
    weights        the edge weights from (index, fp32 dist)
    sym_csr        the symmetric list of every vertex (forward edges in column order, then the lone reverse edges in source order),
                   w_sym = max of the two directions, deg, val = w_sym (dis_i dis_j)
    dense          S as an (N, N) matrix
    sweep, iterate, closed_form, decide, seed_nearest
"""
import numpy as np

U = 2.0 ** -53                            # unit roundoff of float64


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def knn_exact(x, k):
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(d2, order, 1)
    return order.astype(np.int32), dist.astype(np.float32)


def blobs(n, c, d=8, spread=0.35, sep=2.0, seed=0):
    """n points around c centres (point i in blob i % c), the centres `sep` apart on a simplex-like random layout"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((c, d)) * sep
    blob = np.arange(n) % c
    return centres[blob] + spread * rng.standard_normal((n, d)), blob


def make(name):
    """-> dict(index (N, K) i32, dist (N, K) f32, C, seed_index, seed_class, blob (N,)) of a named variant"""
    shapes = {"v257": (257, 5, 2), "v300c3": (300, 15, 3), "v300c5": (300, 15, 5), "v130": (130, 7, 64), "k1": (200, 1, 2),
              "k70": (200, 70, 2), "hub": (150, 4, 3), "split": (200, 6, 2), "dup": (200, 3, 2)}
    n, k, c = shapes[name]
    seed = sorted(shapes).index(name) + 11
    if name == "v130":                                     # 64 classes on 4 blobs: seeds 0..127, class i % 64
        x, blob = blobs(n, 4, seed=seed)
        seed_index, seed_class = np.arange(128), np.arange(128) % 64
    elif name == "split":                                  # two blobs far apart; both classes are seeded inside blob 0 only
        x, blob = blobs(n, 2, sep=40.0, seed=seed)
        x[blob == 0, 0] += np.where(np.arange((blob == 0).sum()) % 2 == 0, -0.6, 0.6)
        zero = np.flatnonzero(blob == 0)
        seed_index, seed_class = zero[:6], np.arange(6) % 2
    elif name == "dup":                                    # 30 points four times each (d2 = 0, s = 0), then 80 of their own
        rng = np.random.default_rng(seed)
        base, blob30 = blobs(30, c, seed=seed)
        tail, blob80 = blobs(80, c, seed=seed)             # the same centres
        tail = tail + 0.05 * rng.standard_normal(tail.shape)
        x, blob = np.concatenate([np.repeat(base, 4, 0), tail]), np.concatenate([np.repeat(blob30, 4), blob80])
        seed_index = np.concatenate([np.flatnonzero(blob == b)[[0, 5, -1, -2]] for b in range(c)])
        seed_class = blob[seed_index]
    else:
        x, blob = blobs(n, c, seed=seed)
        seed_index = np.concatenate([np.flatnonzero(blob == b)[:3] for b in range(c)])
        seed_class = blob[seed_index]
    index, dist = knn_exact(x, k)
    if name == "hub":                                      # every row lists vertex 0 (row 0 itself: an edge that is passed over)
        index[:, 0] = 0
        dist[:, 0] = ((x - x[0]) ** 2).sum(1).astype(np.float32)
        for i in range(1, n):                              # no row lists 0 twice
            twice = np.flatnonzero(index[i, 1:] == 0) + 1
            for col in twice:
                free = [j for j in range(1, n) if j != i and j not in index[i]]
                index[i, col] = free[0]
                dist[i, col] = np.float32(((x[i] - x[free[0]]) ** 2).sum())
    return dict(name=name, x=x, index=index, dist=dist, C=c, seed_index=np.asarray(seed_index, np.int64),
                seed_class=np.asarray(seed_class, np.int64), blob=blob)


VARIANTS = ("v257", "v300c3", "v300c5", "v130", "k1", "k70", "hub", "split", "dup")
# variants on which (asserted from this file alone) at most 1 % of the picks are undecided against the closed form
DECISION_VARIANTS = ("v257", "v300c3", "v300c5", "k70", "hub")


# ---- the restatement --------------------------------------------------------------------------------------------------------

def valid_edges(index):
    n = index.shape[0]
    return (index >= 0) & (index < n) & (index != np.arange(n)[:, None])


def weights(index, dist, mode):
    """(w (N, K) float64, s (N,) float64, t (N, K) float64 = the exponent d2 / sqrt(s_i s_j), 0 where none is formed)"""
    ok = valid_edges(index)
    n, k = index.shape
    if mode == 0:
        return ok.astype(np.float64), np.zeros(n), np.zeros((n, k))
    d2 = np.asarray(dist, np.float64)
    s = np.where(np.isfinite(d2), d2, 0.0).max(1).clip(min=0.0)
    j = np.where(ok, index, 0)
    q = np.sqrt(s[:, None] * s[j])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(q > 0, np.maximum(d2, 0.0) / np.where(q > 0, q, 1.0), 0.0)
    w = np.where(q > 0, np.exp(-t), (d2 <= 0).astype(np.float64))
    w = np.where(ok & np.isfinite(d2), w, 0.0)
    return w, s, np.where(ok & (q > 0), t, 0.0)


def weights_bound(w, t):
    """|device - w| at most this.  The device forms sqrt(s_i) sqrt(s_j) (two square roots within 1 ulp = 2^-23 each, a product
    within 2^-24), the quotient within 2^-24, so its exponent is t (1 + e), |e| <= 3 2^-23, which moves exp(-t) by the factor
    exp(-t e): relative 3 t 2^-23 (1 + small); fp32 exp adds 1 ulp of its result (2^-23 relative), the comparison value's own
    rounding to fp32 nothing (w is kept in float64).  A result below the normal range is allowed one denormal step, 2^-149."""
    return w * ((3.0 * t + 2.0) * 2.0 ** -23) * 1.001 + 2.0 ** -149


def sym_csr(index, w):
    """row_ptr (N + 1,) i64, col (nnz,) i32, wsym (nnz,) f64, deg (N,) f64, val (nnz,) f64 from index and the forward weights w"""
    n, k = index.shape
    ok = valid_edges(index)
    w = np.asarray(w, np.float64)
    fwd = [dict() for _ in range(n)]                       # fwd[i][j] = w_ij of the first valid edge i -> j
    for i in range(n):
        for c in range(k):
            if ok[i, c]:
                fwd[i].setdefault(int(index[i, c]), w[i, c])
    incoming = [[] for _ in range(n)]                      # the sources of the edges that end in i, ascending edge id
    for i in range(n):
        for c in range(k):
            if ok[i, c]:
                incoming[int(index[i, c])].append((i, w[i, c]))
    row_ptr, col, wsym = [0], [], []
    for i in range(n):
        for c in range(k):
            if ok[i, c]:
                j = int(index[i, c])
                col.append(j)
                wsym.append(max(w[i, c], fwd[j].get(i, 0.0)))
        for j, wji in incoming[i]:
            if i not in fwd[j] or j in fwd[i]:
                continue                                   # (a mutual pair is listed among the forward edges)
            col.append(j)
            wsym.append(max(wji, 0.0))
        row_ptr.append(len(col))
    row_ptr, col, wsym = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(wsym, np.float64)
    deg = np.array([wsym[row_ptr[i]:row_ptr[i + 1]].sum() for i in range(n)], np.float64)
    return row_ptr, col, wsym, deg, normalise(row_ptr, col, wsym, deg)


def normalise(row_ptr, col, wsym, deg):
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    rows = np.repeat(np.arange(len(deg)), np.diff(row_ptr))
    return wsym * (dis[rows] * dis[col])


def dense(row_ptr, col, val):
    n = len(row_ptr) - 1
    S = np.zeros((n, n), np.float64)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    np.add.at(S, (rows, col), val)
    return S


def one_hot(n, seed_index, seed_class, c):
    y = np.zeros((n, c), np.float64)
    y[seed_index, seed_class] = 1.0
    return y


def sweep(S, F, Y, alpha):
    return alpha * (S @ F) + (1.0 - alpha) * Y


def iterate(S, Y, alpha, tol, max_iter=100000):
    F = Y.copy()
    for it in range(1, max_iter + 1):
        G = sweep(S, F, Y, alpha)
        res = np.abs(G - F).max()
        F = G
        if res <= tol:
            break
    return F, it, res


def closed_form(S, Y, alpha):
    return (1.0 - alpha) * np.linalg.solve(np.eye(len(S)) - alpha * S, Y)


def decide(F, min_conf):
    """label (argmax, ties to the lowest class; -1 where the mass is 0 or conf < min_conf), conf, mass (the classes added in
    ascending order)"""
    F = np.asarray(F, np.float64)
    mass = F[:, 0].copy()
    for c in range(1, F.shape[1]):
        mass = mass + F[:, c]
    arg = F.argmax(1)                                      # numpy: the first maximum
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = np.where(mass > 0, F[np.arange(len(F)), arg] / np.where(mass > 0, mass, 1.0), 0.0)
    label = np.where((mass > 0) & (conf >= min_conf), arg, -1).astype(np.int32)
    return label, conf, mass


def seed_nearest(picks, pick_tomo, seeds, seed_tomo, radius):
    picks, seeds = np.asarray(picks, np.float64), np.asarray(seeds, np.float64)
    pick, dist = np.full(len(seeds), -1, np.int32), np.full(len(seeds), np.inf)
    for s in range(len(seeds)):
        d = picks - seeds[s]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = np.where(np.asarray(pick_tomo) == seed_tomo[s], d2, np.inf)
        i = int(np.argmin(d2))                             # the first minimum
        if np.isfinite(d2[i]):
            dist[s] = np.sqrt(d2[i])
            pick[s] = i if dist[s] <= radius else -1
    return pick, dist


def planted(seed=5):
    """three well-separated blobs of 90 picks, two seeds each; (x, blob, index, dist, seed_index, seed_class), K = 6"""
    x, blob = blobs(270, 3, spread=0.3, sep=30.0, seed=seed)
    index, dist = knn_exact(x, 6)
    seed_index = np.concatenate([np.flatnonzero(blob == b)[[1, 7]] for b in range(3)])
    return x, blob, index, dist, seed_index, blob[seed_index]


# ---- bounds -----------------------------------------------------------------------------------------------------------------

def longest_row(row_ptr):
    return int(np.diff(row_ptr).max())


def closed_form_bound(n, c, m, alpha, residual, n_seeds, delta=0.0):
    """|F_t - F*| elementwise, F* the closed form: the iteration stopped at max |F_t - F_(t-1)| = residual is within
    alpha / (1 - alpha) sqrt(n c) residual in the 2-norm (|alpha S|_2 <= alpha); a sweep's rounding, (m + 4) 2^-53 relative per
    element of values <= 1, enters the contraction as sqrt(n c) (m + 4) 2^-53 / (1 - alpha); the dense solve behind F* (condition
    (1 + alpha) / (1 - alpha)) is given 64 n 2^-53 of that condition.  delta > 0: S itself is known only to the relative error
    2 delta per entry (fp32 weights: twice the largest relative weight bound), which moves F* by at most
    alpha / (1 - alpha) 2 delta |Y|_F, |Y|_F = sqrt(n_seeds)."""
    k = alpha / (1.0 - alpha)
    return (k * np.sqrt(n * c) * residual + np.sqrt(n * c) * (m + 4) * U / (1.0 - alpha)
            + (1.0 + alpha) / (1.0 - alpha) * 64 * n * U + k * 2.0 * delta * np.sqrt(n_seeds))


def weight_delta(t):
    """the largest relative bound of weights_bound over the edges (the denormal step left out: no variant has such a weight)"""
    return float(((3.0 * t + 2.0) * 2.0 ** -23 * 1.001).max())
