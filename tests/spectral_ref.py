"""The arbiter of the spectral-start tests, in float64 numpy, written from the text of DESIGN.md 4.15 (umap-learn is not a
dependency): the graph's dense weight matrix from the union of umap_ref, its components by scipy, the eigenvectors of the
normalised Laplacian by a dense numpy.linalg.eigh, the sign rule, the placement of several components and the start umap-learn
builds from the layout.  Nothing here calls the code under test."""
import numpy as np

import umap_ref as U

MAX_COMPONENTS = 256


def dense_w(index, wsym, eps):
    """W (N, N) float64, symmetric: wsym of every directed edge with a finite spacing, on both of its matrix entries (an edge
    and its opposite carry the same wsym).  Pruned edges (eps = +inf) are left out, as umap-learn zeroes them before its layout."""
    index = np.asarray(index, np.int64)
    n, k = index.shape
    wsym, eps = np.asarray(wsym, np.float64).reshape(n, k), np.asarray(eps, np.float64).reshape(n, k)
    W = np.zeros((n, n))
    for i in range(n):
        for c in range(k):
            j = int(index[i, c])
            if np.isfinite(eps[i, c]) and 0 <= j < n and j != i:
                W[i, j] = W[j, i] = wsym[i, c]
    return W


def graph_tables(index, dist2, n_epochs):
    """(wsym fp32, mutual, eps) of the first K - 1 columns of a search, as the device holds them: umap_ref's smooth distances and
    union, wsym rounded to fp32 and the spacings from the rounded values."""
    w = U.smooth64(dist2)[2].astype(np.float32)
    wsym, mutual, _, _ = U.union64(index, w, n_epochs)
    wsym = wsym.astype(np.float32)
    return wsym, mutual, U.spacing64(wsym, wsym.max(), n_epochs)


def components(W):
    """(N,) int64: the smallest vertex id of every vertex's connected component."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    _, lab = connected_components(csr_matrix(W > 0), directed=False)
    first = np.full(lab.max() + 1, len(W), np.int64)
    np.minimum.at(first, lab, np.arange(len(W)))
    return first[lab]


def normalised(W):
    """A = D^-1/2 W D^-1/2 and deg; an isolated vertex gets a zero row."""
    deg = W.sum(1)
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return W * dis[:, None] * dis[None, :], deg


def sign_rule(v):
    """v turned so that its entry of largest magnitude is positive; ties go to the lowest index."""
    v = np.asarray(v, np.float64)
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def eigenpairs(W, dim):
    """(lam (n,) ascending eigenvalues of L = I - A, vec (n, dim) the signed eigenvectors 1..dim, gap (dim,) the distance of each
    of those eigenvalues to the rest of the spectrum)."""
    A, _ = normalised(W)
    lam, vec = np.linalg.eigh(np.eye(len(W)) - A)
    v = np.stack([sign_rule(vec[:, a]) for a in range(1, dim + 1)], 1)
    gap = np.array([min(lam[a] - lam[a - 1], lam[a + 1] - lam[a]) for a in range(1, dim + 1)])
    return lam, v, gap


def fixed_centres(c, dim):
    k = int(np.ceil(c / 2.0))
    base = np.hstack([np.eye(k), np.zeros((k, dim - k))])
    return np.vstack([base, -base])[:c]


def eigh_centres(centroids, dim):
    z = np.asarray(centroids, np.float64)
    d2 = ((z[:, None] - z[None]) ** 2).sum(2)
    aff = np.exp(-d2)
    dis = 1.0 / np.sqrt(aff.sum(1))
    lam, vec = np.linalg.eigh(np.eye(len(z)) - aff * dis[:, None] * dis[None, :])
    e = np.stack([sign_rule(vec[:, a]) for a in range(1, dim + 1)], 1)
    return e / np.abs(e).max(), lam


def centres_of(c, dim, centroids=None):
    return fixed_centres(c, dim) if c <= 2 * dim else eigh_centres(centroids, dim)[0]


def data_ranges(centres):
    d = np.sqrt(((centres[:, None] - centres[None]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    return d.min(1) / 2.0


def layout(W, dim=2, seed=42, x=None):
    """(Y (N, dim) float64, info): labels, sizes, centres, data_range, scale, and per large component lam, gap."""
    n = len(W)
    lab = components(W)
    ids = np.unique(lab)
    c = len(ids)
    members = [np.nonzero(lab == l)[0] for l in ids]
    info = dict(labels=lab, n_components=c, sizes=np.array([len(m) for m in members]), lam={}, gap={})
    Y = np.zeros((n, dim))
    if c == 1:
        lam, v, gap = eigenpairs(W, dim)
        info.update(lam={0: lam}, gap={0: gap}, centres=np.zeros((1, dim)), data_range=np.array([np.inf]), scale=np.ones(1))
        return v, info
    centroids = None if c <= 2 * dim else np.stack([np.asarray(x, np.float64)[m].mean(0) for m in members])
    centres = centres_of(c, dim, centroids)
    ranges = data_ranges(centres)
    rs = np.random.RandomState(seed)
    scale = np.ones(c)
    for a, m in enumerate(members):
        if len(m) < max(2 * dim, dim + 2):
            Y[m] = rs.uniform(-ranges[a], ranges[a], (len(m), dim)) + centres[a]
            continue
        lam, v, gap = eigenpairs(W[np.ix_(m, m)], dim)
        info["lam"][a], info["gap"][a] = lam, gap
        scale[a] = ranges[a] / np.abs(v).max()
        Y[m] = v * scale[a] + centres[a]
    info.update(centres=centres, data_range=ranges, scale=scale)
    return Y, info


def start(Y, seed):
    """umap-learn's simplicial_set_embedding on a spectral layout: scaled to 10 / max|Y| as fp32, plus normal(scale=1e-4) noise as
    fp32, then every axis to [0, 10] as fp32."""
    Y = np.asarray(Y, np.float64)
    y = (Y * (10.0 / np.abs(Y).max())).astype(np.float32)
    y = y + np.random.RandomState(seed).normal(scale=1e-4, size=Y.shape).astype(np.float32)
    return (10.0 * (y - y.min(0)) / (y.max(0) - y.min(0))).astype(np.float32)


def strip(n, seed, d=32, noise=0.01, offset=0.0):
    """n points uniform on a 3 x 1 strip, pushed through a random 2 -> d linear map, plus noise: (x (n, d) fp32, the strip's
    coordinates (n, 2))."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(0, 1, (n, 2)) * np.array([3.0, 1.0])
    m = rs.standard_normal((2, d))
    x = p @ m + noise * rs.standard_normal((n, d))
    x[:, 0] += offset
    return x.astype(np.float32), p


def knn(x, k):
    """(index (N, k) int64, dist2 (N, k) fp32): the k nearest other rows by squared L2 in float64, lowest index on ties."""
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None] - x[None]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    index = np.argsort(d2, 1, kind="stable")[:, :k]
    return index, np.take_along_axis(d2, index, 1).astype(np.float32)


def fit64_from(index, dist2, a, b, seed, y0, n_epochs):
    """umap_ref.fit64 from a given start."""
    inc, eps = U.graph64(index, dist2, n_epochs)
    Y = np.asarray(y0, np.float32)
    for e in range(1, n_epochs + 1):
        Y = U.epoch64(Y, inc, eps, e, n_epochs, a, b, seed).astype(np.float32)
    return Y
