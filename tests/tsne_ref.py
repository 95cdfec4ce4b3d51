"""The arbiter of the t-SNE tests, in float64 numpy: sklearn's perplexity search, the joint affinities, the exact gradient with
its divergence and per-row error scale, the gains update in float32, and the maker of the test inputs.  Nothing here calls the
code under test."""
import numpy as np

# The longest serial fp32 accumulation chain of csrc/tsne.hip: a tile of 128 points j summed from zero in
# the repulsion kernel.  Tile sums, splits, Z, the attraction and the divergence are added in double.  Never more than N.
L_CHAIN = 128


def band(n):
    """(L + 16) 2^-24: L roundings of the longest fp32 chain, 16 for the operations of one term and a 1-ulp reciprocal."""
    return (min(L_CHAIN, n) + 16) * 2.0 ** -24


def make_blobs(N, d, n_clusters, seed, sep=4.0):
    """x (N, d) float32 in n_clusters Gaussian blobs of unit spread whose centres are `sep` N(0, 1) draws; label (N,) int."""
    rs = np.random.RandomState(seed)
    centres = sep * rs.standard_normal((n_clusters, d))
    label = np.arange(N) % n_clusters
    x = centres[label] + rs.standard_normal((N, d))
    return x.astype(np.float32), label.astype(np.int64)


def entropy_at(dist, beta):
    """(P64 (N, K), H (N,)) of exp(-beta (d - d_min)) / sum per row, in float64 (the row's smallest distance taken off: the
    same distribution, and no row underflows as a whole)."""
    d = np.asarray(dist, np.float64)
    d = d - d.min(1, keepdims=True)
    b = np.asarray(beta, np.float64)[:, None]
    e = np.exp(-d * b)
    s = e.sum(1, keepdims=True)
    P = e / s
    return P, np.log(s[:, 0]) + b[:, 0] * (d * P).sum(1)


def affinities64(dist, perplexity, n_steps=100, tol=1e-5):
    """sklearn's _binary_search_perplexity on every row of dist (N, K): beta from 1, doubled / halved while unbounded, then
    bisected, until |H - ln perplexity| <= tol or n_steps.  -> (P (N, K), beta (N,)), float64."""
    n = len(dist)
    target = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    live = np.ones(n, bool)
    for _ in range(n_steps):
        diff = entropy_at(dist, beta)[1] - target
        live &= np.abs(diff) > tol
        if not live.any():
            break
        up, dn = live & (diff > 0), live & (diff <= 0)
        lo[up] = beta[up]
        hi[dn] = beta[dn]
        with np.errstate(invalid="ignore"):
            beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
            beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2.0, (beta[dn] + lo[dn]) / 2.0)
    return entropy_at(dist, beta)[0], beta


def joint_P(index, pcond, dense=True):
    """P = (P_cond + P_cond^T) / 2N of the graph index (N, K) with conditional affinities pcond (N, K): dense (N, N) float64,
    or the edge list (row, col, value) of its non-zero entries in row-major order."""
    index = np.asarray(index, np.int64)
    n, k = index.shape
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), k), index.reshape(-1)), np.asarray(pcond, np.float64).reshape(-1))
    P = (P + P.T) / (2.0 * n)
    if dense:
        return P
    r, c = np.nonzero(P)
    return r, c, P[r, c]


def grad_kl64(Y, P, exaggeration=1.0):
    """The exact gradient for one degree of freedom, in float64.  -> grad (N, 2) = 4 (exaggeration sum_j P_ij q_ij (y_i - y_j) -
    sum_j q_ij^2 (y_i - y_j) / Z), Z = sum over i != j of q_ij, KL = sum over P > 0 of P ln(P Z / q) (no exaggeration),
    scale (N,) = 4 (exaggeration sum_j P_ij q_ij |y_i - y_j| + sum_j q_ij^2 |y_i - y_j| / Z), klscale = sum P |ln(P Z / q)|."""
    Y = np.asarray(Y, np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    d2 = (diff ** 2).sum(2)
    q = 1.0 / (1.0 + d2)
    np.fill_diagonal(q, 0.0)
    Z = q.sum()
    dist = np.sqrt(d2)
    attr = exaggeration * ((P * q)[:, :, None] * diff).sum(1)
    rep = ((q * q)[:, :, None] * diff).sum(1) / Z
    grad = 4.0 * (attr - rep)
    scale = 4.0 * (exaggeration * (P * q * dist).sum(1) + (q * q * dist).sum(1) / Z)
    m = P > 0
    terms = P[m] * np.log(P[m] * Z / q[m])
    return grad, Z, float(terms.sum()), scale, float(np.abs(terms).sum())


def kl64(Y, P):
    return grad_kl64(Y, P)[2]


def update32(y, grad, velocity, gains, momentum, lr, min_gain=0.01):
    """sklearn's _gradient_descent step in float32, every operation rounded once.  -> (y, velocity, gains), new arrays."""
    f = np.float32
    y, grad, velocity, gains = (np.asarray(a, f) for a in (y, grad, velocity, gains))
    inc = velocity * grad < f(0)
    gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
    gains = np.maximum(gains, f(min_gain))
    velocity = (f(momentum) * velocity - f(lr) * (grad * gains)).astype(f)
    return (y + velocity).astype(f), velocity, gains


def neighbour_agreement(Y, label, k=5):
    """The share of points whose label is the most frequent label (lowest on ties) of their k nearest 2-D neighbours."""
    Y = np.asarray(Y, np.float64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    nn = np.argsort(d2, axis=1, kind="stable")[:, :k]
    votes = np.stack([(label[nn] == c).sum(1) for c in range(int(label.max()) + 1)], 1)
    return float((votes.argmax(1) == label).mean())
