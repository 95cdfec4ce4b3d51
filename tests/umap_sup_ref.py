"""The arbiter of the label-supervised UMAP map, in float64 numpy, written from the text of DESIGN.md 4.16 (umap-learn is not a
dependency): what umap.UMAP.fit_transform(x, y) adds to the plain fit for a categorical target - the intersection with the labels
and the reset of the local connectivity - as a closed form per directed edge, and the same through the scipy.sparse and sklearn
calls umap-learn makes.  Nothing here calls the code under test."""
import numpy as np

import umap_ref as U

UNKNOWN_DIST = 1.0


def far_dist(target_weight):
    """umap-learn's distance between two different classes."""
    return 2.5 / (1.0 - target_weight) if target_weight < 1.0 else 1.0e12


def factors(target_weight):
    """(f_far, f_unknown): what the weight of a pair is multiplied by where the labels of its ends differ / where one is unknown."""
    return float(np.exp(-far_dist(target_weight))), float(np.exp(-UNKNOWN_DIST))


def _edges(index):
    index = np.asarray(index, np.int64)
    n, k = index.shape
    return n, k, np.repeat(np.arange(n), k), index.reshape(-1)


def _factor(li, lj, f_far, f_unknown):
    return np.where((li < 0) | (lj < 0), f_unknown, np.where(li != lj, f_far, 1.0))


def supervise64(index, wsym, label, f_far, f_unknown):
    """(wsup (N, k), rowmax (N,)), float64: s = wsym f per directed edge i -> j, m the largest s over the pairs of every vertex
    (an edge is a pair of both of its ends), wsup = p + q - p q with p = s / (m_i or 1), q = s / (m_j or 1).  An edge that points
    outside [0, N) or at its own row has s = 0."""
    n, k, i, j = _edges(index)
    label = np.asarray(label, np.int64)
    ok = (j >= 0) & (j < n) & (j != i)
    jj = np.where(ok, j, 0)
    s = np.where(ok, np.asarray(wsym, np.float64).reshape(-1) * _factor(label[i], label[jj], f_far, f_unknown), 0.0)
    m = np.zeros(n)
    np.maximum.at(m, i, s)
    np.maximum.at(m, jj, s)
    d = np.where(m > 0, m, 1.0)
    p, q = s / d[i], s / d[jj]
    return (p + q - p * q).reshape(n, k), m


def supervise_sparse64(index, wsym, label, f_far, f_unknown):
    """The same by the calls umap-learn makes: the symmetric CSR graph, fast_intersection's factor on every stored entry,
    sklearn.preprocessing.normalize(norm="max"), T + T.T - T.multiply(T.T), read back per directed edge.  (The edges of `index`
    are in range and not loops here.)"""
    from scipy.sparse import coo_matrix
    from sklearn.preprocessing import normalize
    n, k, i, j = _edges(index)
    label = np.asarray(label, np.int64)
    A = coo_matrix((np.asarray(wsym, np.float64).reshape(-1), (i, j)), shape=(n, n)).tocsr()
    S = A.maximum(A.T).tocoo()                              # an edge and its opposite carry the same weight
    S.data = S.data * _factor(label[S.row], label[S.col], f_far, f_unknown)
    S = S.tocsr()
    S.eliminate_zeros()
    rowmax = np.asarray(S.max(axis=1).todense()).reshape(-1) if S.nnz else np.zeros(n)
    T = normalize(S, norm="max")
    Tt = T.T.tocsr()
    R = (T + Tt - T.multiply(Tt)).tocsr()
    R.eliminate_zeros()
    return np.asarray(R[i, j]).reshape(n, k), rowmax


def graph64(index, dist2, label, n_epochs, target_weight=0.5):
    """umap_ref.graph64 for the supervised map: (inc, eps, wsup fp32) of the first K - 1 columns of a search; the union's and
    the supervised weights are rounded to fp32 where the device stores them."""
    w = U.smooth64(dist2)[2]
    wsym, mutual, _, _ = U.union64(index, w.astype(np.float32), n_epochs)
    wsup = supervise64(index, wsym.astype(np.float32), label, *factors(target_weight))[0].astype(np.float32)
    return U.incident(index, mutual), U.spacing64(wsup, wsup.max(), n_epochs), wsup


def fit64(index, dist2, label, a, b, seed, n_epochs=None, target_weight=0.5):
    """umap_ref.fit64 on the supervised graph (the random start)."""
    n = len(index)
    n_epochs = n_epochs or U.n_epochs_for(n)
    inc, eps, _ = graph64(index, dist2, label, n_epochs, target_weight)
    Y = U.start(n, seed)
    for e in range(1, n_epochs + 1):
        Y = U.epoch64(Y, inc, eps, e, n_epochs, a, b, seed).astype(np.float32)
    return Y
