"""The arbiter of the cluster-quality tests: the silhouette in float64 by direct differences, in row chunks (never
an N x N x d array), the finalise formula restated, the accuracy bounds computed from the inputs alone, and the makers of the
seeded inputs.  Nothing here calls the code under test or scikit-learn (tests/golden/gen_golden_cluster_quality.py does, once, and
tests/test_cluster_quality_cpu.py holds this file against what it stored)."""
import os

import numpy as np

from kmeans_ref import band  # band(d) = (d + 8) 2^-24: the rowdot parity bound of tests/knn_ref.py

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_quality", "small.npz")

# name: (N, d, class sizes or number of classes, spread, seed)
CASES = {
    "ragged": (1003, 17, 7, 0.15, 11),                         # ragged k-step, scalar loads, N % 32 != 0
    "tail": (1500, 100, 5, 0.5, 12),                           # vector loads with a tail
    "sizes": (829, 32, (1, 33, 64, 200, 31, 500), 0.05, 13),   # a singleton, a tile boundary, exact tiles
    "chunks": (2600, 24, (2100, 300, 200), 0.3, 14),           # the largest class: 66 column tiles = three chunks of 32 tiles
}
VARIANTS = ("ragged", "tail", "sizes", "gaps", "chunks")       # gaps: "ragged" with ids 3 c + 1 (the other ids are empty classes)


def make(name):
    """x (N, d) fp32 blobs around random centres and labels (N,) int32 = the blob of every pick, picks in random order."""
    gaps = name == "gaps"
    n, d, classes, spread, seed = CASES["ragged" if gaps else name]
    rs = np.random.RandomState(seed)
    if isinstance(classes, int):
        labels = rs.randint(0, classes, n)
        c = classes
    else:
        assert sum(classes) == n
        labels = rs.permutation(np.repeat(np.arange(len(classes)), classes))
        c = len(classes)
    centres = rs.randn(c, d)
    x = (centres[labels] + spread * rs.randn(n, d)).astype(np.float32)
    labels = labels.astype(np.int32)
    return x, (labels * 3 + 1 if gaps else labels)


def second_labeling(labels, seed=5):
    """A labeling to compare with `labels`: a fifth of the picks moved to a random other class, one pick in ten marked -1."""
    rs = np.random.RandomState(seed)
    ids = np.unique(labels)
    other = ids[rs.randint(0, len(ids), len(labels))]
    out = np.where(rs.rand(len(labels)) < 0.2, other, labels)
    return np.where(rs.rand(len(labels)) < 0.1, -1, out).astype(np.int32)


def distance_sums(x, labels, k, rows=16):
    """S (N, k) float64: S[i][c] = sum over the members j != i of cluster c of |x_i - x_j|, by direct differences; and E (N, k):
    the bound on the device's error in S[i][c] - per pair e = 2 band(d) (|x_i|^2 + |x_j|^2) on the squared distance, so
    min(sqrt(e), e / delta) on the distance delta."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    onehot = np.zeros((n, k))
    onehot[np.arange(n), labels] = 1.0
    sq = (x * x).sum(1)
    S, E = np.empty((n, k)), np.empty((n, k))
    for s in range(0, n, rows):
        r = np.arange(s, min(s + rows, n))
        diff = x[r, None, :] - x[None, :, :]
        dist = np.sqrt((diff * diff).sum(2))
        e = 2.0 * band(d) * (sq[r, None] + sq[None, :])
        with np.errstate(divide="ignore"):
            eb = np.minimum(np.sqrt(e), e / dist)
        dist[np.arange(len(r)), r] = 0.0
        eb[np.arange(len(r)), r] = 0.0
        S[r] = dist @ onehot
        E[r] = eb @ onehot
    return S, E


def finalise(S, labels, class_of=None):
    """The formula of mi_silhouette_finalise in float64: dict of s, a, b, nearest, count (C,), cs (N, C) class sums, own (N,)."""
    n, k = S.shape
    class_of = np.arange(k) if class_of is None else np.asarray(class_of)
    C = int(class_of.max()) + 1
    fine = np.bincount(labels, minlength=k)
    cs, count = np.zeros((n, C)), np.zeros(C, np.int64)
    for f in range(k):                                         # ascending fine index
        cs[:, class_of[f]] += S[:, f]
        count[class_of[f]] += fine[f]
    own = class_of[labels]
    i = np.arange(n)
    n_own = count[own]
    a = np.where(n_own > 1, cs[i, own] / np.maximum(n_own - 1, 1), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        other = np.where(count[None, :] > 0, cs / count[None, :], np.inf)
    other[i, own] = np.inf
    nearest = other.argmin(1)                                  # the lowest index on a tie
    b = other[i, nearest]
    big = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where((n_own > 1) & (big > 0), (b - a) / big, 0.0)
    return dict(s=s, a=a, b=b, nearest=nearest.astype(np.int32), count=count, cs=cs, own=own, other=other)


def silhouette64(x, labels):
    """(S, E, finalise(S, labels)) for labels in [0, max + 1)."""
    S, E = distance_sums(x, labels, int(labels.max()) + 1)
    return S, E, finalise(S, labels)


def bounds(E, fin, class_of=None):
    """From the sum bounds E (N, k) and the float64 figures: ea (N,) on a, eb (N,) on b (the largest bound over the other
    classes), es (N,) = 2 (ea + eb) / max(a, b) on s (0 where s is 0 by definition), and `decided` (N,): the float64 gap between
    the two smallest candidates for b exceeds 2 eb - there `nearest` must be the arbiter's."""
    n, k = E.shape
    class_of = np.arange(k) if class_of is None else np.asarray(class_of)
    count, own = fin["count"], fin["own"]
    ce = np.zeros((n, len(count)))
    for f in range(k):
        ce[:, class_of[f]] += E[:, f]
    i = np.arange(n)
    ea = np.where(count[own] > 1, ce[i, own] / np.maximum(count[own] - 1, 1), 0.0)
    mean_e = np.where(count[None, :] > 0, ce / np.maximum(count[None, :], 1), 0.0)
    mean_e[i, own] = 0.0
    eb = mean_e.max(1)
    big = np.maximum(fin["a"], fin["b"])
    es = np.where((count[own] > 1) & (big > 0), 2.0 * (ea + eb) / np.where(big > 0, big, 1.0), 0.0)
    two = np.sort(fin["other"], axis=1)[:, :2]
    decided = (two[:, 1] - two[:, 0]) > 2.0 * eb
    return ea, eb, es, decided


def contingency(a, b):
    """(table, ids of a, ids of b): picks per pair of classes, classes in ascending id."""
    ia, xa = np.unique(a, return_inverse=True)
    ib, xb = np.unique(b, return_inverse=True)
    t = np.zeros((len(ia), len(ib)), np.int64)
    np.add.at(t, (xa, xb), 1)
    return t, ia, ib
