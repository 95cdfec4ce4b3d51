"""How good a clustering of the picks is (this project's own; the reference judges classes by eye in its interactive session;
csrc/cluster_quality.hip):

    silhouette(x, labels, class_of=None)     the exact silhouette of every pick (scikit-learn's silhouette_samples, Euclidean)
    SilhouetteSums(x, fine_labels, k)        the pass over the N x N pairs, made once; .score(class_of) for any merge of the k fine
                                             clusters - a sweep over class counts pays for the pairs once
    compare_labelings(a, b)                  contingency table, adjusted Rand index, normalised mutual information

The distances, their sums and the per-pick figures are made on the MI355X; there is no CPU path (a bank that is not on the GPU
raises HipExtensionError).  ARI and NMI are host arithmetic in float64 on the integer table.
"""
import numpy as np

from .. import _lib as L


class Silhouette:
    """s, a, b (N,) float64, nearest (N,) int32, class_mean (C,) float64 (NaN: no member), class_count (C,) int32, mean (float),
    confusion (C, C) int32 [own][nearest]: numpy arrays, picks in input order."""
    KEYS = ("s", "a", "b", "nearest", "class_mean", "class_count", "mean", "confusion")

    def __init__(self, out):
        for key in self.KEYS:
            setattr(self, key, out[key].cpu().numpy())
        self.mean = float(self.mean)

    def arrays(self, prefix=""):
        """the fields as a dict for np.savez, keys prefixed"""
        return {prefix + key: np.asarray(getattr(self, key)) for key in self.KEYS}


def _bank(x, device=None):
    """x as the kernels take it: (N, d) fp32, contiguous, on the GPU (a numpy array goes to `device`, which must be a GPU)."""
    import torch
    if isinstance(x, np.ndarray):
        if device is None or torch.device(device).type != "cuda":
            raise L.HipExtensionError("the embeddings are a host array and no MI355X (cuda) device was named; there is no CPU path")
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    L.require_cuda(x, "x")
    return x


def _labels(labels, device):
    import torch
    if isinstance(labels, torch.Tensor):
        return labels.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(device)


class SilhouetteSums:
    """The distance sums of every pick to every one of k fine clusters, kept on the device ((N, k) float64)."""

    def __init__(self, x, fine_labels, k, device=None):
        from .. import hipops as H
        x = _bank(x, device)
        self.k = int(k)
        self.labels = _labels(fine_labels, x.device)
        self.sums = H.silhouette_sums(x, self.labels, self.k)

    def score(self, class_of=None):
        """The silhouette of the classes class_of[fine label] ((k,) ints; None: the fine clusters themselves).  A merged class's
        sum is the sum of its fine columns, so its figures agree with a direct run on the merged labels to rounding (the order of
        the float64 additions differs), not to the bit."""
        from .. import hipops as H
        if class_of is not None:
            class_of = _labels(class_of, self.sums.device)
            if tuple(class_of.shape) != (self.k,):
                raise ValueError("class_of must name a class for each of the %d fine clusters, got %s" % (self.k, tuple(class_of.shape)))
        return Silhouette(H.silhouette_finalise(self.sums, self.labels, class_of))


def silhouette(x, labels, class_of=None, device=None):
    """The silhouette of the picks x (N, d) under `labels` (N,) ints >= 0 (ids without a pick are empty classes and ignored), or
    under class_of[labels]."""
    import torch
    x = _bank(x, device)
    lab = _labels(labels, x.device)
    if lab.numel() == 0 or tuple(lab.shape) != (x.shape[0],):
        raise ValueError("labels must be (%d,), got %s" % (x.shape[0], tuple(lab.shape)))
    lo, hi = (int(v) for v in torch.aminmax(lab))
    if lo < 0:
        raise ValueError("labels holds %d; classes are numbered from 0" % lo)
    return SilhouetteSums(x, lab, hi + 1).score(class_of)


def ari_nmi(table):
    """(adjusted Rand index, normalised mutual information) of a contingency table of counts, float64 on the host: sklearn's
    adjusted_rand_score (pair counts in exact integers) and normalized_mutual_info_score with its arithmetic-mean normaliser."""
    t = [[int(v) for v in row] for row in np.asarray(table)]
    n = sum(sum(row) for row in t)
    ra, rb = [sum(row) for row in t], [sum(col) for col in zip(*t)]
    pairs = sum(v * (v - 1) // 2 for row in t for v in row)           # exact integers: n^2 passes 2^53 only beyond 9 10^7 picks
    pa, pb, pn = sum(v * (v - 1) // 2 for v in ra), sum(v * (v - 1) // 2 for v in rb), n * (n - 1) // 2
    # sklearn's form on the pair confusion matrix (tn, fp, fn, tp), each counted twice there; the factor cancels
    tp, fp, fn = pairs, pb - pairs, pa - pairs
    tn = pn - tp - fp - fn
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp * tn - fn * fp) / float((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    nz_a, nz_b = sum(v > 0 for v in ra), sum(v > 0 for v in rb)
    if nz_a == 1 and nz_b == 1:
        return ari, 1.0                                   # sklearn: two one-class labelings agree
    p = np.asarray(t, np.float64)
    i, j = np.nonzero(p)
    v = p[i, j]
    fa, fb = np.asarray(ra, np.float64), np.asarray(rb, np.float64)
    terms = v / n * (np.log(v) - np.log(n)) + v / n * (-np.log(fa[i] * fb[j]) + 2.0 * np.log(n))
    mi = max(float(np.sum(np.where(np.abs(terms) < np.finfo(np.float64).eps, 0.0, terms))), 0.0)
    if mi <= np.finfo(np.float64).eps:
        return ari, 0.0
    ha = -float(np.sum([c / n * (np.log(c) - np.log(n)) for c in fa if c > 0]))
    hb = -float(np.sum([c / n * (np.log(c) - np.log(n)) for c in fb if c > 0]))
    return ari, mi / max(0.5 * (ha + hb), np.finfo(np.float64).eps)


class Comparison:
    """table (Ca, Cb) int64: picks per (class of a, class of b), the classes of each labeling in ascending order of their ids
    (ids_a, ids_b); ari, nmi floats."""

    def __init__(self, table, ids_a, ids_b):
        self.table, self.ids_a, self.ids_b = table, ids_a, ids_b
        self.ari, self.nmi = ari_nmi(table)


def compare_labelings(a, b, device="cuda"):
    """Two labelings of the same picks (any integer ids, -1 included: an id is a class): the table counted on the device."""
    import torch
    from .. import hipops as H
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if len(a) != len(b) or len(a) == 0:
        raise ValueError("the labelings name %d and %d picks" % (len(a), len(b)))
    if torch.device(device).type != "cuda":
        raise L.HipExtensionError("the contingency table is counted on the MI355X (cuda) device; there is no CPU path")
    ids_a, ia = np.unique(a, return_inverse=True)
    ids_b, ib = np.unique(b, return_inverse=True)
    ta = torch.from_numpy(ia.astype(np.int32)).to(device)
    tb = torch.from_numpy(ib.astype(np.int32)).to(device)
    table = H.label_contingency(ta, tb, len(ids_a), len(ids_b)).cpu().numpy()
    return Comparison(table, ids_a, ids_b)


def parse_sweep(text):
    """--sweep_n_cluster "4,8,16": the class counts of a sweep, each >= 2, in the order given, none twice."""
    try:
        vals = [int(v) for v in str(text).split(",") if v.strip()]
    except ValueError:
        raise ValueError("--sweep_n_cluster takes comma-separated integers, got %r" % (text,)) from None
    if not vals:
        raise ValueError("--sweep_n_cluster names no class count: %r" % (text,))
    if min(vals) < 2:
        raise ValueError("--sweep_n_cluster: a clustering has at least 2 classes, got %d" % min(vals))
    if len(set(vals)) != len(vals):
        raise ValueError("--sweep_n_cluster names a class count twice: %r" % (text,))
    return vals
