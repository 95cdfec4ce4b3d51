"""UMAP on the MI355X (csrc/umap.hip) with the constants of the `umap.UMAP(n_neighbors=K, min_dist=m, random_state=seed)` the
reference's plot_2d.py runs:

    um = UMAP(n_neighbors=40, min_dist=0.5, seed=42); y = um.fit_transform(x); um.n_epochs_; um.a_; um.b_

The K - 1 nearest other points of every point by L2 (n_neighbors counts the point itself; hipops.knn_search returns the squared
distance), umap-learn's smooth distances (rho the nearest positive distance, sigma by bisection to log2 K, floored at 1e-3 of
the mean distance), the fuzzy union a + b - a b kept on the directed graph, (a, b) fitted to min_dist by scipy on the host,
500 epochs up to 10000 points and 200 above, every pair sampled every wmax / w epochs, 5 negatives per sample, the learning
rate falling linearly from 1.

Departures from umap-learn:
  1. The epoch is SYNCHRONOUS.  umap-learn moves points in place, pair after pair (and, run in parallel, races on them); here
     every force of an epoch is evaluated from the positions at its start, summed per vertex in a fixed order in double and
     applied once.  The map is then a pure function of (graph, seed): repeated runs give identical bytes, and every term can be
     checked against a float64 restatement.
  2. The start is umap-learn's init="random" (numpy.random.RandomState(seed).uniform(-10, 10, (N, 2))) unless init="spectral" is
     asked for: umap-learn's default, the eigenvectors 1 and 2 of the graph's normalised Laplacian (utils/spectral.py,
     csrc/spectral.hip), scaled to 10 / max|Y|, plus normal(scale=1e-4) noise, every axis then brought to [0, 10].
     Where the eigen-solver does not converge one log line is printed and the random start is used, as umap-learn warns and falls
     back; init_ says which start was used, n_components_ and eigenvalues_ what the solver found.
  3. Exactly 5 negatives per sample (umap-learn's floating-point bookkeeping gives 5, now and then 4 or 6), drawn by
     Philox-4x32-10 from (vertex, incident slot, epoch, seed).
The label-supervised map, `fit_transform(x, y=labels)`, is umap-learn's fit with a categorical target at its
defaults (target_weight 0.5, -1 an unknown label): the weight of a pair is multiplied by exp(-2.5 / (1 - target_weight)) where the
labels of its ends differ (by 0 at target_weight 1) and by exp(-1) where one is unknown, the local connectivity is reset (every
row divided by its largest entry, then the fuzzy union with the transpose), and the spacings, the pruning and the spectral start
are taken from that graph.  Everything after the graph is the plain fit.
2 <= n_neighbors <= 128, N >= n_neighbors + 1.  There is no CPU path.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from .. import hipops as H
from .graph import reverse_graph

N_NEIGHBORS_MIN, N_NEIGHBORS_MAX = 2, 128       # K - 1 <= 127 columns, and the neighbour search's k <= 128
EPOCHS_SMALL, EPOCHS_LARGE, SMALL_N = 500, 200, 10000
INITS = ("random", "spectral")
UNKNOWN_DIST, FAR_DIST_AT_ONE = 1.0, 1.0e12     # umap-learn's categorical intersection: an unknown label, target_weight = 1


def check_range(n, n_neighbors):
    """ValueError outside the supported range, before anything is launched."""
    if int(n_neighbors) != n_neighbors or not N_NEIGHBORS_MIN <= n_neighbors <= N_NEIGHBORS_MAX:
        raise ValueError("n_neighbors must be an integer in %d..%d (the point itself and up to 127 others), got %r"
                         % (N_NEIGHBORS_MIN, N_NEIGHBORS_MAX, n_neighbors))
    if n < n_neighbors + 1:
        raise ValueError("n_neighbors %d needs N >= n_neighbors + 1 = %d points, got %d" % (n_neighbors, n_neighbors + 1, n))


def check_target_weight(target_weight):
    """ValueError unless 0 <= target_weight <= 1 (a NaN is outside)."""
    if not 0.0 <= float(target_weight) <= 1.0:
        raise ValueError("target_weight must be in [0, 1], got %r" % (target_weight,))
    return float(target_weight)


def far_dist(target_weight):
    """umap-learn's distance between two different classes: 2.5 / (1 - target_weight), 1e12 at target_weight 1."""
    return 2.5 / (1.0 - target_weight) if target_weight < 1.0 else FAR_DIST_AT_ONE


def check_labels(y, n):
    """y as a contiguous (N,) int32 numpy array: ValueError for a wrong length, a non-integer dtype or a value below -1 (-1 is
    the unknown label), before anything is launched."""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.dtype.kind not in "iu":
        raise ValueError("y must hold integer class labels (-1: unknown), got dtype %s" % y.dtype)
    if y.shape != (n,):
        raise ValueError("y must have shape (%d,), one label per point, got %s" % (n, y.shape))
    if y.size and (int(y.min()) < -1 or int(y.max()) > 2 ** 31 - 1):
        raise ValueError("labels must be in -1..2^31 - 1 (-1: unknown), got %d..%d" % (int(y.min()), int(y.max())))
    return np.ascontiguousarray(y, dtype=np.int32)


def find_ab_params(min_dist, spread=1.0):
    """umap-learn's curve: (a, b) of 1 / (1 + a x^(2b)) fitted on linspace(0, 3 spread, 300) to 1 below min_dist and
    exp(-(x - min_dist) / spread) above.  Host plumbing; it needs scipy."""
    try:
        from scipy.optimize import curve_fit
    except ImportError as e:
        raise RuntimeError("UMAP fits its curve parameters (a, b) with scipy.optimize.curve_fit, and scipy does not import (%s)"
                           % e) from None
    x = np.linspace(0, spread * 3, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    p, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    return float(p[0]), float(p[1])


class UMAP:
    def __init__(self, n_neighbors, min_dist=0.5, seed=42, n_epochs=None, device="cuda", init="random", spectral_options=None,
                 target_weight=0.5):
        if init not in INITS:
            raise ValueError("init must be one of %s, got %r" % (", ".join(INITS), init))
        self.target_weight = target_weight                  # checked by fit_transform, where y is given
        self.supervised_, self.far_dist_ = False, None
        self.n_neighbors, self.min_dist, self.seed = n_neighbors, float(min_dist), int(seed)
        self.init, self.spectral_options = init, dict(spectral_options or {})      # tol, max_basis, max_restarts of the solver
        self.init_, self.n_components_, self.eigenvalues_ = None, None, None
        self.n_epochs = None if n_epochs is None else int(n_epochs)
        self.device = torch.device(device)
        self.embedding_, self.n_epochs_, self.a_, self.b_ = None, None, None, None

    find_ab_params = staticmethod(find_ab_params)
    check_range = staticmethod(check_range)

    def graph(self, x):
        """(index (N, K) int32, dist (N, K) fp32 squared L2) of x on the device: the search for n_neighbors = K other points.
        The map takes its first K - 1 columns."""
        return H.knn_search(x, x, int(self.n_neighbors), metric="l2", exclude_self=True)

    def fit_transform(self, x, graph=None, y=None):
        """(N, 2) float32 numpy.  graph: (index, dist) of a search already made, with K or K - 1 columns.  y: (N,) integer class
        labels, -1 for an unknown one: the label-supervised map."""
        n = int(x.shape[0])
        check_range(n, self.n_neighbors)
        self.supervised_, self.far_dist_ = y is not None, None
        if y is not None:
            self.far_dist_ = far_dist(check_target_weight(self.target_weight))
            y = check_labels(y, n)
        if self.n_epochs is not None and self.n_epochs < 1:
            raise ValueError("n_epochs must be at least 1, got %d" % self.n_epochs)
        if self.device.type != "cuda":
            raise L.HipExtensionError("UMAP runs on the MI355X (cuda) device; there is no CPU path")
        a, b = find_ab_params(self.min_dist)
        with torch.cuda.device(self.device):
            if graph is None:
                if isinstance(x, np.ndarray):
                    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(n, -1)).to(self.device)
                graph = self.graph(L.require_cuda(x, "x").contiguous())
            elif self.init == "spectral" and isinstance(x, np.ndarray):     # the centres of many components need the data
                x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(n, -1)).to(self.device)
            index, dist = graph
            k = int(self.n_neighbors) - 1
            if index.shape[0] != n or index.shape[1] not in (k, k + 1) or tuple(dist.shape) != tuple(index.shape):
                raise ValueError("graph must have N = %d rows and %d or %d columns, got %s" % (n, k, k + 1, tuple(index.shape)))
            label = None if y is None else torch.from_numpy(y).to(index.device)
            return self._fit(index[:, :k].contiguous(), dist[:, :k].contiguous(), a, b, x, label)

    def setup(self, index, dist, n_epochs, with_wsym=False, label=None):
        """(rev_ptr, rev_edge, mutual, eps) of the graph's K - 1 columns: what the epochs read; with_wsym: and the weights.
        label (N,) int32 on the device: the weights and spacings of the label-supervised graph in their place."""
        n, k = index.shape
        mean_all = float(torch.sqrt(dist).sum(dtype=torch.float64).item()) / (n * (k + 1))
        w = H.umap_smooth_knn(dist, mean_all)[2]
        rev_ptr, rev_edge = reverse_graph(index)
        out = H.umap_union(index, w, rev_ptr, rev_edge, n_epochs)
        wmax = out[0].max().reshape(1)                      # stays on the device
        wsym, mutual, eps = H.umap_union(index, w, rev_ptr, rev_edge, n_epochs, wmax=wmax, out=out)
        if label is not None:
            f_far, f_unknown = math.exp(-far_dist(float(self.target_weight))), math.exp(-UNKNOWN_DIST)     # exp(-1e12) = 0.0
            rowmax = H.umap_rowmax(index, wsym, label, rev_ptr, rev_edge, f_far, f_unknown)
            sup = H.umap_supervise(index, wsym, label, rowmax, f_far, f_unknown, n_epochs)
            wmax = sup[0].max().reshape(1)                  # 1.0 wherever an edge is left; taken from the device all the same
            wsym, eps = H.umap_supervise(index, wsym, label, rowmax, f_far, f_unknown, n_epochs, wmax=wmax, out=sup)
        return (rev_ptr, rev_edge, mutual, eps) + ((wsym,) if with_wsym else ())

    def spectral_start(self, index, wsym, eps, mutual, rev_ptr, rev_edge, x=None):
        """umap-learn's start from the spectral layout, (N, 2) fp32 numpy, or None (and one log line) where the eigen-solver did
        not converge.  Sets n_components_ and eigenvalues_."""
        from .spectral import spectral_layout, umap_start
        Y, info = spectral_layout(index, wsym, eps, mutual, rev_ptr, rev_edge, dim=2, seed=self.seed, x=x, **self.spectral_options)
        self.n_components_, self.eigenvalues_ = info["n_components"], info["eigenvalues"]
        if not info["converged"]:
            print("[cet_pick_amd] UMAP: the spectral start did not converge (%d graph components, %d Lanczos steps, %d restarts); "
                  "using the random start" % (info["n_components"], info["steps"], info["restarts"]))
            return None
        return umap_start(Y.cpu().numpy(), self.seed)

    def _fit(self, index, dist, a, b, x=None, label=None):
        n = index.shape[0]
        n_epochs = self.n_epochs or (EPOCHS_SMALL if n <= SMALL_N else EPOCHS_LARGE)
        y0 = None
        if self.init == "spectral":
            rev_ptr, rev_edge, mutual, eps, wsym = self.setup(index, dist, n_epochs, with_wsym=True, label=label)
            y0 = self.spectral_start(index, wsym, eps, mutual, rev_ptr, rev_edge, x if isinstance(x, torch.Tensor) else None)
        else:
            rev_ptr, rev_edge, mutual, eps = self.setup(index, dist, n_epochs, label=label)
        self.init_ = "random" if y0 is None else "spectral"
        if y0 is None:
            y0 = np.random.RandomState(self.seed % 2 ** 32).uniform(-10, 10, (n, 2)).astype(np.float32)
        y, y2 = torch.from_numpy(y0).to(index.device), torch.empty(n, 2, dtype=torch.float32, device=index.device)
        for epoch in range(1, n_epochs + 1):
            H.umap_epoch(y, y2, index, rev_ptr, rev_edge, mutual, eps, epoch, n_epochs, a, b, self.seed)
            y, y2 = y2, y
        self.n_epochs_, self.a_, self.b_ = n_epochs, a, b
        self.embedding_ = y.cpu().numpy()
        return self.embedding_
