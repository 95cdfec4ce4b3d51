"""Exact t-SNE on the MI355X (csrc/tsne.hip) with the schedule of the `sklearn.manifold.TSNE` the reference's plot_2d.py runs:

    ts = TSNE(perplexity=30, n_iter=1000, seed=42); y = ts.fit_transform(x); ts.kl_divergence_; ts.n_iter_

K = min(N - 1, 3 perplexity + 1) nearest neighbours by squared L2 (hipops.knn_search, self excluded), conditional affinities
by sklearn's binary search, P = (P_cond + P_cond^T) / 2N kept on the graph; learning rate max(N / early_exaggeration / 4, 50);
250 iterations with the exaggeration and momentum 0.5, then momentum 0.8; gains as sklearn's; every 50 iterations the
divergence and the gradient norm are read back, and the descent stops on a norm <= 1e-7 or after 300 iterations (250 in
the exaggerated stage) without progress.

Differences from sklearn: the gradient is the EXACT one (all pairs; sklearn's default is Barnes-Hut with
angle 0.5), the start is sklearn's init="random" (numpy.random.RandomState(seed).standard_normal((N, 2)) * 1e-4; the PCA
init is not built), the divergence read back is always the one without the exaggeration, and kl_divergence_ belongs to the
returned embedding (sklearn reports the one before the last step).  Integer perplexity 2..42, N >= perplexity + 2.  There is
no CPU path.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import hipops as H
from .graph import reverse_graph          # its home; kept importable from here

PERPLEXITY_MIN, PERPLEXITY_MAX = 2, 42          # K = 3 perplexity + 1 <= 127 fits the neighbour search's k <= 128
N_ITER_CHECK, EXPLORATION_ITER, MIN_GRAD_NORM = 50, 250, 1e-7


def n_neighbors(n, perplexity):
    """sklearn's neighbour count for the affinities: min(N - 1, 3 perplexity + 1)."""
    return int(min(n - 1, 3 * perplexity + 1))


def check_range(n, perplexity):
    """ValueError outside the supported range, before anything is launched."""
    if int(perplexity) != perplexity or not PERPLEXITY_MIN <= perplexity <= PERPLEXITY_MAX:
        raise ValueError("perplexity must be an integer in %d..%d (K = 3 perplexity + 1 <= 127 neighbours), got %r"
                         % (PERPLEXITY_MIN, PERPLEXITY_MAX, perplexity))
    if n < perplexity + 2:
        raise ValueError("perplexity %d needs N >= perplexity + 2 = %d points, got %d" % (perplexity, perplexity + 2, n))


class TSNE:
    def __init__(self, perplexity, n_iter=1000, seed=42, early_exaggeration=12.0, learning_rate="auto", device="cuda"):
        self.perplexity, self.n_iter, self.seed = perplexity, int(n_iter), int(seed)
        self.early_exaggeration, self.learning_rate = float(early_exaggeration), learning_rate
        self.device = torch.device(device)
        self.n_split = 0                   # parts of the all-pairs sum (0: chosen from N)
        self.kl_divergence_, self.n_iter_, self.embedding_ = None, None, None

    def graph(self, x):
        """(index (N, K) int32, dist (N, K) fp32) of x on the device: the neighbours the affinities are made from."""
        return H.knn_search(x, x, n_neighbors(x.shape[0], self.perplexity), metric="l2", exclude_self=True)

    def fit_transform(self, x, graph=None):
        """(N, 2) float32 numpy.  graph: (index, dist) of a search already made with K = n_neighbors(N, perplexity)."""
        n = int(x.shape[0])
        check_range(n, self.perplexity)
        if self.n_iter < EXPLORATION_ITER:
            raise ValueError("n_iter must be at least %d, got %d" % (EXPLORATION_ITER, self.n_iter))
        if self.device.type != "cuda":
            raise L.HipExtensionError("TSNE runs on the MI355X (cuda) device; there is no CPU path")
        with torch.cuda.device(self.device):
            if graph is None:
                if isinstance(x, np.ndarray):
                    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(n, -1)).to(self.device)
                graph = self.graph(L.require_cuda(x, "x").contiguous())
            index, dist = graph
            if tuple(index.shape) != (n, n_neighbors(n, self.perplexity)):
                raise ValueError("graph must have K = %d columns, got %s" % (n_neighbors(n, self.perplexity), tuple(index.shape)))
            return self._fit(index.contiguous(), dist.contiguous())

    def _fit(self, index, dist):
        n, k = index.shape
        dev = index.device
        p, _ = H.tsne_affinities(dist, self.perplexity)
        rev_ptr, rev_edge = reverse_graph(index)
        lr = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)
        y0 = np.random.RandomState(self.seed).standard_normal((n, 2)).astype(np.float32) * np.float32(1e-4)
        y = torch.from_numpy(y0).to(dev)
        ws = H.tsne_workspace(n, k, self.n_split, dev)
        grad = torch.empty(n, 2, dtype=torch.float32, device=dev)
        z, kl = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)

        def descend(first, last, exaggeration, momentum, patience):
            vel, gains = torch.zeros_like(y), torch.ones_like(y)
            best, best_it, i = float("inf"), first, first
            for i in range(first, last):
                check = (i + 1) % N_ITER_CHECK == 0
                H.tsne_gradient(y, index, p, rev_ptr, rev_edge, exaggeration, self.n_split, kl=check, out=(grad, z, kl), ws=ws)
                if check:                                           # the only read-backs of the descent
                    err, gnorm = float(kl.item()), float(torch.linalg.norm(grad).item())
                H.tsne_update(y, grad, vel, gains, momentum, lr)
                if check:
                    if err < best:
                        best, best_it = err, i
                    elif i - best_it > patience:
                        break
                    if gnorm <= MIN_GRAD_NORM:
                        break
            return i

        it = descend(0, EXPLORATION_ITER, self.early_exaggeration, 0.5, EXPLORATION_ITER)
        if self.n_iter > EXPLORATION_ITER:
            it = descend(it + 1, self.n_iter, 1.0, 0.8, 300)
        H.tsne_gradient(y, index, p, rev_ptr, rev_edge, 1.0, self.n_split, kl=True, out=(grad, z, kl), ws=ws)
        self.kl_divergence_, self.n_iter_ = float(kl.item()), int(it)
        self.embedding_ = y.cpu().numpy()
        return self.embedding_
