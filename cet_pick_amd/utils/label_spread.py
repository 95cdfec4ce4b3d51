"""Spread a few hand labels over the neighbour graph (this project's stand-in for selecting picks by hand in the reference's
interactive session; csrc/label_spread.hip): label spreading of Zhou et al. 2004, "Learning with local and global
consistency", as scikit-learn's LabelSpreading states it.

    spread_graph(index, dist, edge_weight)   the symmetric, degree-normalised graph S in CSR form, on the device, built once
    spread(graph, seed_index, seed_class, n_classes, alpha, tol, max_iter, check_every)
                                             F <- alpha S F + (1 - alpha) Y from F = Y, Y one-hot on the seeds
    decide(F, min_conf)                      label, confidence and mass per pick
    match_seeds(coords, tomo, seeds, seed_tomo, radius)   the nearest pick of every seed within its tomogram

Everything runs on the MI355X; there is no CPU path (host arrays with no GPU named raise HipExtensionError).
"""
import numpy as np

from .. import _lib as L

EDGE_WEIGHTS = {"binary": 0, "gauss": 1}


class SpreadGraph:
    """row_ptr (N + 1,) int64, col (nnz,) int32, val (nnz,) float64, deg (N,) float64, w (N, K) fp32: device tensors."""

    def __init__(self, row_ptr, col, val, deg, w, edge_weight):
        self.row_ptr, self.col, self.val, self.deg, self.w, self.edge_weight = row_ptr, col, val, deg, w, edge_weight
        self.n = row_ptr.shape[0] - 1
        self.device = row_ptr.device


def _device_tensor(a, dtype, device, what):
    """a as a contiguous tensor of `dtype` on the GPU (a host array goes to `device`, which must be a GPU)."""
    import torch
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a.to(dtype).contiguous()
    if device is None or torch.device(device).type != "cuda":
        raise L.HipExtensionError("%s is a host array and no MI355X (cuda) device was named; there is no CPU path" % what)
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def check_index(index):
    """The host refusals of reverse_graph, before anything reaches the device: N K < 2^31 and every row inside [0, N)."""
    shape = tuple(index.shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("index must be (N, K) with N, K >= 1, got %s" % (shape,))
    n, k = shape
    if n * k >= 2 ** 31:
        raise ValueError("N K = %d edges do not fit int32 edge ids" % (n * k))
    lo, hi = int(index.min()), int(index.max())
    if lo < 0 or hi >= n:
        raise ValueError("index holds rows outside [0, %d)" % n)
    return n, k


def spread_graph(index, dist=None, edge_weight="gauss", device=None):
    """The graph of label spreading from the k-NN graph index (N, K), dist (N, K) squared L2 (knn_graph.npz): edge weights
    ("binary": 1 per edge; "gauss": exp(-d2 / sqrt(s_i s_j)), s_i the squared distance to row i's last neighbour), made symmetric by
    the larger of the two directions, normalised by the square roots of the degrees."""
    import torch
    from .. import hipops as H
    from .graph import reverse_graph
    if edge_weight not in EDGE_WEIGHTS:
        raise ValueError("edge_weight must be one of %s, got %r" % (sorted(EDGE_WEIGHTS), edge_weight))
    if edge_weight == "gauss" and dist is None:
        raise ValueError("edge_weight gauss needs the graph's distances (dist); a graph without them takes edge_weight binary")
    check_index(index)
    if dist is not None and tuple(dist.shape) != tuple(index.shape):
        raise ValueError("dist is %s, index %s" % (tuple(dist.shape), tuple(index.shape)))
    index = _device_tensor(index, torch.int32, device, "index")
    with torch.cuda.device(index.device):
        d = _device_tensor(dist, torch.float32, index.device, "dist") if edge_weight == "gauss" else None
        w, _ = H.spread_weights(index, d, EDGE_WEIGHTS[edge_weight])
        rev_ptr, rev_edge = reverse_graph(index)
        row_ptr, col, val, deg = H.spread_csr(index, rev_ptr, rev_edge, w)
    return SpreadGraph(row_ptr, col, val, deg, w, edge_weight)


def seed_matrix(n, seed_index, seed_class, n_classes):
    """Y (n, n_classes) float64 on the host, one-hot on the seeds.  A seed named twice with one class counts once; with two
    classes it is a ValueError."""
    seed_index = np.asarray(seed_index, np.int64).ravel()
    seed_class = np.asarray(seed_class, np.int64).ravel()
    if len(seed_index) != len(seed_class) or len(seed_index) == 0:
        raise ValueError("seed_index and seed_class name %d and %d seeds" % (len(seed_index), len(seed_class)))
    if seed_index.min() < 0 or seed_index.max() >= n:
        raise ValueError("seed_index names a pick outside 0..%d" % (n - 1))
    if seed_class.min() < 0 or seed_class.max() >= n_classes:
        raise ValueError("seed_class holds a class outside 0..%d" % (n_classes - 1))
    first = {}
    for i, c in zip(seed_index.tolist(), seed_class.tolist()):
        if first.setdefault(i, c) != c:
            raise ValueError("pick %d is a seed of class %d and of class %d" % (i, first[i], c))
    y = np.zeros((n, n_classes), np.float64)
    y[seed_index, seed_class] = 1.0
    return y


def spread(graph, seed_index, seed_class, n_classes, alpha=0.9, tol=1e-6, max_iter=1000, check_every=10):
    """F <- alpha S F + (1 - alpha) Y from F = Y until max |F_new - F| <= tol, read from the device every `check_every` sweeps, or
    `max_iter` sweeps (one log line, no error).  -> F (N, n_classes) float64 on the device, n_iter, residual (the last one read)."""
    import torch
    from .. import hipops as H
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must be in (0, 1), got %g" % alpha)
    if max_iter < 1 or check_every < 1:
        raise ValueError("max_iter and check_every must be >= 1, got %d and %d" % (max_iter, check_every))
    n_classes = int(n_classes)
    y = torch.from_numpy(seed_matrix(graph.n, seed_index, seed_class, n_classes)).to(graph.device)
    with torch.cuda.device(graph.device):
        f, g = y.clone(), torch.empty_like(y)
        word = torch.zeros(1, dtype=torch.int64, device=graph.device)
        n_iter, residual = 0, float("inf")
        while n_iter < max_iter:
            n_iter += 1
            look = n_iter % check_every == 0 or n_iter == max_iter
            H.spread_step(graph.row_ptr, graph.col, graph.val, alpha, f, y, g, word if look else None)
            f, g = g, f
            if look:
                residual = float(word.view(torch.float64).cpu()[0])
                if residual <= tol:
                    break
        else:
            print("[cet_pick_amd] label_spread: stopped at max_iter = %d sweeps with residual %.3g > tol %.3g"
                  % (max_iter, residual, tol))
    return f, n_iter, residual


def decide(F, min_conf):
    """label (N,) int32 (-1: no seed reaches the pick, or its confidence is below min_conf), conf, mass (N,) float64: device
    tensors."""
    from .. import hipops as H
    import torch
    if not isinstance(F, torch.Tensor) or not F.is_cuda:
        raise L.HipExtensionError("F is not on the MI355X (cuda) device; there is no CPU path")
    with torch.cuda.device(F.device):
        return H.spread_decide(F.contiguous(), min_conf)


def match_seeds(coords, tomo, seeds, seed_tomo, radius, device=None):
    """pick (M,) int32, dist (M,) float64 as numpy arrays: for every seed (M, 3) the nearest pick (N, 3) with the same tomogram id,
    -1 where none lies within `radius`."""
    import torch
    from .. import hipops as H
    p = _device_tensor(coords, torch.float64, device, "coords")
    with torch.cuda.device(p.device):
        pick, dist = H.seed_nearest(p, _device_tensor(tomo, torch.int32, p.device, "tomo"),
                                    _device_tensor(seeds, torch.float64, p.device, "seeds"),
                                    _device_tensor(seed_tomo, torch.int32, p.device, "seed_tomo"), radius)
        return pick.cpu().numpy(), dist.cpu().numpy()
