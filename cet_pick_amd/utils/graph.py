"""The directed k-nearest-neighbour graph the t-SNE, UMAP and spectral kernels share (csrc/knn_graph.h):
index (N, K) int32 holds the forward edges, edge e = i K + c running from i to index[e]; reverse_graph makes its transpose."""
import torch


def reverse_graph(index):
    """(rev_ptr (N + 1,) int32, rev_edge (N K,) int32) of index (N, K): the ids e = i K + c of the edges whose destination
    index[e] is row r are rev_edge[rev_ptr[r] : rev_ptr[r + 1]], in ascending order.  CPU or device tensors."""
    n, k = index.shape
    if n * k >= 2 ** 31:
        raise ValueError("N K = %d edges do not fit int32 edge ids" % (n * k))
    dest = index.reshape(-1).to(torch.int64)
    if n * k and (int(dest.min()) < 0 or int(dest.max()) >= n):
        raise ValueError("index holds rows outside [0, %d)" % n)
    order = torch.sort(dest, stable=True)[1]
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=index.device)
    ptr[1:] = torch.cumsum(torch.bincount(dest, minlength=n), 0)
    return ptr.to(torch.int32), order.to(torch.int32)
