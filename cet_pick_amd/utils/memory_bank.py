"""The reference's `utils/memory_bank.py` on the MI355X: a bank of `n` feature rows with their class targets, and nearest-
neighbour queries against it.  Same constructor, attributes (n, dim, features, targets, ptr, device, K, temperature, C) and
methods; the return shapes and the return order are the reference's.

Every search is `hipops.knn_search` (csrc/knn.hip) with the inner product as metric: the bank x bank similarity matrix of
`mine_nearest_neighbors` (faiss.IndexFlatIP in the reference) and the batch x bank matrix of `weighted_knn` / `knn`
(matmul + topk / argmax in the reference) are never stored.  Equal similarities go to the lowest bank index.  There is no CPU
path: the bank is filled on any device, but a search needs it on the GPU (`bank.cuda()`) and raises HipExtensionError
otherwise.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import hipops as H


class MemoryBank(object):
    def __init__(self, n, dim, num_classes, temperature):
        self.n = n
        self.dim = dim
        self.features = torch.zeros(self.n, self.dim, dtype=torch.float32)
        self.targets = torch.zeros(self.n, dtype=torch.int64)
        self.ptr = 0
        self.device = 'cpu'
        self.K = 100                       # neighbours that vote in weighted_knn
        self.temperature = temperature
        self.C = num_classes

    def _search(self, queries, k):
        """(similarity (B, k) fp32, index (B, k) int64) of the k most similar bank rows, most similar first."""
        if not self.features.is_cuda:
            raise L.HipExtensionError("MemoryBank searches on the MI355X (cuda) device; there is no CPU path: call .cuda() first")
        queries = L.require_cuda(queries, "predictions").detach()
        with torch.cuda.device(self.features.device):
            index, value = H.knn_search(queries.contiguous(), self.features.contiguous(), k, metric="ip")
        return value, index.long()

    def weighted_knn(self, predictions):
        # every one of the K nearest bank rows votes for its class with weight exp(similarity / temperature)
        yd, yi = self._search(predictions, self.K)
        votes = torch.zeros(predictions.shape[0], self.C, dtype=torch.float32, device=yd.device)
        votes.scatter_add_(1, self.targets[yi], (yd / self.temperature).exp())
        _, class_preds = votes.sort(1, True)
        class_pred = class_preds[:, 0]

        return class_pred

    def knn(self, predictions):
        # the class of the single nearest bank row
        _, sample_pred = self._search(predictions, 1)
        class_pred = torch.index_select(self.targets, 0, sample_pred[:, 0])
        return class_pred

    def mine_nearest_neighbors(self, topk, calculate_accuracy=True):
        # the topk nearest neighbours of every bank row; the row itself is searched too: topk + 1 columns
        sims, idx = self._search(self.features, topk + 1)
        indices, distances = idx.cpu().numpy(), sims.cpu().numpy()
        if calculate_accuracy:
            targets = self.targets.cpu().numpy()
            neighbor_targets = np.take(targets, indices[:, 1:], axis=0)        # without the row itself
            accuracy = np.mean(neighbor_targets == targets.reshape(-1, 1))
            return indices, accuracy, distances

        else:
            return indices, distances

    def reset(self):
        self.ptr = 0

    def update(self, features, targets):
        b = features.size(0)

        assert (b + self.ptr <= self.n)

        self.features[self.ptr:self.ptr + b].copy_(features.detach())
        self.targets[self.ptr:self.ptr + b].copy_(targets.detach())
        self.ptr += b

    def to(self, device):
        self.features = self.features.to(device)
        self.targets = self.targets.to(device)
        self.device = device

    def cpu(self):
        self.to('cpu')

    def cuda(self):
        self.to('cuda:0')
