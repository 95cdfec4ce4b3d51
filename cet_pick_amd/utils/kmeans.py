"""Lloyd's k-means on the MI355X (csrc/kmeans.hip), with the interface of the `faiss.Kmeans` the reference's plot_2d.py uses:

    km = Kmeans(d, 256, niter=300, seed=1234); km.train(x); D, I = km.assign(x); km.centroids; km.obj

Differences from faiss: it trains on ALL points (faiss subsamples to 256 per centroid;
`max_points_per_centroid=` restores that), an empty cluster is refilled by a deterministic split of the largest cluster
(faiss draws the donor at random), and ties go to the lowest centroid index.  There is no CPU path.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import hipops as H


class Kmeans:
    def __init__(self, d, k, niter=300, seed=1234, max_points_per_centroid=None, device="cuda"):
        self.d, self.k, self.niter, self.seed = int(d), int(k), int(niter), int(seed)
        self.max_points_per_centroid = max_points_per_centroid
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HipExtensionError("Kmeans runs on the MI355X (cuda) device; there is no CPU path")
        self.centroids_dev = None          # (k, d) device tensor
        self.counts = None                 # (k,) int32, of the last iteration (after the empty-cluster splits)
        self.obj = np.zeros(0, np.float32)
        self.n_split = 0                   # empty clusters served over the whole fit
        self.iteration_hook = None         # tests: called with (iteration, self, centroids, counts) after every iteration (it may synchronise)

    @property
    def centroids(self):
        return None if self.centroids_dev is None else self.centroids_dev.cpu().numpy()

    def _device_x(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)       # copied once
        x = L.require_cuda(x, "x")
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError("x must be (N, %d), got %s" % (self.d, tuple(x.shape)))
        return x.contiguous()

    def train(self, x, init=None):
        x = self._device_x(x)
        n = x.shape[0]
        rs = np.random.RandomState(self.seed)
        if init is None:
            rows = rs.permutation(n)[:self.k]
            cent = x[torch.from_numpy(rows).to(self.device)].clone()
        else:
            cent = torch.as_tensor(np.asarray(init, dtype=np.float32) if not isinstance(init, torch.Tensor) else init)
            cent = cent.to(self.device, torch.float32).contiguous().clone()
            if tuple(cent.shape) != (self.k, self.d):
                raise ValueError("init must be (%d, %d), got %s" % (self.k, self.d, tuple(cent.shape)))
        if self.max_points_per_centroid is not None and n > self.k * int(self.max_points_per_centroid):
            keep = rs.permutation(n)[:self.k * int(self.max_points_per_centroid)]
            x = x[torch.from_numpy(np.sort(keep)).to(self.device)].contiguous()
            n = x.shape[0]
        dev = x.device
        ws = H.kmeans_workspace(n, self.d, self.k, dev)
        image = H.kmeans_prep(cent)
        xnorm = H.kmeans_xnorm(x)                                  # once per fit
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        counts = torch.empty(self.k, dtype=torch.int32, device=dev)
        obj = torch.zeros(max(self.niter, 1), dtype=torch.float32, device=dev)
        nsplit = torch.zeros(1, dtype=torch.int32, device=dev)
        slots = [obj[i:i + 1] for i in range(self.niter)]
        # the iterations: launches on one stream, nothing comes back to the host in between
        for it in range(self.niter):
            H.kmeans_prep(cent, image)
            H.kmeans_assign(x, xnorm, image, self.k, labels, dist, ws)
            H.kmeans_update(x, labels, cent, counts, slots[it], nsplit, ws)
            if self.iteration_hook is not None:
                self.iteration_hook(it, self, cent, counts)
        self.centroids_dev, self.counts = cent, counts
        self.obj = obj[:self.niter].cpu().numpy()                   # read back once
        self.n_split = int(nsplit.cpu().numpy()[0])
        return self.obj[-1] if self.niter else 0.0

    def assign_device(self, x):
        """(dist (N,) fp32, labels (N,) int32) device tensors against the trained centroids."""
        if self.centroids_dev is None:
            raise RuntimeError("Kmeans.assign before train")
        x = self._device_x(x)
        image = H.kmeans_prep(self.centroids_dev)
        labels, dist = H.kmeans_assign(x, H.kmeans_xnorm(x), image, self.k)
        return dist, labels

    def assign(self, x):
        """(D, I) numpy arrays of shape (N, 1), like `index.search(x, 1)`."""
        dist, labels = self.assign_device(x)
        return dist.cpu().numpy()[:, None], labels.cpu().numpy().astype(np.int64)[:, None]
