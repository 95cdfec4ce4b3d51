"""The SCAN step ("learning to classify by nearest neighbours") on stored embeddings: the reference's head-only mode
(`--cluster_head`: ClusteringModel's list of nn.Linear heads, simsiam_model_2d.py:885-921, trained by TomoSCANTrainer with SCANLoss
on (pick, random graph neighbour) pairs of its `scan` datasets), DESIGN.md 4.25.

All heads are ONE `hipops.HipLinear(d, nheads x nclusters)` - the product and the weight gradient are the MFMA path every other
Linear of the package takes - and the loss of all heads with its gradient is csrc/scan_loss.hip.  HipLinear takes widths that are
multiples of 16: the embeddings get zero columns and the stacked heads zero rows up to the next one, and the logits are cut back to
nheads x nclusters columns in front of the loss (no -inf ever enters a softmax).  torch.optim.Adam is the optimiser; the
pairs of an epoch are drawn on the host, copied once, and gathered on the device.  There is no CPU path.

After the clustering step (csrc/scan_selflabel.hip): ScanHeads.evaluate scores every head over the whole graph
as the reference's scan_evaluate does, ScanHeads.selflabel trains the best head on alone with the confidence-based cross-entropy.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import hipops as H


def draw_neighbours(index, seed, epoch, batch_size):
    """One epoch of (anchor, neighbour) picks: index (N, k) holds the k graph neighbours of every pick.  With a Generator seeded
    from (seed, epoch): a permutation of the N picks, cut to whole batches, and for every pick one of the k + 1 entries
    [the pick itself, neighbour 1 .. k], uniformly (the reference's neighbour table keeps the pick in column 0, so a pick can be its
    own neighbour).  -> anchor (m,), neighbour (m,) int64 with m = (N // batch_size) batch_size."""
    index = np.asarray(index)
    if index.ndim != 2 or index.shape[0] == 0:
        raise ValueError("index must be (N, k) with N >= 1, got %s" % (index.shape,))
    n, k = index.shape
    batch_size = int(batch_size)
    if not 1 <= batch_size <= n:
        raise ValueError("batch_size must be in 1..%d (the number of picks), got %d" % (n, batch_size))
    rng = np.random.default_rng([int(seed), int(epoch)])
    perm = rng.permutation(n)
    column = rng.integers(0, k + 1, size=n)
    table = np.concatenate([np.arange(n, dtype=np.int64)[:, None], index.astype(np.int64)], axis=1)
    anchor = perm[:(n // batch_size) * batch_size].astype(np.int64)
    return anchor, table[anchor, column[anchor]]


def selflabel_draws(index, seed, first_epoch, num_epochs, batch_size):
    """The draws of the self-labelling epochs: draw_neighbours with the epoch numbering continued after the `first_epoch`
    clustering epochs, so no self-label epoch repeats a clustering epoch's pairs.  Yields (epoch, anchor, strong row)."""
    for epoch in range(int(first_epoch), int(first_epoch) + int(num_epochs)):
        yield (epoch,) + draw_neighbours(index, seed, epoch, batch_size)


def check_sizes(nclusters, nheads):
    if not 1 <= int(nclusters) <= H.SCAN_MAX_CLASSES:
        raise ValueError("--nclusters must be in 1..%d, got %d" % (H.SCAN_MAX_CLASSES, nclusters))
    if not 1 <= int(nheads) <= H.SCAN_MAX_HEADS:
        raise ValueError("--nheads must be in 1..%d, got %d" % (H.SCAN_MAX_HEADS, nheads))


def initial_heads(d, nclusters, nheads, seed):
    """(weight (nheads nclusters, d), bias (nheads nclusters,)) fp32: nn.Linear's U(-1 / sqrt(d), 1 / sqrt(d)) from a host Generator."""
    g = torch.Generator().manual_seed(int(seed))
    bound = 1.0 / d ** 0.5
    w = (torch.rand(nheads * nclusters, d, generator=g) * 2 - 1) * bound
    b = (torch.rand(nheads * nclusters, generator=g) * 2 - 1) * bound
    return w, b


def state_keys(nheads):
    return [k for h in range(nheads) for k in ("cluster_head.%d.weight" % h, "cluster_head.%d.bias" % h)]


def checkpoint(state_dict, epoch, optimizer, best_loss, best_loss_head):
    """The reference's save_model_scan layout."""
    return {"epoch": int(epoch), "state_dict": state_dict, "optimizer": optimizer, "best_loss": float(best_loss),
            "best_loss_head": int(best_loss_head)}


def _pad16(v):
    return (v + 15) // 16 * 16


def _checked_graph(index, n, max_k=None):
    """index (n, k) as an array, checked once on the host: n rows, entries in 0..n-1, and 1 <= k <= max_k where one is given"""
    index = np.asarray(index)
    if index.ndim != 2 or index.shape[0] != n:
        raise ValueError("the graph has %s rows, the embeddings %d" % (index.shape[:1], n))
    if max_k is not None and not 1 <= index.shape[1] <= max_k:
        raise ValueError("the graph must have 1..%d neighbours per pick, got %d" % (max_k, index.shape[1]))
    if index.size and (index.min() < 0 or index.max() >= n):
        raise ValueError("the graph names a pick outside 0..%d" % (n - 1))
    return index


class ScanHeads:
    """nheads linear heads of nclusters classes on d-dimensional embeddings."""

    def __init__(self, d, nclusters, nheads=1, seed=317, device="cuda"):
        check_sizes(nclusters, nheads)
        if int(d) < 1:
            raise ValueError("embedding dimension must be >= 1, got %d" % d)
        self.d, self.nclusters, self.nheads, self.seed = int(d), int(nclusters), int(nheads), int(seed)
        self.width = self.nheads * self.nclusters
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HipExtensionError("ScanHeads live on the MI355X (cuda) device; there is no CPU path")
        self.lin = H.HipLinear(_pad16(self.d), _pad16(self.width)).to(self.device)
        w, b = initial_heads(self.d, self.nclusters, self.nheads, self.seed)
        with torch.no_grad():
            self.lin.weight.zero_()
            self.lin.bias.zero_()
            self.lin.weight[:self.width, :self.d].copy_(w)
            self.lin.bias[:self.width].copy_(b)
        self.epoch, self.best_loss, self.best_loss_head = 0, float("inf"), 0
        self.optimizer = None
        self.history = []                                  # per epoch: (nheads, 3) mean total, consistency, entropy

    # -- the reference's names ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """cluster_head.{h}.weight (nclusters, d) and .bias (nclusters,): slices of the stacked HipLinear, not copies."""
        c, out = self.nclusters, {}
        for h in range(self.nheads):
            out["cluster_head.%d.weight" % h] = self.lin.weight.detach()[h * c:(h + 1) * c, :self.d]
            out["cluster_head.%d.bias" % h] = self.lin.bias.detach()[h * c:(h + 1) * c]
        return out

    def load_state_dict(self, sd):
        mine = self.state_dict()
        if sorted(sd) != sorted(mine):
            raise ValueError("state dict holds %s, these heads %s" % (sorted(sd), sorted(mine)))
        with torch.no_grad():
            for k, v in mine.items():
                if tuple(sd[k].shape) != tuple(v.shape):
                    raise ValueError("%s is %s in the state dict, %s here" % (k, tuple(sd[k].shape), tuple(v.shape)))
                v.copy_(sd[k])

    def save(self, path):
        sd = {k: v.cpu().contiguous().clone() for k, v in self.state_dict().items()}
        torch.save(checkpoint(sd, self.epoch, self.optimizer.state_dict() if self.optimizer is not None else None,
                              self.best_loss, self.best_loss_head), path)

    @classmethod
    def load(cls, path, device="cuda"):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        sd = ck["state_dict"]
        nheads = len([k for k in sd if k.endswith(".weight")])
        if nheads == 0 or sorted(sd) != sorted(state_keys(nheads)):
            raise ValueError("%s holds no cluster_head.{h}.weight / .bias state" % path)
        nclusters, d = (int(s) for s in sd["cluster_head.0.weight"].shape)
        heads = cls(d, nclusters, nheads, device=device)
        heads.load_state_dict(sd)
        heads.epoch, heads.best_loss, heads.best_loss_head = int(ck["epoch"]), float(ck["best_loss"]), int(ck["best_loss_head"])
        return heads

    # -- the device work --------------------------------------------------------------------------------------------------------
    def _embeddings(self, x):
        """x (N, d) -> fp32 on the device with zero columns up to the HipLinear's width"""
        x = torch.as_tensor(x, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.d or x.shape[0] == 0:
            raise ValueError("embeddings must be (N, %d) with N >= 1, got %s" % (self.d, tuple(x.shape)))
        x = x.to(self.device)
        return torch.nn.functional.pad(x, (0, self.lin.in_f - self.d)).contiguous()

    def _logits(self, xp):
        z = self.lin(xp)
        return z if z.shape[1] == self.width else z[:, :self.width]

    def fit(self, x, index, num_epochs=100, batch_size=1024, lr=1e-3, weight_decay=1e-4, entropy_weight=2.0, log=None):
        """Train every head so that a pick and a random entry of [itself, its graph neighbours index (N, k)] get the same class while
        the classes stay balanced.  -> history (num_epochs, nheads, 3): per epoch and head the mean total, consistency, entropy over the
        epoch's batches.  best_loss_head is the head with the lowest mean total of the last epoch."""
        with torch.cuda.device(self.device):
            xp = self._embeddings(x)
            index = _checked_graph(index, xp.shape[0])

            def step(za, zn, acc):
                loss, stats = H.scan_loss(za.contiguous(), zn.contiguous(), self.nheads, entropy_weight)
                acc += stats
                return loss

            self._train(xp, index, num_epochs, batch_size, lr, weight_decay, step, (self.nheads, 3), self.history, log)
            last = self.history[-1][:, 0]
            self.best_loss_head = int(np.argmin(last))
            self.best_loss = float(last[self.best_loss_head])
            return np.stack(self.history)

    def _train(self, xp, index, num_epochs, batch_size, lr, weight_decay, step, shape, history, log, divide=None):
        """The epochs of fit and selflabel, Adam on these heads, the draws numbered on from self.epoch: per batch ONE index_select +
        HipLinear call on [anchors; partners], step(anchor logits, partner logits, acc) -> loss adds the batch's row to acc (`shape`,
        on the device); the mean over the epoch's batches (/ divide) - the epoch's one host read - goes to `history` and to
        log(epochs done, mean)."""
        bs = int(batch_size)
        if bs > H.SCAN_MAX_ROWS:
            raise ValueError("batch_size is at most %d, got %d" % (H.SCAN_MAX_ROWS, bs))
        self.optimizer = torch.optim.Adam(self.lin.parameters(), lr=lr, weight_decay=weight_decay)
        for epoch, anchor, partner in selflabel_draws(index, self.seed, self.epoch, num_epochs, bs):
            pairs = torch.from_numpy(np.stack([anchor.reshape(-1, bs), partner.reshape(-1, bs)], axis=1)).to(self.device)
            acc = torch.zeros(shape, dtype=torch.float32, device=self.device)
            for rows in pairs:                             # (2, bs): the anchors, then their partners
                z = self._logits(xp.index_select(0, rows.reshape(-1)))
                loss = step(z[:bs], z[bs:], acc)
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self.optimizer.step()
            mean = (acc / len(pairs)).cpu().numpy()        # the epoch's one host read
            if divide is not None:
                mean /= divide
            history.append(mean)
            self.epoch = epoch + 1
            if log is not None:
                log(self.epoch, mean)

    def _graph(self, index, n):
        """index (N, k) checked once on the host -> int32 on the device"""
        index = _checked_graph(index, n, H.SCAN_MAX_NEIGHBOURS)
        return torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(self.device)

    def evaluate(self, x, index):
        """The reference's scan_evaluate: every head scored on every pick against all entries of [itself, its graph neighbours
        index (N, k)] under the weights as they stand.  -> stats (nheads, 3): total = consistency - entropy, consistency, entropy;
        sets best_loss_head (lowest total, lowest index on a tie) and best_loss.  One host read."""
        with torch.cuda.device(self.device), torch.no_grad():
            xp = self._embeddings(x)
            table = self._graph(index, xp.shape[0])
            stats, best = H.scan_graph_eval(self._logits(xp).contiguous(), table, self.nheads, with_self=True, validate=False)
            both = torch.cat([stats.reshape(-1), best.float()]).cpu().numpy()
            stats = both[:-1].reshape(self.nheads, 3)
            self.best_loss_head = int(both[-1])
            self.best_loss = float(stats[self.best_loss_head, 0])
            return stats

    def selflabel(self, x, index, head, num_epochs=10, batch_size=1024, lr=1e-4, threshold=0.99, balance=True, log=None,
                  weight_decay=1e-4):
        """SCAN's third step on head `head` alone (the reference's load_model_selflabel keeps the best head only): a one-head
        ScanHeads is rebuilt from that slice and trained with the confidence-based cross-entropy.  Per step ONE HipLinear call on
        [anchors; strong rows]: the weak logits are the anchors' own, detached; the strong rows are an entry of [the pick, its
        graph neighbours], the draw of fit() with the epoch numbering continued - stored embeddings have no image augmentation, so
        the graph neighbour stands in for the reference's strong view.  Adam.
        -> (the one-head ScanHeads, stats (num_epochs, 3): per epoch the mean loss, the share of confident picks and the mean number
        of classes present over the epoch's batches - one host read per epoch)."""
        if not 0 <= int(head) < self.nheads:
            raise ValueError("head must be in 0..%d, got %d" % (self.nheads - 1, head))
        if not 0.0 <= float(threshold) < 1.0:
            raise ValueError("the confidence threshold must be in [0, 1), got %g" % threshold)
        with torch.cuda.device(self.device):
            one = ScanHeads(self.d, self.nclusters, 1, seed=self.seed, device=self.device)
            sd = self.state_dict()
            one.load_state_dict({"cluster_head.0.weight": sd["cluster_head.%d.weight" % head],
                                 "cluster_head.0.bias": sd["cluster_head.%d.bias" % head]})
            one.epoch = self.epoch
            xp = one._embeddings(x)
            index = _checked_graph(index, xp.shape[0], H.SCAN_MAX_NEIGHBOURS)

            def step(weak, strong, acc):                   # acc: loss, confident rows, classes present
                loss, info, _ = H.scan_selflabel_loss(weak.detach().contiguous(), strong.contiguous(), threshold, balance)
                acc[0] += loss.detach()
                acc[1:] += info[:2]
                return loss

            history = []
            one._train(xp, index, num_epochs, batch_size, lr, weight_decay, step, (3,), history, log,
                       divide=np.array([1, int(batch_size), 1], np.float32))
            if history:
                one.best_loss = float(history[-1][0])
            return one, np.stack(history) if history else np.zeros((0, 3), np.float32)

    def predict(self, x, with_prob=False):
        """-> label (N, nheads) int32, conf (N, nheads) fp32, counts (nheads, nclusters) int32 [, prob (N, nheads nclusters) fp32]
        as numpy arrays: every pick classified by every head."""
        with torch.cuda.device(self.device), torch.no_grad():
            z = self._logits(self._embeddings(x)).contiguous()
            label, conf, counts, prob = H.scan_assign(z, self.nheads, with_prob=with_prob)
            out = (label.cpu().numpy(), conf.cpu().numpy(), counts.cpu().numpy())
            return out + (prob.cpu().numpy(),) if with_prob else out
