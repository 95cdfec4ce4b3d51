"""Float64 numpy restatement of csrc/scan_loss.hip and utils/scan.py: the SCAN loss of every head, its gradients, the class
assignment, the contract of draw_neighbours, and the training loop of ScanHeads.fit (same draws, same Adam) - the oracle of
tests/test_scan_cpu.py and tests/test_scan_gpu.py.  The inputs of the loss cases are made here from seeds, so the golden file
(tests/golden/scan/scan_small.npz, written by tests/golden/gen_golden_scan.py) holds results only."""
import numpy as np

CHUNK = 256                                # MI_SCAN_CHUNK: rows per partial sum of mi_scan_loss_fwd

# name -> B, C, H, kind, upstream gradient.  B crosses the chunk, C the half wave and the wave, H runs to its limit; the elements
# of all cases together keep the golden file under a megabyte.
CASES = {
    "b1": (1, 3, 1, "x1", 1.0),
    "b2_c64_h16": (2, 64, 16, "x1", 1.0),
    "chunk_less_c1": (CHUNK - 1, 1, 3, "x1", 1.0),
    "chunk_c2": (CHUNK, 2, 3, "x1", 1.0),
    "chunk_more_c33": (CHUNK + 1, 33, 1, "x1", 1.0),
    "chunks_c3": (2 * CHUNK + 3, 3, 3, "x1", 1.0),
    "b2_c32": (2, 32, 3, "x1", 1.0),
    "x30": (CHUNK + 1, 3, 1, "x30", 1.0),
    "extreme": (40, 5, 2, "extreme", 1.0),
    "dead_class": (300, 4, 1, "dead", 1.0),
    "upstream": (64, 10, 2, "x1", -2.5),
    "chunk_more_h16": (CHUNK + 1, 2, 16, "x1", 1.0),
}
ENTROPY_WEIGHT = 2.0
BCE_FLOOR = float(np.float32(1e-12))       # torch keeps the floor of BCELoss's backward as a float constant, in float64 too: 9.99999996e-13


def case_inputs(name):
    """(anchors, neighbours) fp32 (B, H C), H, upstream gradient, of a case.
    x1: standard normal logits, the neighbour's = the anchor's + noise.  x30: thirty times that, near one-hot.
    extreme: rows of +-200 (the hot classes equal: s is exactly 1; different: s underflows, the -100 clamp and the 1e-12 floor act),
    rows of +-15 (s about 1e-13: below the floor, above fp32's underflow) and ordinary rows.
    dead: class 0 at -40 in every anchor row: its mean probability is below 1e-8."""
    B, C, H, kind, up = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng([317, seed])
    a = rng.standard_normal((B, H, C))
    b = a + 0.5 * rng.standard_normal((B, H, C))
    if kind == "x30":
        a, b = 30 * a, 30 * b
    elif kind == "extreme":
        for i in range(B):
            for h in range(H):
                hot_a, hot_b = int(rng.integers(C)), int(rng.integers(C))
                if i % 4 == 0:
                    hot_b = hot_a
                if i % 4 == 2 and hot_b == hot_a:
                    # not at +-15: there s = 1 - 8e-13, and s - 1 keeps four digits in float64 - the float64 reference would differ
                    # from any other float64 evaluation by 1e-4 of that row's gradient
                    hot_b = (hot_a + 1) % C
                if i % 4 == 3:
                    continue                               # an ordinary row
                amp = 200.0 if i % 4 < 2 else 15.0
                a[i, h], b[i, h] = -amp, -amp
                a[i, h, hot_a], b[i, h, hot_b] = amp, amp
    elif kind == "dead":
        a[:, :, 0] = -40.0
    return (np.ascontiguousarray(a.reshape(B, H * C), np.float32), np.ascontiguousarray(b.reshape(B, H * C), np.float32), H, up)


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def norm_value(got, want):
    """the deviation of a figure v: |dv| / (1 + |v|), the largest over an array"""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / (1.0 + np.abs(want))).max())


def norm_grad(got, want):
    """the deviation of a gradient: max |dg| / max |g| over its case (several tensors of one case: stacked)"""
    want = np.asarray(want, np.float64)
    top = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / (top if top > 0 else 1.0)


def loss(anchors, neighbours, nheads, entropy_weight=ENTROPY_WEIGHT):
    """-> stats (H, 3) float64: total, consistency, entropy per head; and the sum of the totals."""
    B = anchors.shape[0]
    p = softmax(np.asarray(anchors, np.float64).reshape(B, nheads, -1))
    q = softmax(np.asarray(neighbours, np.float64).reshape(B, nheads, -1))
    s = (p * q).sum(-1)                                                    # (B, H)
    with np.errstate(divide="ignore"):
        consistency = -np.maximum(np.log(s), -100.0).sum(0) / B
    x = np.maximum(p.sum(0) / B, 1e-8)                                     # (H, C)
    entropy = -(x * np.log(x)).sum(-1)
    total = consistency - entropy_weight * entropy
    return np.stack([total, consistency, entropy], axis=1), float(total.sum())


def grads(anchors, neighbours, nheads, entropy_weight=ENTROPY_WEIGHT, upstream=1.0):
    """d (upstream x sum of totals) / d anchors, / d neighbours, float64, with torch's conventions: BCELoss's backward
    (s - 1) / max((1 - s) s, 1e-12) (the -100 clamp passes no test), clamp(min=1e-8) passes where m >= 1e-8."""
    B = anchors.shape[0]
    p = softmax(np.asarray(anchors, np.float64).reshape(B, nheads, -1))
    q = softmax(np.asarray(neighbours, np.float64).reshape(B, nheads, -1))
    s = (p * q).sum(-1, keepdims=True)
    ds = (s - 1.0) / np.maximum((1.0 - s) * s, BCE_FLOOR) / B
    m = p.sum(0) / B
    with np.errstate(divide="ignore"):
        gm = np.where(m >= 1e-8, entropy_weight * (np.log(m) + 1.0), 0.0) / B
    ga, gb = ds * q + gm[None], ds * p
    da = p * (ga - (p * ga).sum(-1, keepdims=True))
    db = q * (gb - (q * gb).sum(-1, keepdims=True))
    return upstream * da.reshape(anchors.shape), upstream * db.reshape(anchors.shape)


def assign(logits, nheads):
    """-> label (N, H) int32 (argmax, lowest index on a tie), conf (N, H) float64, counts (H, C) int64, prob (N, H C) float64"""
    N = logits.shape[0]
    z = np.asarray(logits, np.float64).reshape(N, nheads, -1)
    prob = softmax(z)
    label = z.argmax(-1).astype(np.int32)                                 # numpy's argmax returns the first maximum
    conf = np.take_along_axis(prob, label[..., None].astype(np.int64), -1)[..., 0]
    counts = np.stack([np.bincount(label[:, h], minlength=z.shape[-1]) for h in range(nheads)])
    return label, conf, counts, prob.reshape(N, -1)


def check_draw(index, anchor, neighbour, batch_size):
    """The contract of utils/scan.draw_neighbours for one epoch's table."""
    n = len(index)
    assert anchor.shape == neighbour.shape == ((n // batch_size) * batch_size,)
    assert len(np.unique(anchor)) == len(anchor) and anchor.min() >= 0 and anchor.max() < n      # every pick at most once
    table = np.concatenate([np.arange(n)[:, None], np.asarray(index, np.int64)], axis=1)
    assert (table[anchor] == neighbour[:, None]).any(axis=1).all()         # an entry of [i, index[i]]


def knn_l2(x, k):
    """index (N, k): the k nearest other rows by squared L2, ascending, lowest index on ties (what hipops.knn_search gives)"""
    x = np.asarray(x, np.float64)
    d = ((x[:, None] - x[None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


def blobs(seed=5, per=100, d=16, centres=3, spread=1.0, far=12.0):
    """`centres` Gaussian blobs of `per` picks in d dimensions, unit spread, centres `far` apart along different axes; shuffled."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.standard_normal((per, d)) * spread + far * np.eye(d)[c] for c in range(centres)])
    blob = np.repeat(np.arange(centres), per)
    order = rng.permutation(len(x))
    return np.ascontiguousarray(x[order], np.float32), blob[order]


def train(x, index, w0, b0, nheads, draw, seed, num_epochs, batch_size, lr, weight_decay, entropy_weight=ENTROPY_WEIGHT):
    """ScanHeads.fit in float64 on the host: the same draws (`draw` = utils/scan.draw_neighbours), torch.optim.Adam's update with
    its defaults (betas 0.9 / 0.999, eps 1e-8, L2 weight decay added to the gradient).  w0 (H C, d), b0 (H C,).
    -> w, b, history (num_epochs, H, 3)."""
    x = np.asarray(x, np.float64)
    w, b = np.asarray(w0, np.float64).copy(), np.asarray(b0, np.float64).copy()
    mom = [np.zeros_like(w), np.zeros_like(b)]
    var = [np.zeros_like(w), np.zeros_like(b)]
    step, history = 0, []
    for epoch in range(num_epochs):
        anchor, neighbour = draw(index, seed, epoch, batch_size)
        acc, nb = 0.0, 0
        for s in range(0, len(anchor), batch_size):
            xa, xn = x[anchor[s:s + batch_size]], x[neighbour[s:s + batch_size]]
            za, zn = xa @ w.T + b, xn @ w.T + b
            stats, _ = loss(za, zn, nheads, entropy_weight)
            da, dn = grads(za, zn, nheads, entropy_weight)
            g = [da.T @ xa + dn.T @ xn + weight_decay * w, da.sum(0) + dn.sum(0) + weight_decay * b]
            step += 1
            for i, prm in enumerate((w, b)):
                mom[i] = 0.9 * mom[i] + 0.1 * g[i]
                var[i] = 0.999 * var[i] + 0.001 * g[i] ** 2
                prm -= lr * (mom[i] / (1 - 0.9 ** step)) / (np.sqrt(var[i] / (1 - 0.999 ** step)) + 1e-8)
            acc, nb = acc + stats, nb + 1
        history.append(acc / nb)
    return w, b, np.stack(history)


def blobs_separated(label, blob):
    """True when every blob got one class and the blobs' classes differ"""
    classes = [np.unique(label[blob == c]) for c in np.unique(blob)]
    return all(len(c) == 1 for c in classes) and len({int(c[0]) for c in classes}) == len(classes)
