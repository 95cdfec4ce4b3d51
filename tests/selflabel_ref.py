"""Float64 numpy restatement of csrc/scan_selflabel.hip and of ScanHeads.selflabel: the heads scored over the whole graph (the
reference's scan_evaluate), the self-labelling loss with its gradient (ConfidenceBasedCE), and the self-label training loop (same
draws, same Adam) - the oracle of tests/test_scan_selflabel_cpu.py and tests/test_scan_selflabel_gpu.py.  The inputs of every case
are made here from seeds, so the golden file (tests/golden/scan/selflabel_small.npz, written by
tests/golden/gen_golden_scan_selflabel.py) holds results only."""
import numpy as np

from scan_ref import CHUNK, norm_grad, norm_value, softmax  # noqa: F401  (the tests reach the norms through this module too)

MARGIN = 1e-4                              # no row's largest probability lies this close to its case's threshold

# name -> B, C, kind, threshold rule, balance, upstream gradient.  B crosses the chunk, C the half wave and the wave.
#   threshold rule: a number, "half" (about half the rows confident), "one" (exactly one row confident)
#   kind: x1      weak = 2 x standard normal, strong = weak + noise
#         absent  x1 with class 0 at -40 in every weak row: no row targets it
#         wrong   x1 with the strong logits thirty times one-hot on ANOTHER class than the target: a large, finite loss
#         pm200   rows of +-200, the strong row's hot class the target's in every other row (loss 0 there, 400 in the others)
#         flat    weak = 0.1 x standard normal: no row is confident at 0.9
SELFLABEL_CASES = {
    "b1_c3": (1, 3, "x1", 0.0, True, 1.0),
    "b2_c64": (2, 64, "x1", 0.0, True, 1.0),
    "b2_c64_unbalanced": (2, 64, "x1", 0.0, False, 1.0),
    "b255_c1": (CHUNK - 1, 1, "x1", 0.5, True, 1.0),
    "b256_c2": (CHUNK, 2, "x1", "half", True, 1.0),
    "b257_c33": (CHUNK + 1, 33, "x1", "half", True, 1.0),
    "b515_c3": (2 * CHUNK + 3, 3, "x1", "half", True, 1.0),
    "b515_c3_unbalanced": (2 * CHUNK + 3, 3, "x1", "half", False, 1.0),
    "every_row": (CHUNK + 1, 3, "x1", 0.0, True, 1.0),
    "one_row": (CHUNK + 1, 3, "x1", "one", True, 1.0),
    "absent_class": (300, 4, "absent", "half", True, 1.0),
    "x30_wrong": (CHUNK + 1, 3, "wrong", "half", True, 1.0),
    "pm200": (40, 5, "pm200", 0.5, True, 1.0),
    "upstream": (64, 10, "x1", "half", True, -2.5),
    "zz_none": (CHUNK + 1, 3, "flat", 0.9, True, 1.0),           # the last: n = 0, the reference raises
}
NONE_CASE = "zz_none"

# name -> N, k, H, C, kind, with_self.  kind: x1 standard normal logits; x30 thirty times that; dead: class 0 of head 0 at -40;
# close: head 1 = head 0 + a little noise, the two totals differ in the third digit
GRAPH_CASES = {
    "n2_k1": (2, 1, 1, 2, "x1", True),
    "n255_k5_c1": (CHUNK - 1, 5, 1, 1, "x1", True),
    "n257_k20_h16_c2": (CHUNK + 1, 20, 16, 2, "x1", True),
    "n515_k5_h3_c33": (2 * CHUNK + 3, 5, 3, 33, "x1", True),
    "n515_k5_h3_c33_noself": (2 * CHUNK + 3, 5, 3, 33, "x1", False),
    "n257_k1_c64_noself": (CHUNK + 1, 1, 1, 64, "x1", False),
    "dead_class": (300, 5, 2, 4, "dead", True),
    "x30": (CHUNK + 1, 5, 3, 3, "x30", True),
    "x30_noself": (CHUNK + 1, 5, 3, 3, "x30", False),
    "close_heads": (CHUNK + 1, 5, 2, 3, "close", True),
}


def _threshold(pmax, rule):
    """A threshold with at least MARGIN to every row's largest probability, by the case's rule."""
    if not isinstance(rule, str):
        return float(rule)
    s = np.sort(pmax)[::-1]                                # descending
    want = 1 if rule == "one" else max(1, len(s) // 2)     # rows to leave above the threshold
    for r in ([want] if rule == "one" else list(range(want, len(s))) + list(range(want - 1, 0, -1))):
        if r < len(s) and s[r - 1] - s[r] > 4 * MARGIN:
            return float(min(0.5 * (s[r - 1] + s[r]), 1.0 - 2 * MARGIN))
    raise AssertionError("no gap of %g among the rows' largest probabilities" % (4 * MARGIN))


def selflabel_inputs(name):
    """-> weak, strong (B, C) fp32, threshold (float), balance, upstream gradient of a case"""
    B, C, kind, rule, balance, up = SELFLABEL_CASES[name]
    rng = np.random.default_rng([318, sorted(SELFLABEL_CASES).index(name)])
    weak = (0.1 if kind == "flat" else 2.0) * rng.standard_normal((B, C))
    strong = weak + 0.5 * rng.standard_normal((B, C))
    if kind == "absent":
        weak[:, 0] = -40.0
    elif kind == "wrong":
        t = weak.astype(np.float32).argmax(1)
        strong = np.full((B, C), -1.0)
        strong[np.arange(B), (t + 1) % C] = 1.0
        strong = 30.0 * (strong + 0.01 * rng.standard_normal((B, C)))
    elif kind == "pm200":
        hot = rng.integers(C, size=B)
        other = np.where(np.arange(B) % 2 == 0, hot, (hot + 1 + rng.integers(C - 1, size=B)) % C)
        weak, strong = np.full((B, C), -200.0), np.full((B, C), -200.0)
        weak[np.arange(B), hot], strong[np.arange(B), other] = 200.0, 200.0
    if rule == "one":
        weak[B // 3, 1] += 12.0                            # one row far above the rest
    weak, strong = np.ascontiguousarray(weak, np.float32), np.ascontiguousarray(strong, np.float32)
    return weak, strong, _threshold(softmax(weak.astype(np.float64)).max(1), rule), balance, up


def class_weights(count, n, balance):
    """(C,) float64: 1 / (count / n) formed in float32, as the reference forms it from counts.float() / n, where balance and the
    class is present; else 1"""
    w = np.ones(len(count), np.float64)
    if balance and n > 0:
        present = count > 0
        w[present] = (np.float32(1.0) / (count[present].astype(np.float32) / np.float32(n))).astype(np.float64)
    return w


def selflabel(weak, strong, threshold, balance, upstream=1.0):
    """-> dict: loss (float), grad (B, C) = upstream x d loss / d strong, target (B,) int32 (argmax, lowest index on a tie),
    mask (B,) uint8, count (C,) int64, info (3,) = n, classes present, B, pmax (B,), weight (C,), denom.  n = 0: loss 0, gradient 0."""
    B, C = weak.shape
    p = softmax(np.asarray(weak, np.float64))
    target = np.asarray(weak).argmax(1).astype(np.int32)   # on the logits; numpy's argmax returns the first maximum
    pmax = p[np.arange(B), target]
    mask = pmax > threshold
    n = int(mask.sum())
    count = np.bincount(target[mask], minlength=C)
    w = class_weights(count, n, balance)
    q = softmax(np.asarray(strong, np.float64))            # (no entry underflows in float64: the cases' logits span 400 at most)
    wt = w[target] * mask
    denom = float(wt.sum())
    onehot = np.zeros((B, C))
    onehot[np.arange(B), target] = 1.0
    if n == 0:
        loss, grad = 0.0, np.zeros((B, C))
    else:
        loss = float((wt * -np.log(q[np.arange(B), target])).sum() / denom)
        grad = upstream * (wt / denom)[:, None] * (q - onehot)
    return dict(loss=loss, grad=grad, target=target, mask=mask.astype(np.uint8), count=count,
                info=np.array([n, int((count > 0).sum()), B]), pmax=pmax, weight=w, denom=denom)


def graph_inputs(name):
    """-> logits (N, H C) fp32, index (N, k) int32 (k other picks per pick, no repeats), H, with_self"""
    N, k, H, C, kind, with_self = GRAPH_CASES[name]
    rng = np.random.default_rng([319, sorted(GRAPH_CASES).index(name)])
    z = rng.standard_normal((N, H, C)) * (1.0 + 0.15 * np.arange(H))[None, :, None]       # sharper from head to head: totals apart
    if kind == "x30":
        z *= 30.0
    elif kind == "dead":
        z[:, 0, 0] = -40.0
    elif kind == "close":
        z[:, 1] = z[:, 0] + 0.2 * rng.standard_normal((N, C))
    index = np.stack([rng.choice(np.delete(np.arange(N), i), size=k, replace=False) for i in range(N)]).astype(np.int32)
    return np.ascontiguousarray(z.reshape(N, H * C), np.float32), index, H, with_self


def table(index, with_self):
    """[self, neighbour 1..k] (the table draw_neighbours draws from) or the neighbours alone"""
    index = np.asarray(index, np.int64)
    return np.concatenate([np.arange(len(index))[:, None], index], axis=1) if with_self else index


def graph_eval(logits, index, nheads, with_self=True):
    """-> stats (H, 3) float64: total = consistency - entropy, consistency, entropy per head; best: the head with the lowest total,
    the lowest index on a tie"""
    N = logits.shape[0]
    p = softmax(np.asarray(logits, np.float64).reshape(N, nheads, -1))        # (N, H, C)
    t = table(index, with_self)
    s = np.einsum("nhc,nkhc->nkh", p, p[t])                                   # (N, K, H)
    with np.errstate(divide="ignore"):
        consistency = -np.maximum(np.log(s), -100.0).sum((0, 1)) / (N * t.shape[1])
    x = np.maximum(p.sum(0) / N, 1e-8)
    entropy = -(x * np.log(x)).sum(-1)
    total = consistency - entropy
    return np.stack([total, consistency, entropy], axis=1), int(np.argmin(total))


def best_gap(stats):
    """the distance of the two lowest totals (inf for one head)"""
    t = np.sort(stats[:, 0])
    return float(t[1] - t[0]) if len(t) > 1 else float("inf")


def selflabel_train(x, index, w0, b0, draws, seed, first_epoch, num_epochs, batch_size, lr, threshold, balance, weight_decay=1e-4):
    """ScanHeads.selflabel in float64 on the host for ONE head w0 (C, d), b0 (C,): `draws` = utils/scan.selflabel_draws, per step
    the weak logits are the anchors', the strong rows the drawn entries of [self, neighbours]; torch.optim.Adam's update with its
    defaults.  -> w, b, stats (num_epochs, 3): mean loss, share of confident picks, mean number of classes present."""
    x = np.asarray(x, np.float64)
    w, b = np.asarray(w0, np.float64).copy(), np.asarray(b0, np.float64).copy()
    mom, var = [np.zeros_like(w), np.zeros_like(b)], [np.zeros_like(w), np.zeros_like(b)]
    step, history = 0, []
    for _, anchor, strong in draws(index, seed, first_epoch, num_epochs, batch_size):
        acc, nb = np.zeros(3), 0
        for s in range(0, len(anchor), batch_size):
            xa, xs = x[anchor[s:s + batch_size]], x[strong[s:s + batch_size]]
            r = selflabel(xa @ w.T + b, xs @ w.T + b, threshold, balance)
            g = [r["grad"].T @ xs + weight_decay * w, r["grad"].sum(0) + weight_decay * b]
            step += 1
            for i, prm in enumerate((w, b)):
                mom[i] = 0.9 * mom[i] + 0.1 * g[i]
                var[i] = 0.999 * var[i] + 0.001 * g[i] ** 2
                prm -= lr * (mom[i] / (1 - 0.9 ** step)) / (np.sqrt(var[i] / (1 - 0.999 ** step)) + 1e-8)
            acc, nb = acc + [r["loss"], r["info"][0] / batch_size, r["info"][1]], nb + 1
        history.append(acc / nb)
    return w, b, np.stack(history)
