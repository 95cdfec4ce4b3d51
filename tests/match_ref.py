"""Host arbiter of the pick-to-target matching (csrc/match.hip): scipy on the dense float64 matrix, a float64 restatement
of the kernel's own algorithm, and generators of RIGID inputs - inputs whose optimal set of negative-cost pairs is unique,
proved by enumerating every connected component of the graph of negative pairs.

cost = min(d2 - radius ** 3, 0), the reference's cube (evaluation/algorithms.py:6-21)."""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment


def cost_matrix(preds, targets, radius):
    preds, targets = np.asarray(preds, np.float64).reshape(-1, 3), np.asarray(targets, np.float64).reshape(-1, 3)
    d2 = np.sum((preds[:, None] - targets[None]) ** 2, 2)
    return d2, np.minimum(d2 - float(radius) ** 3, 0.0)


def _result(d2, cost, rows, cols):
    p2t = np.full(d2.shape[0], -1, np.int32)
    dist = np.zeros(d2.shape[0])
    neg = cost[rows, cols] < 0
    p2t[rows[neg]] = cols[neg]
    dist[rows[neg]] = np.sqrt(d2[rows[neg], cols[neg]])
    return p2t, dist, float(cost[rows[neg], cols[neg]].sum())


def solve_scipy(preds, targets, radius):
    """(pred_to_target int32 (P,), dist (P,), total cost) of scipy's optimum, in the form the C entry returns."""
    d2, cost = cost_matrix(preds, targets, radius)
    rows, cols = linear_sum_assignment(cost)
    return _result(d2, cost, rows, cols)


def solve_f64(preds, targets, radius):
    """The kernel's algorithm restated in float64: shortest augmenting paths over the shorter side's rows, duals updated once
    per augmentation, arg-min ties to a free column first and then to the lower column."""
    d2, cost = cost_matrix(preds, targets, radius)
    P, T = cost.shape
    c = cost if P <= T else cost.T
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = np.full(nr, -1), np.full(nc, -1), np.full(nc, -1)
    for cur in range(nr):
        sp = np.full(nc, np.inf)
        scanned = np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            r = min_val + c[i] - u[i] - v
            upd = ~scanned & (r < sp)
            sp[upd], path[upd] = r[upd], i
            cand = np.flatnonzero(~scanned)
            key = np.lexsort((cand, row4col[cand] >= 0, sp[cand]))[0]
            j = cand[key]
            min_val = sp[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        d = min_val - sp[scanned]
        v[scanned] -= d
        owners = row4col[scanned]
        u[owners[owners >= 0]] += d[owners >= 0]
        u[cur] += min_val
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows, cols = (np.arange(nr), col4row) if P <= T else (col4row, np.arange(nr))
    return _result(d2, cost, rows, cols)


def check_valid(preds, targets, radius, p2t, dist):
    """Every target used at most once, every matched pair below the radius' cube, dist its distance; returns the pairs' cost."""
    d2, cost = cost_matrix(preds, targets, radius)
    p2t, dist = np.asarray(p2t), np.asarray(dist)
    assert p2t.shape == (d2.shape[0],) and dist.shape == p2t.shape
    m = np.flatnonzero(p2t >= 0)
    assert (p2t[m] < d2.shape[1]).all() and (p2t >= -1).all()
    assert len(np.unique(p2t[m])) == len(m), "a target is used twice"
    assert (d2[m, p2t[m]] < float(radius) ** 3).all(), "a matched pair is not below radius ** 3"
    assert np.array_equal(dist[m], np.sqrt(d2[m, p2t[m]])), "dist is not sqrt(d2) of the matched pair"
    assert (np.delete(dist, m) == 0).all(), "dist is not 0 where unmatched"
    return float(cost[m, p2t[m]].sum())


def is_rigid(preds, targets, radius, max_points=7):
    """True when the optimal set of negative-cost pairs is unique: every component of the graph of negative pairs (at most
    max_points points, asserted) has exactly one matching of minimum cost, found by enumerating all of its matchings."""
    _, cost = cost_matrix(preds, targets, radius)
    P, T = cost.shape
    ps, ts = np.nonzero(cost < 0)
    parent = list(range(P + T))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for p, t in zip(ps, ts):
        parent[find(p)] = find(P + t)
    comps = {}
    for p, t in zip(ps, ts):
        comps.setdefault(find(p), []).append((p, t))
    for edges in comps.values():
        assert len({p for p, _ in edges}) + len({t for _, t in edges}) <= max_points, "component too large to enumerate"
        sums = []
        for k in range(len(edges) + 1):
            for sub in itertools.combinations(edges, k):
                if len({p for p, _ in sub}) == k and len({t for _, t in sub}) == k:
                    sums.append(sum(cost[p, t] for p, t in sub))
        sums = np.sort(sums)
        if len(sums) > 1 and sums[0] == sums[1]:
            return False
    return True


RIGID_RADIUS = 3        # pairs closer than sqrt(27) may match
_CELL = 40              # components sit in cells this far apart: no pair across cells is negative

# components as (pick offsets along x, target offsets along x) from the cell's corner
_COMPONENTS = [
    ([0], [1]), ([0], [2]), ([0], [4]),       # isolated pairs
    ([0, 7], [4]),                            # two picks contest one target at distances 4 and 3: the nearer pick wins
    ([0], [3, 5]),                           # one pick, two targets at distances 3 and 5
    ([0, 5], [2, 9]),                         # chain pick-target-pick-target, lengths 2, 3, 4
    ([0, 3, 8], [1, 7]),                      # chain of five
    ([0], []), ([], [0]),                     # a far-away false positive, an unmatched target
]


def rigid_case(P, T, seed, shuffle=True):
    """(preds (P, 3), targets (T, 3)) integer-valued float64 built from the components above in far-apart cells, rows
    shuffled.  Rigid by construction; the tests assert it with is_rigid."""
    rng = np.random.default_rng(seed)
    comps, p, t = [], 0, 0
    while p < P or t < T:
        fits = [c for c in _COMPONENTS if p + len(c[0]) <= P and t + len(c[1]) <= T]
        c = fits[rng.integers(len(fits))]
        comps.append(c)
        p, t = p + len(c[0]), t + len(c[1])
    side = int(np.ceil(len(comps) ** (1 / 3))) if comps else 1
    cells = rng.permutation(side ** 3)[:len(comps)]
    preds, targets = [], []
    for cell, (po, to) in zip(cells, comps):
        corner = np.array([cell % side, cell // side % side, cell // side ** 2]) * _CELL
        axis = np.eye(3)[rng.integers(3)]
        preds += [corner + o * axis for o in po]
        targets += [corner + o * axis for o in to]
    preds = np.array(preds, np.float64).reshape(-1, 3)
    targets = np.array(targets, np.float64).reshape(-1, 3)
    if shuffle:
        preds, targets = preds[rng.permutation(P)], targets[rng.permutation(T)]
    return preds, targets


def crowded(P, T, box, seed):
    """Integer points in a small box: many negative pairs per point, an optimum that need not be unique."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, box, (P, 3)).astype(np.float64), rng.integers(0, box, (T, 3)).astype(np.float64)


def match_batch_scipy(targets, preds, radius):
    """The host arbiter in the form of evaluation.algorithms.match_coordinates_batch."""
    out, totals = [], []
    for t, p in zip(targets, preds):
        p2t, dist, total = solve_scipy(p, t, radius)
        out.append(((p2t >= 0).astype(np.float32), dist))
        totals.append(total)
    return out, np.array(totals)
