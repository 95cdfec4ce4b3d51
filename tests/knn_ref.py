"""The arbiter of the k-nearest-neighbour tests: a blocked float64 q @ x.T with a stable sort (ties go to the lowest index), an
optional self exclusion, the parity statement `check_knn` and the makers of the test inputs.  Nothing here
calls the code under test."""
import numpy as np

from kmeans_ref import band, make  # noqa: F401  (make: the inputs of the k-means tests; band(d) = (d + 8) 2^-24)

CASES = {            # name: (N, d, k, spread) - N not a multiple of 32, d not a multiple of 16, k not a power of two
    "A": (4099, 32, 10, 0.15),
    "B": (4099, 128, 16, 0.15),
    "C": (3000, 100, 10, 0.15),
}
NONEXACT_CAP = 0.003   # at most 0.3 % of a case's (row, rank) pairs may be near-ties with the next rank (see nonexact)
TIE_ROWS = (5, 37, 2051, 4090)


def values64(q, x, metric, rows=None):
    """float64 values of the query rows `rows` (all) against every database row: q.x, or max(0, |q|^2 + (|x|^2 - 2 q.x))."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    if rows is not None:
        q = q[rows]
    v = q @ x.T
    if metric == "l2":
        v = np.maximum((q * q).sum(1)[:, None] + ((x * x).sum(1)[None, :] - 2.0 * v), 0.0)
    return v


def scales64(q, x, metric, index):
    """scale of the pairs (row i, index[i, r]): |q||x| for ip, |q|^2 + |x|^2 for l2."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    qn, xn = (q * q).sum(1), (x * x).sum(1)
    if metric == "ip":
        return np.sqrt(qn)[:, None] * np.sqrt(xn)[index]
    return qn[:, None] + xn[index]


def topk64(q, x, k, metric, exclude_self=False, block=512):
    """-> index (M, k) int64, value (M, k) float64: the k best columns of every row, best first, lowest index on ties."""
    M, N = len(q), len(x)
    k = min(k, N - (1 if exclude_self else 0))
    index, value = np.empty((M, k), np.int64), np.empty((M, k))
    for s in range(0, M, block):
        rows = np.arange(s, min(s + block, M))
        v = values64(q, x, metric, rows)
        key = -v if metric == "ip" else v.copy()               # ascending key = best first
        if exclude_self:
            key[np.arange(len(rows)), rows] = np.inf
        order = np.argsort(key, axis=1, kind="stable")[:, :k]
        index[rows] = order
        value[rows] = np.take_along_axis(v, order, axis=1)
    return index, value


def nonexact(q, x, k, metric, exclude_self=False):
    """The arbiter alone: (index, value, scale, exact, share) for ranks 0 .. k - 1, from a search for k + 1.  exact[i, r]: both
    neighbouring gaps of rank r (for the last rank the lower gap is the one to rank k + 1) are >= 2 band scale: there the
    device must return the arbiter's index.  share: the part of the (row, rank) pairs whose gap to the next rank is inside the
    band (< band scale): a rank that fp32 cannot be asked to tell from its successor.  This is the measure behind the cap of
    0.3 % and the figures it was set by (0.03 % .. 0.17 % for CASES; 0.23 % for k = 100 on 1500 x 64); counting every pair
    with a neighbouring gap below 2 band scale instead gives 0.06 % .. 0.64 % on the same inputs."""
    d = q.shape[1]
    idx, val = topk64(q, x, k + 1, metric, exclude_self)
    scale = scales64(q, x, metric, idx[:, :k])
    gap = np.abs(np.diff(val, axis=1))                          # gap[:, r] between ranks r and r + 1
    lower = np.full((len(q), k), np.inf)
    lower[:, :gap.shape[1]] = gap[:, :k]
    upper = np.full((len(q), k), np.inf)
    upper[:, 1:] = gap[:, :k - 1]
    exact = (lower >= 2 * band(d) * scale) & (upper >= 2 * band(d) * scale)
    return idx[:, :k], val[:, :k], scale, exact, float((lower < band(d) * scale).mean())


def check_knn(q, x, k, metric, got_index, got_value, exclude_self=False, what="", cap=NONEXACT_CAP, arbiter=None):
    """The parity statement.  q (M, d), x (N, d) fp32 are what the device was given.  Prints the figures, then asserts, with
    scale = |q||x| (ip) or |q|^2 + |x|^2 (l2) and s_r the float64 r-th best value of the row:
      0. (before the device's output is looked at) <= cap of the (row, rank) pairs are near-ties with the next rank;
      1. every returned row has k distinct indices in range, none the row itself when self is excluded; values sorted;
      2. the float64 value of the returned index is within band scale of s_r;
      3. the returned value is within 2 band scale of the float64 value of the returned index;
      4. where rank r is exact the index is the arbiter's.
    The cap of 0. is on the near-ties, not on the complement of 4.'s "exact" (up to 0.64 % of the pairs on CASES, see nonexact);
    both shares are printed.  arbiter: a cached nonexact(q, x, k, metric, exclude_self).  Returns the share of near-ties."""
    M, N, d = len(q), len(x), q.shape[1]
    idx, val, scale, exact, share = arbiter if arbiter is not None else nonexact(q, x, k, metric, exclude_self)
    assert share <= cap, "%s: %.4f %% of the (row, rank) pairs are near-ties (cap %.2f %%)" % (what, 100 * share, 100 * cap)
    gi = np.asarray(got_index).astype(np.int64)
    gv = np.asarray(got_value, np.float64)
    assert gi.shape == (M, k) and gv.shape == (M, k), (gi.shape, gv.shape)
    assert gi.min() >= 0 and gi.max() < N, "%s: index out of range [%d, %d]" % (what, gi.min(), gi.max())
    srt = np.sort(gi, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "%s: a row returns an index twice" % what
    if exclude_self:
        assert (gi != np.arange(M)[:, None]).all(), "%s: a row returns itself" % what
    dv = np.diff(gv, axis=1)
    assert (dv <= 0).all() if metric == "ip" else (dv >= 0).all(), "%s: returned values are not sorted" % what
    true = np.empty((M, k))
    for s in range(0, M, 512):
        rows = np.arange(s, min(s + 512, M))
        true[rows] = np.take_along_axis(values64(q, x, metric, rows), gi[rows], axis=1)
    tol = band(d) * scale
    e_rank = np.abs(true - val) / tol
    e_val = np.abs(gv - true) / (band(d) * scales64(q, x, metric, gi))
    differ = gi != idx
    print("%s: M=%d N=%d d=%d k=%d %s: near-ties %.4f %% of pairs (capped), pairs not exact %.4f %% (exempt from index equality, "
          "not capped), index differs on %d pairs (%d of them exact), rank error max %.3f band (bound 1), value error max %.3f "
          "band (bound 2)"
          % (what, M, N, d, k, metric, 100 * share, 100 * float((~exact).mean()), int(differ.sum()), int((differ & exact).sum()),
             float(e_rank.max()), float(e_val.max())))
    assert float(e_rank.max()) <= 1.0, "%s: a returned index is %.3f band scale from the rank's float64 value" % (what, e_rank.max())
    assert float(e_val.max()) <= 2.0, "%s: a returned value is %.3f band scale from float64" % (what, e_val.max())
    assert not (differ & exact).any(), "%s: %d exact (row, rank) pairs differ from the arbiter" % (what, int((differ & exact).sum()))
    return share


def tie_case(N=4099, d=16, seed=3):
    """Small integers (exact in bf16x3, fp32 and float64 alike: |value| <= 9 d): many equal values in every row, and row
    TIE_ROWS[0] copied to the other TIE_ROWS - different column tiles of 32, different splits for n_split 3 and 7."""
    x = np.random.RandomState(seed).randint(-3, 4, size=(N, d)).astype(np.float32)
    for r in TIE_ROWS[1:]:
        x[r] = x[TIE_ROWS[0]]
    return x


def split_of(col, N, n_split):
    """The part of the database that holds column `col`: parts of ceil(ceil(N / 32) / n_split) column tiles of 32."""
    tiles = (N + 31) // 32
    return (col // 32) // ((tiles + n_split - 1) // n_split)
