"""k-nearest-neighbour search on the MI355X (csrc/knn.hip, hipops.knn_search, utils/memory_bank.py, plot_2d --num_neighbor)
against the float64 arbiter of tests/knn_ref.py.  Parity statement: the index is the arbiter's wherever both
neighbouring gaps of a rank are >= 2 (d + 8) 2^-24 scale; elsewhere a swap between near-ties only."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_ref as R
from conftest import REPO

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _search(q, x, k, metric, exclude_self=False, n_split=0):
    from cet_pick_amd import hipops as H
    index, value = H.knn_search(_dev(q), _dev(x), k, metric=metric, exclude_self=exclude_self, n_split=n_split)
    return index.cpu().numpy(), value.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _data(N, d, spread=0.15, seed=7):
    return R.make(N, d, seed=seed, spread=spread)


@functools.lru_cache(maxsize=None)
def _arbiter(N, d, k, spread, metric, exclude_self):
    x = _data(N, d, spread)
    return R.nonexact(x, x, k, metric, exclude_self)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_self_search_matches_float64(name, metric, exclude_self):
    N, d, k, spread = R.CASES[name]
    x = _data(N, d, spread)
    arb = _arbiter(N, d, k, spread, metric, exclude_self)
    assert arb[4] <= R.NONEXACT_CAP
    index, value = _search(x, x, k, metric, exclude_self)
    R.check_knn(x, x, k, metric, index, value, exclude_self, what="case %s" % name, arbiter=arb)


# 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_k_100_spans_several_column_tiles(metric):
    """k = 100 > the 32 columns of a tile and > the 64 lanes of a wave.  Near-tie share at spread 0.15, the arbiter alone:
    0.23 % (ip), 0.21 % (l2)."""
    N, d, k, spread = 1500, 64, 100, 0.15
    x = _data(N, d, spread)
    arb = _arbiter(N, d, k, spread, metric, True)
    assert arb[4] <= R.NONEXACT_CAP
    index, value = _search(x, x, k, metric, True)
    R.check_knn(x, x, k, metric, index, value, True, what="k = 100", arbiter=arb)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [257, 1])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_queries_are_not_the_database(M, metric):
    N, d, k, spread = R.CASES["A"]                 # near-tie share of these queries, the arbiter alone: 0.04 % (case B: 0.34 %)
    x = _data(N, d, spread)
    q = R.make(M, d, seed=11, spread=spread)
    index, value = _search(q, x, k, metric)
    R.check_knn(q, x, k, metric, index, value, what="M = %d" % M)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_database_of_exactly_k_rows(metric):
    d, k = 100, 10
    x = _data(3000, d)
    q = R.make(70, d, seed=11)
    index, value = _search(q, x[:k], k, metric)                        # N = k: every row, sorted
    R.check_knn(q, x[:k], k, metric, index, value, what="N = k")
    index, value = _search(x[:k + 1], x[:k + 1], k, metric, True)      # N = k + 1, self excluded: every other row
    R.check_knn(x[:k + 1], x[:k + 1], k, metric, index, value, True, what="N = k + 1")


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_result_does_not_depend_on_the_split_count(metric):
    N, d, k, spread = R.CASES["B"]
    x = _data(N, d, spread)
    runs = [_search(x, x, k, metric, True, n_split) for n_split in (1, 3, 7, 1, 3, 7, 0)]
    for index, value in runs[1:]:
        assert index.tobytes() == runs[0][0].tobytes() and value.tobytes() == runs[0][1].tobytes()


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("k", [16, 100])
def test_ties_go_to_the_lowest_index(metric, k):
    x = R.tie_case()
    want_i, want_v = R.topk64(x, x, k, metric, True)
    for n_split in (1, 3, 7):
        index, value = _search(x, x, k, metric, True, n_split)
        assert np.array_equal(index, want_i), "n_split %d: %d rows differ" % (n_split, int((index != want_i).any(1).sum()))
        assert np.array_equal(value.astype(np.float64), want_v)


@pytest.mark.parametrize("n_split", [1, 2])
@pytest.mark.parametrize("d", [17, 100, 300])
def test_l2_nearest_neighbour_is_the_kmeans_assignment_bit_for_bit(d, n_split):
    """The contract of csrc/rowdot.h: the squared L2 distance of knn_search and the dist of kmeans_assign are
    one product chain, one column-norm sum and one row-norm sum, and both orders take the lowest index on ties - so the
    nearest of k centroids is the k-means label and its value the same bytes.  M = 257: four 64-row workgroups and one row;
    48 centroids: a full column tile and half of one (the padding columns carry +inf in one image and 0 in the other);
    duplicates inside a tile and across the tile boundary; d = 17 scalar loads and a ragged k-step, 100 vector loads with a
    scalar last group, 300 32-row workgroups in k-means against 64-row ones here."""
    import torch
    from cet_pick_amd import hipops as H
    M, k = 257, 48
    x = _dev(R.make(M, d, seed=7, spread=0.15))
    c = R.make(k, d, seed=11, spread=0.15)
    c[40], c[33] = c[5], c[2]
    c = _dev(c)
    labels, dist = H.kmeans_assign(x, H.kmeans_xnorm(x), H.kmeans_prep(c), k)
    index, value = H.knn_search(x, c, 1, metric="l2", n_split=n_split)
    differ = index[:, 0] != labels
    print("d=%d n_split=%d: %d of %d indices differ, %d values differ" % (
        d, n_split, int(differ.sum()), M, int((value[:, 0].view(torch.int32) != dist.view(torch.int32)).sum())))
    assert not bool(((labels == 40) | (labels == 33)).any())          # a duplicate never wins over its lower-index twin
    assert torch.equal(index[:, 0], labels)
    assert torch.equal(value[:, 0].contiguous().view(torch.int32), dist.view(torch.int32))


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_unsupported_arguments_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    x = torch.zeros(600, 16, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.knn_search(x, x, 129)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.knn_search(x, x[:15].contiguous(), 16)                     # N < k
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.knn_search(x[:16].contiguous(), x[:16].contiguous(), 16, exclude_self=True)
    wide = torch.zeros(64, 513, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.knn_search(wide, wide, 4)
    with pytest.raises(L.HipExtensionError):
        H.knn_search(x, x, 4, metric="cosine")
    with pytest.raises(L.HipExtensionError):
        H.knn_search(x, torch.zeros(600, 8, device="cuda"), 4)
    lib = L.lib()
    out_i, out_v = torch.empty(600, 4, dtype=torch.int32, device="cuda"), torch.empty(600, 4, device="cuda")
    ws = torch.empty(lib.mi_knn_workspace_bytes(600, 600, 16, 4, 0, 0), dtype=torch.uint8, device="cuda")
    args = [600, 600, 16, 4, 0, 0, 0, L.ptr(out_i), L.ptr(out_v), L.ptr(ws), ws.numel(), L.stream()]
    assert lib.mi_knn_search(None, L.ptr(x), *args) == -1            # a null pointer
    assert lib.mi_knn_search(L.ptr(x), L.ptr(x), *(args[:9] + [None] + args[10:])) == -1
    assert lib.mi_knn_search(L.ptr(x), L.ptr(x), *(args[:10] + [16] + args[11:])) == -2       # workspace too small
    # a valid call still works
    y = _data(3000, 100)
    index, value = _search(y[:300], y, 10, "l2")
    R.check_knn(y[:300], y, 10, "l2", index, value, what="after the refusals")


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_database_past_2_gib():
    """N x d x 4 bytes > 2 GiB: queries copied from rows behind the 2 GiB offset find themselves at rank 0, and the float64
    distances of every returned pair are the returned ones.  The rank-0 index is asserted exactly.  The rank-0 value is not
    asserted to be the bits of 0: |q|^2 and |x|^2 are fp32 fmaf sums and q.x is a bf16x3 product, which need not cancel
    exactly; it is held to the parity bound of a pair at true distance 0, 0 <= value <= 2 band (|q|^2 + |x|^2) = 4 band |x|^2
    (about 4e-3 here against neighbours at distance > 1), asserted on its own."""
    import torch
    from cet_pick_amd import hipops as H
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip("%.2f GiB of device memory are free, the test needs 8" % (free / 2.0 ** 30))
    N, d, M, k = 4200000, 128, 64, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, d, device="cuda", generator=g)
    first = (1 << 31) // (d * 4) + 1
    assert x.numel() * 4 > (1 << 31) and first < N - M
    rows = torch.linspace(first, N - 1, M, device="cuda").long()
    rows[-2] = N - 5
    assert int(rows.min()) * d * 4 >= (1 << 31) and int((rows >= N - 32).sum()) >= 2
    q = x[rows].contiguous()
    index, value = H.knn_search(q, x, k, metric="l2")
    assert torch.equal(index[:, 0].long(), rows)
    idx = index.long()
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    true = (q.double()[:, None, :] - x[idx].double()).pow(2).sum(2)                 # (M, k), float64, the direct form
    scale = q.double().pow(2).sum(1)[:, None] + x[idx].double().pow(2).sum(2)
    err = ((value.double() - true).abs() / (R.band(d) * scale)).cpu().numpy()
    print("past 2 GiB: value error max %.3f band (bound 2), rank 0 value max %.3e" % (float(err.max()), float(value[:, 0].max())))
    assert float(err.max()) <= 2.0
    xn = q.double().pow(2).sum(1)
    assert bool(((value[:, 0].double() >= 0) & (value[:, 0].double() <= 2 * R.band(d) * 2 * xn)).all())
    v = value.cpu().numpy()
    assert (np.diff(v, axis=1) >= 0).all() and (v[:, 1] > 1.0).all()                # the others are random rows: far away
    assert len(set(map(tuple, np.sort(idx.cpu().numpy(), axis=1)))) == M


# 8 ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bank_case():
    N, d = 4099, 32
    x, cls, _ = R.make(N, d, seed=7, spread=0.15, return_classes=True)
    x = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    p = R.make(257, d, seed=11, spread=0.15)
    p = (p / np.linalg.norm(p.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return x, cls.astype(np.int64), p


def _bank(x, cls, temperature=0.1):
    import torch
    from cet_pick_amd.utils.memory_bank import MemoryBank
    bank = MemoryBank(len(x), x.shape[1], 48, temperature)
    half = len(x) // 2
    bank.update(torch.from_numpy(x[:half]), torch.from_numpy(cls[:half]))
    bank.update(torch.from_numpy(x[half:]), torch.from_numpy(cls[half:]))
    bank.cuda()
    return bank


def test_memory_bank_mines_the_arbiters_neighbours():
    x, cls, _ = _bank_case()
    bank = _bank(x, cls)
    indices, accuracy, distances = bank.mine_nearest_neighbors(10)
    assert indices.shape == (len(x), 11) and distances.shape == (len(x), 11) and indices.dtype == np.int64
    R.check_knn(x, x, 11, "ip", indices, distances, what="mine_nearest_neighbors")
    assert accuracy == np.mean(cls[indices[:, 1:]] == cls[:, None])
    i2, d2 = bank.mine_nearest_neighbors(10, calculate_accuracy=False)
    assert np.array_equal(i2, indices) and np.array_equal(d2, distances)


def test_memory_bank_votes_like_the_reference_in_float64():
    """weighted_knn: exp(similarity / T) summed per class over the K = 100 nearest, argmax; knn: the class of the nearest.
    Rows whose float64 vote margin is <= 1e-4 of the vote sum are exempt, at most 1 % of them (checked first)."""
    x, cls, p = _bank_case()
    T, K, C = 0.1, 100, 48
    yi, yd = R.topk64(p, x, K, "ip")
    votes = np.zeros((len(p), C))
    np.add.at(votes, (np.arange(len(p))[:, None], cls[yi]), np.exp(yd / T))
    order = np.argsort(-votes, axis=1, kind="stable")
    top = np.take_along_axis(votes, order[:, :2], axis=1)
    decided = (top[:, 0] - top[:, 1]) > 1e-4 * votes.sum(1)
    assert (~decided).mean() <= 0.01
    import torch
    bank = _bank(x, cls, T)
    got = bank.weighted_knn(torch.from_numpy(p).cuda())
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(p),)
    got = got.cpu().numpy()
    print("weighted_knn: %d of %d rows exempt, %d differ" % (int((~decided).sum()), len(p), int((got != order[:, 0]).sum())))
    assert np.array_equal(got[decided], order[decided, 0])
    # knn: the nearest row's class, or the second's where float64 cannot be asked to tell the two apart
    near = bank.knn(torch.from_numpy(p).cuda()).cpu().numpy()
    tie = (yd[:, 0] - yd[:, 1]) < 2 * R.band(x.shape[1]) * R.scales64(p, x, "ip", yi[:, :1])[:, 0]
    assert np.array_equal(near[~tie], cls[yi[~tie, 0]]) and np.isin(near[tie], cls[yi[tie, :2]]).all()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_plot_2d_writes_the_neighbour_graph(tmp_path):
    N, d, K = 3000, 100, 12
    x = _data(N, d)
    rs = np.random.RandomState(11)
    names = np.array(["tomo_a", "tomo_b"])[rs.randint(2, size=N)]
    coords = rs.randint(20, 400, size=(N, 3)).astype(np.int64)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=names, coords=coords)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for tag, extra in (("plain", []), ("graph", ["--num_neighbor", str(K)])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path",
                            str(out), "--n_cluster", "0", "--k", "48", "--niter", "20"] + extra, cwd=REPO, env=env, timeout=300,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = (out, r.stdout)
    assert not (outs["plain"][0] / "knn_graph.npz").exists() and "knn_graph" not in outs["plain"][1]
    assert "knn_graph.npz" in outs["graph"][1] and "are not made here" in outs["graph"][1]
    z = np.load(outs["graph"][0] / "knn_graph.npz")
    assert z["index"].dtype == np.int32 and z["dist"].dtype == np.float32 and int(z["k"]) == K
    R.check_knn(x, x, K, "l2", z["index"], z["dist"], True, what="plot_2d --num_neighbor")
    # the k-means output does not change with the flag: every member, byte for byte (the zip container carries a time stamp)
    a, b = np.load(outs["plain"][0] / "kmeans_labels.npz"), np.load(outs["graph"][0] / "kmeans_labels.npz")
    assert sorted(a.files) == sorted(b.files)
    for f in a.files:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes(), f
