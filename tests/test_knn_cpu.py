"""The k-nearest-neighbour arbiter (tests/knn_ref.py) against a naive per-row argsort, the integer tie case, the interface of
MemoryBank and the host side of plot_2d --num_neighbor.  No GPU."""
import argparse
import contextlib
import inspect

import numpy as np
import pytest

import knn_ref as R


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("exclude_self", [False, True])
def test_arbiter_matches_a_naive_argsort(metric, exclude_self):
    x = R.make(300, 20, seed=5, spread=0.15)
    k = 7
    idx, val = R.topk64(x, x, k, metric, exclude_self, block=64)
    x64 = x.astype(np.float64)
    for i in range(300):
        v = x64 @ x64[i]
        if metric == "l2":
            v = ((x64 - x64[i]) ** 2).sum(1)                    # the direct form: the expanded one differs by rounding only
        cols = [j for j in np.argsort(-v if metric == "ip" else v, kind="stable") if not (exclude_self and j == i)][:k]
        assert idx[i].tolist() == cols
        assert np.allclose(val[i], v[cols], rtol=0, atol=1e-12)
    # check_knn takes the arbiter's own answer, and refuses a swapped pair, a repeated index and the row itself
    R.check_knn(x, x, k, metric, idx, val, exclude_self, what="arbiter")
    bad = idx.copy()
    bad[:, [0, k - 1]] = bad[:, [k - 1, 0]]
    with pytest.raises(AssertionError):
        R.check_knn(x, x, k, metric, bad, val, exclude_self)
    bad = idx.copy()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(AssertionError, match="twice"):
        R.check_knn(x, x, k, metric, bad, val, exclude_self)
    if exclude_self:
        bad = idx.copy()
        bad[:, 0] = np.arange(300)
        with pytest.raises(AssertionError, match="itself"):
            R.check_knn(x, x, k, metric, bad, val, exclude_self)


def test_cap_holds_on_the_arbiter_alone():
    for name, (N, d, k, spread) in R.CASES.items():
        x = R.make(N, d, seed=7, spread=spread)
        for metric in ("ip", "l2"):
            share = R.nonexact(x, x, k, metric, True)[4]
            print("case %s %s: %.4f %%" % (name, metric, 100 * share))
            assert share <= R.NONEXACT_CAP


def test_integer_tie_case_has_the_ties_it_claims():
    x = R.tie_case()
    N = len(x)
    a = R.TIE_ROWS[0]
    assert all(np.array_equal(x[r], x[a]) for r in R.TIE_ROWS)
    assert len({r // 32 for r in R.TIE_ROWS}) == len(R.TIE_ROWS)                    # four column tiles
    for n_split in (3, 7):
        assert len({R.split_of(r, N, n_split) for r in R.TIE_ROWS}) >= 3           # first, a middle and the last part
        assert R.split_of(R.TIE_ROWS[-1], N, n_split) == n_split - 1
    assert float(np.abs(x).max()) <= 3 and np.array_equal(x, np.round(x))
    for metric in ("ip", "l2"):
        idx, val = R.topk64(x, x, 17, metric, True)
        assert (np.diff(val[:, :16], axis=1) == 0).mean() > 0.3                     # equal values next to each other in most rows
        assert (val[:, 15] == val[:, 16]).mean() > 0.3                              # ... and across the k-th place
        for r in R.TIE_ROWS if metric == "l2" else ():                               # the copies lead each other's lists, lowest first
            assert idx[r, :3].tolist() == [c for c in R.TIE_ROWS if c != r] and (val[r, :3] == 0).all()


def test_memory_bank_has_the_reference_interface():
    from cet_pick_amd.utils.memory_bank import MemoryBank
    want = {                                                     # the reference's utils/memory_bank.py, by inspect.signature
        "__init__": "(self, n, dim, num_classes, temperature)",
        "weighted_knn": "(self, predictions)",
        "knn": "(self, predictions)",
        "mine_nearest_neighbors": "(self, topk, calculate_accuracy=True)",
        "reset": "(self)",
        "update": "(self, features, targets)",
        "to": "(self, device)",
        "cpu": "(self)",
        "cuda": "(self)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(MemoryBank, name))) == sig, name
    public = {n for n, f in vars(MemoryBank).items() if inspect.isfunction(f) and not n.startswith("_")}
    assert public == set(want) - {"__init__"}
    bank = MemoryBank(12, 4, 3, 0.1)
    assert (bank.n, bank.dim, bank.C, bank.K, bank.temperature, bank.ptr, bank.device) == (12, 4, 3, 100, 0.1, 0, "cpu")
    assert tuple(bank.features.shape) == (12, 4) and tuple(bank.targets.shape) == (12,)
    import torch
    assert bank.features.dtype == torch.float32 and bank.targets.dtype == torch.int64
    bank.update(torch.ones(5, 4), torch.arange(5))
    bank.update(2 * torch.ones(7, 4), torch.arange(7))
    assert bank.ptr == 12 and float(bank.features[5:].min()) == 2.0 and bank.targets[5:].tolist() == list(range(7))
    with pytest.raises(AssertionError):
        bank.update(torch.ones(1, 4), torch.zeros(1, dtype=torch.int64))
    bank.reset()
    assert bank.ptr == 0


def test_memory_bank_and_knn_search_have_no_cpu_path():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    from cet_pick_amd.utils.memory_bank import MemoryBank
    x = torch.zeros(64, 8)
    with pytest.raises(L.HipExtensionError):
        H.knn_search(x, x, 4)
    bank = MemoryBank(64, 8, 3, 0.1)
    bank.update(x, torch.zeros(64, dtype=torch.int64))
    bank.cpu()
    for call in (lambda: bank.mine_nearest_neighbors(5), lambda: bank.knn(x[:4]), lambda: bank.weighted_knn(x[:4])):
        with pytest.raises(L.HipExtensionError):
            call()


def test_size_entries_refuse_what_the_search_refuses():
    """The two size entries are host code, so they are called without a GPU; the library has to exist for that, hence the
    build() (a no-op when it is built already, a full compile of the HIP sources otherwise, as in test_abi.py)."""
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    ws, img = _lib.lib().mi_knn_workspace_bytes, _lib.lib().mi_knn_image_bytes
    assert ws(100, 4099, 128, 16, 0, 0) > img(4099, 128) > 4099 * 128 * 6
    assert ws(100, 4099, 128, 129, 0, 0) == 0                   # k > 128
    assert ws(100, 4099, 513, 16, 0, 0) == 0                    # d > 512
    assert ws(100, 15, 128, 16, 0, 0) == 0                      # N < k
    assert ws(16, 16, 128, 16, 0, 0) > 0 and ws(16, 16, 128, 16, 1, 0) == 0         # N = k; with exclude_self N >= k + 1
    assert ws(100, 4099, 128, 16, 0, 33) == 0                   # more splits than the merge takes
    assert ws(100, 4099, 128, 16, 0, 7) > ws(100, 4099, 128, 16, 0, 1)


def test_plot_2d_num_neighbor_is_parsed_and_off_by_default(tmp_path, monkeypatch, capsys):
    """The parser yields num_neighbor; main() without it writes no knn_graph.npz and makes no search (Kmeans is a stub)."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args
    base = ["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"), "--k", "4", "--niter", "2"]
    assert parse(base).num_neighbor is None and parse(base + ["--num_neighbor", "12"]).num_neighbor == 12
    x = R.make(40, 6, seed=1)
    np.savez(tmp_path / "in.npz", pred=x, name=np.array(["a"] * 40), coords=np.zeros((40, 3)))

    class Stub:
        def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
            self.k, self.niter = k, niter

        def train(self, p):
            self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

        def assign(self, p):
            return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]

    calls = []
    monkeypatch.setattr(KM, "Kmeans", Stub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "knn_graph", lambda projs, k, device: calls.append(k) or (np.zeros((len(projs), k), np.int32),
                                                                                     np.zeros((len(projs), k), np.float32)))
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    P.main(parse(base))
    out = capsys.readouterr().out
    assert not calls and not (tmp_path / "o" / "knn_graph.npz").exists() and (tmp_path / "o" / "kmeans_labels.npz").exists()
    assert "--num_neighbor, --mode" in out and "knn_graph" not in out            # today's notice, word for word
    P.main(parse(base + ["--num_neighbor", "5"]))
    out = capsys.readouterr().out
    z = np.load(tmp_path / "o" / "knn_graph.npz")
    assert calls == [5] and z["index"].shape == (40, 5) and z["index"].dtype == np.int32 and z["dist"].dtype == np.float32
    assert int(z["k"]) == 5 and "knn_graph.npz" in out and "are not made here" in out
