"""The UMAP arbiter (tests/umap_ref.py) against the published curve parameters and its own invariants, the range checks and the
host side of plot_2d --mode umap.  No GPU."""
import argparse
import contextlib

import numpy as np
import pytest

import tsne_ref as T
import umap_ref as U


def test_find_ab_reproduces_the_published_parameters():
    """min_dist 0.1: umap-learn's documented (1.577, 0.895) to all printed digits; 0.5 (the reference's default): recorded in
    the issue.  The product's fit and the arbiter's are the same scipy call."""
    from cet_pick_amd.utils.umap import find_ab_params
    want = {0.1: (1.5769434603, 0.8950608779), 0.5: (0.5830300203, 1.3341669924)}
    for md, ab in want.items():
        for got in (U.find_ab(md), find_ab_params(md)):
            assert np.abs(np.array(got) / np.array(ab) - 1).max() <= 1e-6, (md, got)


def test_fixture_records_what_the_generator_states(golden):
    z = golden("umap_small.npz")
    assert len(z["seq_seeds"]) >= 3 and z["seq_agree"].shape == z["seq_trust"].shape == z["seq_seeds"].shape
    assert float(z["trust_margin"]) == z["seq_trust"].max() - z["seq_trust"].min()
    assert np.abs(z["ab"] / np.array(U.find_ab(float(z["min_dist"]))) - 1).max() <= 1e-9
    assert float(z["sync_agree"]) >= z["seq_agree"].min() and float(z["sync_trust"]) >= z["seq_trust"].min() - float(z["trust_margin"])


def test_firing_counts_are_the_floor_of_epochs_over_spacing():
    rs = np.random.RandomState(2)
    eps = np.concatenate([[1.0, 2.0, 500.0, 499.99, 3.0, 1.5, np.inf], 1.0 / rs.uniform(1.0 / 500, 1.0, 200)])
    count = sum(U.fires(n, eps).astype(np.int64) for n in range(1, 501))
    assert np.array_equal(count, np.floor(500 / eps))
    assert count[0] == 500 and count[2] == 1 and count[6] == 0
    wsym = np.array([1.0, 0.5, 1.0 / 500, 0.999 / 500, 0.0])
    eps = U.spacing64(wsym, 1.0, 500)
    assert eps[:3].tolist() == [1.0, 2.0, 500.0] and np.isinf(eps[3:]).all()        # pruned below wmax / n_epochs


def _graph(n, k, seed):
    rs = np.random.RandomState(seed)
    index = np.stack([rs.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)])
    return index, rs.uniform(0.05, 1.0, (n, k))


def test_union_is_symmetric_and_incident_lists_every_pair_once():
    n, k = 60, 7
    index, w = _graph(n, k, 5)
    wsym, mutual, eps, wmax = U.union64(index, w, 500)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), k), index.reshape(-1)] = w.reshape(-1)
    W = A + A.T - A * A.T
    assert np.array_equal(W, W.T) and wmax == W.max()
    assert np.array_equal(wsym, W[np.repeat(np.arange(n), k), index.reshape(-1)].reshape(n, k))
    assert np.array_equal(mutual, (A.T > 0)[np.repeat(np.arange(n), k), index.reshape(-1)].reshape(n, k))
    assert 0 < mutual.sum() < n * k
    vert, slot, other, edge = U.incident(index, mutual)
    pairs = sorted(zip(vert.tolist(), other.tolist()))
    assert len(set(pairs)) == len(pairs)                                           # no pair twice in one vertex's list
    assert set(pairs) == {(i, j) for i in range(n) for j in range(n) if W[i, j] > 0}        # and every pair from both ends
    for i in range(n):
        m = vert == i
        assert slot[m].tolist() == list(range(m.sum())) and edge[m][:k].tolist() == list(range(i * k, i * k + k))
        assert (np.diff(edge[m][k:]) > 0).all() and (other[m][k:] == edge[m][k:] // k).all()
    assert np.array_equal(eps.reshape(-1)[edge], wmax / W[vert, other])            # one spacing per pair, from either end


def test_smooth_distances_hit_log2_k():
    x = T.make_blobs(120, 8, 3, seed=4)[0].astype(np.float64)
    d2 = np.sort(((x[:, None] - x[None]) ** 2).sum(2), 1)[:, 1:15].astype(np.float32)
    rho, sigma, w = U.smooth64(d2)
    d = U.distances(d2)
    assert np.array_equal(rho, d[:, 0]) and (sigma > 0).all()
    assert np.abs(w.sum(1) - np.log2(15)).max() < 1e-5 and (w[:, 0] == 1).all() and (np.diff(w, axis=1) <= 0).all()


def test_range_checks_refuse_what_the_kernels_refuse():
    """mi_umap_check is host code (the library has to exist: build() is a no-op when it is built already); the Python checks
    raise before anything is launched, so they run without a GPU."""
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    from cet_pick_amd.utils.umap import UMAP, check_range
    ok = _lib.lib().mi_umap_check
    assert ok(17, 15) == 0 and ok(129, 127) == 0 and ok(3, 1) == 0 and ok(100000, 39) == 0
    assert ok(129, 128) == -3 and ok(1000, 0) == -3 and ok(1000, -1) == -3         # columns outside 1..127
    assert ok(16, 15) == -3 and ok(2, 1) == -3                                     # N < k + 2
    assert ok(2 ** 31 // 100 + 1, 100) == -3 and ok(2 ** 31 // 100, 100) == 0      # N k >= 2^31
    for bad in (1, 129, 0, 5.5):
        with pytest.raises(ValueError, match="2..128"):
            check_range(1000, bad)
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        check_range(15, 15)
    check_range(16, 15)
    check_range(129, 128)
    check_range(3, 2)
    for k in (1, 129):
        with pytest.raises(ValueError, match="2..128"):
            UMAP(k, device="cpu").fit_transform(np.zeros((300, 4), np.float32))
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        UMAP(15, device="cpu").fit_transform(np.zeros((15, 4), np.float32))
    with pytest.raises(_lib.HipExtensionError):              # in range: and then there is no CPU path
        UMAP(15, device="cpu").fit_transform(np.zeros((100, 4), np.float32))


def test_plot_2d_umap_mode(tmp_path, monkeypatch, capsys):
    """An explicit --mode umap --num_neighbor 5 calls the map once (n_neighbors 5, min_dist 0.5, seed 42), makes one search and
    writes the graph and the map; the bare default (with or without --num_neighbor) and --mode umap without --num_neighbor
    call nothing new and print today's notices (Kmeans, the search and the maps are stubs)."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args
    base = ["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"), "--k", "4", "--niter", "2"]
    assert parse(base).mode == "umap" and parse(base + ["--mode", "umap"]).mode == "umap" and parse(base).min_dist_umap == 0.5
    assert parse(base + ["--mode", "anything"]).mode == "anything"               # no choices: what was accepted stays accepted
    x = T.make_blobs(40, 6, 3, seed=1)[0]
    np.savez(tmp_path / "in.npz", pred=x, name=np.array(["a"] * 40), coords=np.zeros((40, 3)))

    class Stub:
        made = 0

        def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
            self.k, self.niter = k, niter
            Stub.made += 1

        def train(self, p):
            self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

        def assign(self, p):
            return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]

    maps, searches, tsne = [], [], []

    def fake_map(projs, n_neighbors, min_dist, seed, device):
        maps.append((n_neighbors, min_dist, seed))
        y = np.random.RandomState(0).standard_normal((len(projs), 2)).astype(np.float32) * 7
        return np.zeros((len(projs), n_neighbors), np.int32), np.zeros((len(projs), n_neighbors), np.float32), y, 500, 0.583, 1.334

    monkeypatch.setattr(KM, "Kmeans", Stub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "umap_map", fake_map, raising=False)
    monkeypatch.setattr(P, "tsne_map", lambda *a: tsne.append(a))
    monkeypatch.setattr(P, "knn_graph", lambda projs, k, device: searches.append(k) or (np.zeros((len(projs), k), np.int32),
                                                                                        np.zeros((len(projs), k), np.float32)))
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    emb = tmp_path / "o" / "embeddings_2d.npz"
    P.main(parse(base))
    P.main(parse(base + ["--mode", "umap"]))
    out = capsys.readouterr().out
    assert not maps and not searches and not emb.exists() and out.count("--num_neighbor, --mode") == 2       # today's notice, twice
    P.main(parse(base + ["--num_neighbor", "5"]))
    out = capsys.readouterr().out
    assert not maps and searches == [5] and not emb.exists() and "(--mode, --min_dist_umap," in out and "embeddings_2d" not in out
    P.main(parse(base + ["--mode", "umap", "--num_neighbor", "5"]))
    out = capsys.readouterr().out
    assert maps == [(5, 0.5, 42)] and searches == [5] and not tsne               # one map, and no second search
    z = np.load(emb)
    assert sorted(z.files) == ["a", "b", "min_dist", "n_epochs", "n_neighbors", "seed", "y", "y01"]
    assert z["y"].shape == (40, 2) and z["y"].dtype == np.float32 and z["y01"].dtype == np.float32
    assert np.array_equal(z["y01"].min(0), [0, 0]) and np.array_equal(z["y01"].max(0), [1, 1])
    assert (int(z["n_neighbors"]), int(z["seed"]), int(z["n_epochs"]), float(z["min_dist"])) == (5, 42, 500, 0.5)
    assert (float(z["a"]), float(z["b"])) == (0.583, 1.334)
    g = np.load(tmp_path / "o" / "knn_graph.npz")
    assert g["index"].shape == (40, 5) and int(g["k"]) == 5
    assert "--mode umap --num_neighbor 5 writes" in out and "UMAP map of 40 picks, n_neighbors 5, min_dist 0.5, 500 epochs" in out
    P.main(parse(base + ["--mode", "umap", "--num_neighbor", "5", "--min_dist_umap", "0.1", "--map_seed", "7"]))
    assert maps[-1] == (5, 0.1, 7)
    made = Stub.made
    for bad in ("1", "129"):                                 # refused before the clustering starts
        with pytest.raises(ValueError, match="2..128"):
            P.main(parse(base + ["--mode", "umap", "--num_neighbor", bad]))
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        P.main(parse(base + ["--mode", "umap", "--num_neighbor", "40"]))
    assert Stub.made == made
