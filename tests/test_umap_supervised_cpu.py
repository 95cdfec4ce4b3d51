"""The arbiter of the label-supervised UMAP map (tests/umap_sup_ref.py): its closed form per directed edge against
the scipy.sparse / sklearn calls umap-learn makes, the properties the device code relies on, the argument checks of UMAP and
plot_2d --label_map, and plot_2d's host side with stubs.  No GPU."""
import argparse
import contextlib

import numpy as np
import pytest

import spectral_ref as S
import tsne_ref as T
import umap_ref as U
import umap_sup_ref as R

# Both forms make the same six roundings per edge (s = w f, p = s / m_i, q = s / m_j, p + q, p q, the difference), every one
# 2^-53 relative on a value <= 2, and d wsup / dp = 1 - q lies in [0, 1], so nothing is amplified: s 1 u relative, p and q 2 u
# absolute, p + q 4 u + 2 u, p q 4 u + u, the difference 11 u + u = 12 u from the exact value on either side, u = 2^-53.
BAND = 24 * 2.0 ** -53
N_EPOCHS = 500


def small_graph():
    """40 points in three blobs, K = 8: index (40, 7) int64 and the union's weights as the device holds them (fp32)."""
    x = T.make_blobs(40, 6, 3, seed=40)[0]
    index, dist2 = S.knn(x, 7)
    w = U.smooth64(dist2)[2].astype(np.float32)
    return index, U.union64(index, w, N_EPOCHS)[0].astype(np.float32).astype(np.float64)


def hub_graph():
    """The hub graph of test_umap_gpu.py from a float64 search: N = 300, K = 14, vertex 0 with more than 64 reverse edges,
    vertex N - 1 with none."""
    N, K = 300, 14
    x = T.make_blobs(N, 12, 3, seed=N)[0]
    x[N - 1] += 100.0
    index, dist2 = S.knn(x, K - 1)
    index = index.copy()
    for r in range(20, 120):
        if 0 not in index[r]:
            index[r, -1] = 0
    assert (index == 0).sum() > 64 and (index == N - 1).sum() == 0
    w = U.smooth64(dist2)[2].astype(np.float32)
    return index, U.union64(index, w, N_EPOCHS)[0].astype(np.float32).astype(np.float64)


def label_sets(n):
    """(labels, target_weight).  The blobs of both graphs are arange(n) % 3, so classes taken modulo 4 cut across them."""
    mixed = np.arange(n) % 4
    mixed[[1, 4, 11, n - 2]] = -1
    return {"mixed": (mixed, 0.5), "equal": (np.full(n, 2), 0.5), "distinct": (np.arange(n), 0.5), "weight one": (np.arange(n) % 4, 1.0),
            "distinct, weight one": (np.arange(n), 1.0)}


def test_far_dist_and_factors():
    assert R.far_dist(0.5) == 5.0 and R.far_dist(1.0) == 1e12 and R.far_dist(0.0) == 2.5
    assert R.factors(0.5) == (float(np.exp(-5.0)), float(np.exp(-1.0)))
    assert R.factors(1.0)[0] == 0.0                                           # exp(-1e12) is exactly zero
    from cet_pick_amd.utils import umap as M
    assert M.far_dist(0.5) == 5.0 and M.far_dist(1.0) == 1e12 and M.UNKNOWN_DIST == 1.0


@pytest.mark.parametrize("graph", [small_graph, hub_graph])
def test_closed_form_equals_the_sparse_calls(graph):
    index, wsym = graph()
    n, k = index.shape
    i, j = np.repeat(np.arange(n), k), index.reshape(-1)
    for name, (label, tw) in label_sets(n).items():
        f = R.factors(tw)
        wsup, m = R.supervise64(index, wsym, label, *f)
        wsp, msp = R.supervise_sparse64(index, wsym, label, *f)
        err = np.abs(wsup - wsp).max() / BAND
        print("%s N=%d k=%d: |closed form - sparse| max %.4f of 24 2^-53, rowmax equal %s, %d of %d edges zero, max %.17g"
              % (name, n, k, err, np.array_equal(m, msp), (wsup == 0).sum(), wsup.size, wsup.max()))
        assert err <= 1.0 and np.array_equal(m, msp)
        assert wsup.min() >= 0.0 and wsup.max() <= 1.0
        alive = wsup > 0
        if alive.any():                                      # every vertex's strongest pair has p = 1
            assert np.float32(wsup.max()) == 1.0 and abs(wsup.max() - 1.0) <= 2.0 ** -52
            top = np.zeros(n)
            np.maximum.at(top, i, wsup.reshape(-1))
            np.maximum.at(top, j, wsup.reshape(-1))
            assert (np.float32(top[m > 0]) == 1.0).all() and (top[m == 0] == 0).all()
        li, lj = label[i], label[j]
        cross = ((li != lj) & (li >= 0) & (lj >= 0)).reshape(n, k)
        if tw == 1.0:
            assert (wsup[cross] == 0).all() and cross.any()
            lonely = np.nonzero(m == 0)[0]                   # a vertex all of whose pairs cross classes: an all-zero row
            assert name != "distinct, weight one" or (len(lonely) == n and not alive.any())
            for v in lonely:
                assert (wsup[v] == 0).all() and (wsup.reshape(-1)[j == v] == 0).all()
        if name == "equal":                                  # the factor is 1 everywhere: the reset alone
            assert np.array_equal(R.supervise64(index, wsym, label, 0.0, 0.0)[0], wsup)
        # symmetric across the two directed edges of a mutual pair, bit for bit
        at = {(a, b): v for a, b, v in zip(i.tolist(), j.tolist(), wsup.reshape(-1).tolist())}
        assert all(at[(b, a)] == v for (a, b), v in at.items() if (b, a) in at)


def test_spacings_of_the_supervised_graph():
    """graph64 prunes and spaces the supervised weights as the plain fit does its own: eps = max / wsup from the fp32 values."""
    x, label = T.make_blobs(40, 6, 3, seed=40)[0], np.arange(40) % 4
    index, dist2 = S.knn(x, 7)
    inc, eps, wsup = R.graph64(index, dist2, label, N_EPOCHS, 1.0)
    assert wsup.dtype == np.float32 and wsup.max() == 1.0
    assert np.array_equal(np.isinf(eps), wsup < 1.0 / N_EPOCHS) and (eps[np.isfinite(eps)] >= 1.0).all()
    cross = label[np.repeat(np.arange(40), 7)] != label[index.reshape(-1)]
    assert cross.any() and np.isinf(eps.reshape(-1)[cross]).all() and np.isfinite(eps).any()


def test_umap_refuses_bad_targets_before_any_launch():
    """device="cpu": a call that got as far as the device would raise HipExtensionError, as the last one does."""
    from cet_pick_amd import _lib
    from cet_pick_amd.utils.umap import UMAP, check_labels, check_target_weight
    x = np.zeros((100, 4), np.float32)
    good = np.arange(100) % 3
    for y, what in ((good[:99], "shape"), (good.reshape(100, 1), "shape"), (good.astype(np.float32), "integer"),
                    (np.where(good == 0, -2, good), "-1")):
        with pytest.raises(ValueError, match=what):
            UMAP(15, device="cpu").fit_transform(x, y=y)
    for tw in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target_weight"):
            UMAP(15, device="cpu", target_weight=tw).fit_transform(x, y=good)
        with pytest.raises(ValueError, match="target_weight"):
            check_target_weight(tw)
    with pytest.raises(ValueError, match="2..128"):          # the plain checks come first
        UMAP(1, device="cpu").fit_transform(x, y=good)
    um = UMAP(15, device="cpu", target_weight=1.0)
    assert um.supervised_ is False and um.far_dist_ is None
    with pytest.raises(_lib.HipExtensionError):              # in range: and then there is no CPU path
        um.fit_transform(x, y=good)
    assert um.supervised_ is True and um.far_dist_ == 1e12
    with pytest.raises(_lib.HipExtensionError):              # target_weight is not looked at without y
        UMAP(15, device="cpu", target_weight=7).fit_transform(x)
    got = check_labels(np.array([-1, 0, 5], np.int64), 3)
    assert got.dtype == np.int32 and got.tolist() == [-1, 0, 5] and got.flags.c_contiguous


LISTED = ["a", "b", "far_dist", "label", "min_dist", "n_epochs", "n_neighbors", "seed", "target_weight", "y", "y01"]


def test_plot_2d_label_map(tmp_path, monkeypatch, capsys):
    """--label_map --num_neighbor 5 under no --mode, --mode umap and --mode tsne calls the supervised map once, with the classes
    of the class table and the table of the search already made, and writes the listed keys; without the flag nothing new is
    written and embeddings_2d.npz keeps its keys (Kmeans, the search and the maps are stubs)."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args
    base = ["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"), "--k", "4", "--niter", "2"]
    assert parse(base).label_map is False and parse(base).target_weight == 0.5 and parse(base + ["--label_map"]).label_map is True
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

    calls, searches = [], []
    table = lambda n, k: (np.tile(np.arange(1, k + 1, dtype=np.int32), (n, 1)), np.ones((n, k), np.float32))       # noqa: E731
    rand = lambda n: np.random.RandomState(0).standard_normal((n, 2)).astype(np.float32) * 7                        # noqa: E731

    def fake_label_map(projs, index, dist, label, n_neighbors, min_dist, seed, device, init="random", target_weight=0.5):
        calls.append(dict(index=index, dist=dist, label=label, args=(n_neighbors, min_dist, seed, init, target_weight)))
        start = None if init == "random" else ("spectral", 3, np.array([0.1, 0.2]))
        return rand(len(projs)) + 1, 500, 0.583, 1.334, 5.0, start

    def fake_map(projs, n_neighbors, min_dist, seed, device):
        return table(len(projs), n_neighbors) + (rand(len(projs)), 500, 0.583, 1.334)

    def fake_search(projs, k, device):
        searches.append(k)
        return table(len(projs), k)

    monkeypatch.setattr(KM, "Kmeans", Stub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "umap_label_map", fake_label_map)
    monkeypatch.setattr(P, "umap_map", fake_map)
    monkeypatch.setattr(P, "tsne_map", lambda projs, k, seed, device: table(len(projs), k) + (rand(len(projs)), 1.25, 1000))
    monkeypatch.setattr(P, "knn_graph", fake_search)
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    emb, sup = tmp_path / "o" / "embeddings_2d.npz", tmp_path / "o" / "embeddings_2d_labels.npz"

    P.main(parse(base + ["--mode", "umap", "--num_neighbor", "5"]))          # without the flag: nothing new
    out = capsys.readouterr().out
    assert not calls and not sup.exists() and "supervised" not in out and "--label_map" not in out
    assert sorted(np.load(emb).files) == ["a", "b", "min_dist", "n_epochs", "n_neighbors", "seed", "y", "y01"]
    plain = emb.read_bytes()

    want_label = (np.arange(40) % 4).astype(np.int32)
    for mode, n_search in (([], 1), (["--mode", "umap"], 0), (["--mode", "tsne"], 0)):
        calls.clear()
        searches.clear()
        P.main(parse(base + mode + ["--num_neighbor", "5", "--label_map"]))
        out = capsys.readouterr().out
        assert len(calls) == 1 and len(searches) == n_search, mode           # one supervised map, and no second search
        c = calls[0]
        assert c["args"] == (5, 0.5, 42, "random", 0.5) and np.array_equal(c["label"], want_label) and c["label"].dtype == np.int32
        assert c["index"].shape == (40, 5) and np.array_equal(c["index"][:, :4], table(40, 5)[0][:, :4])
        z = np.load(sup)
        assert sorted(z.files) == LISTED
        assert np.array_equal(z["label"], np.load(tmp_path / "o" / "kmeans_labels.npz")["label"]) and z["label"].dtype == np.int32
        assert z["y"].shape == (40, 2) and z["y"].dtype == np.float32 and z["y01"].dtype == np.float32
        assert np.array_equal(z["y01"].min(0), [0, 0]) and np.array_equal(z["y01"].max(0), [1, 1])
        assert (int(z["n_neighbors"]), int(z["seed"]), int(z["n_epochs"]), float(z["min_dist"])) == (5, 42, 500, 0.5)
        assert (float(z["a"]), float(z["b"]), float(z["target_weight"]), float(z["far_dist"])) == (0.583, 1.334, 0.5, 5.0)
        assert out.count("label-supervised UMAP map of 40 picks in 4 classes") == 1 and "embeddings_2d_labels.npz" in out
        if mode == ["--mode", "umap"]:
            assert emb.read_bytes() == plain                 # the plain map does not notice
        sup.unlink()
    calls.clear()
    P.main(parse(base + ["--num_neighbor", "5", "--label_map", "--umap_init", "spectral", "--target_weight", "1", "--min_dist_umap", "0.1",
                         "--map_seed", "7"]))
    assert calls[0]["args"] == (5, 0.1, 7, "spectral", 1.0)
    z = np.load(sup)
    assert sorted(z.files) == sorted(LISTED + ["eigenvalues", "init", "n_graph_components"])
    assert str(z["init"]) == "spectral" and int(z["n_graph_components"]) == 3 and z["eigenvalues"].tolist() == [0.1, 0.2]
    assert float(z["target_weight"]) == 1.0

    made, n_calls = Stub.made, len(calls)                    # refused before the clustering starts
    with pytest.raises(ValueError, match="--num_neighbor"):
        P.main(parse(base + ["--label_map"]))
    with pytest.raises(ValueError, match="--num_neighbor"):
        P.main(parse(base + ["--mode", "tsne", "--label_map"]))
    for bad in ("1", "129"):
        with pytest.raises(ValueError, match="2..128"):
            P.main(parse(base + ["--num_neighbor", bad, "--label_map"]))
    with pytest.raises(ValueError, match="n_neighbors \\+ 1"):
        P.main(parse(base + ["--num_neighbor", "40", "--label_map"]))
    with pytest.raises(ValueError, match="target_weight"):
        P.main(parse(base + ["--num_neighbor", "5", "--label_map", "--target_weight", "1.5"]))
    assert Stub.made == made and len(calls) == n_calls
