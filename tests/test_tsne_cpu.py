"""The t-SNE arbiter (tests/tsne_ref.py) against finite differences and against sklearn's recorded affinities, the graph
transpose, the range checks and the host side of plot_2d --mode tsne.  No GPU."""
import argparse
import contextlib

import numpy as np
import pytest

import tsne_ref as T


@pytest.fixture(scope="module")
def small(golden):
    return golden("tsne_small.npz")


def random_graph(n, k, seed):
    """index (n, k): k distinct other rows of every row, and conditional affinities whose rows sum to 1"""
    rs = np.random.RandomState(seed)
    index = np.stack([rs.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)])
    p = rs.uniform(0.1, 1.0, (n, k))
    return index, p / p.sum(1, keepdims=True)


@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_arbiter_gradient_is_the_derivative_of_its_divergence(exaggeration):
    """Central differences of the arbiter's own divergence at exaggeration 1.  With an exaggeration sklearn scales the
    attraction only, which is no longer the gradient of one function: there the two parts are differenced on their own,
    KL = sum P ln P + sum P ln(1 / q) + ln Z, grad = e d/dy [sum P ln(1 / q)] + d/dy ln Z."""
    n = 40
    index, pc = random_graph(n, 6, seed=3)
    P = T.joint_P(index, pc)
    Y = np.random.RandomState(4).standard_normal((n, 2))
    assert abs(P.sum() - 1) < 1e-12 and np.array_equal(P, P.T)

    def attraction_energy(Yf):                               # sum P ln(1 / q): its gradient is 4 sum P q (y_i - y_j)
        d2 = ((Yf[:, None, :] - Yf[None, :, :]) ** 2).sum(2)
        return float((P * np.log1p(d2)).sum())

    def log_z(Yf):                                           # its gradient is -4 sum q^2 (y_i - y_j) / Z
        d2 = ((Yf[:, None, :] - Yf[None, :, :]) ** 2).sum(2)
        q = 1.0 / (1.0 + d2)
        np.fill_diagonal(q, 0.0)
        return float(np.log(q.sum()))

    def numeric(f, h=1e-5):                                  # rounding 2^-52 |f| / h = 1e-10, truncation h^2 f''' / 6 = 1e-10
        g = np.zeros_like(Y)
        for i in range(n):
            for c in range(2):
                a, b = Y.copy(), Y.copy()
                a[i, c] += h
                b[i, c] -= h
                g[i, c] = (f(a) - f(b)) / (2 * h)
        return g

    grad, Z, kl, scale, klscale = T.grad_kl64(Y, P, exaggeration)
    want = exaggeration * numeric(attraction_energy) + numeric(log_z)
    assert np.abs(grad - want).max() <= 1e-7 * np.abs(want).max()
    assert abs(kl - (attraction_energy(Y) + log_z(Y) + float((P[P > 0] * np.log(P[P > 0])).sum()))) <= 1e-12 * klscale
    assert abs(Z - np.exp(log_z(Y))) <= 1e-12 * Z and (scale >= np.abs(grad).max(1)).all() and klscale >= abs(kl)
    if exaggeration == 1.0:                                  # and the whole thing at once: grad = d KL / d y
        assert np.abs(grad - numeric(lambda Yf: T.kl64(Yf, P))).max() <= 1e-7 * np.abs(grad).max()


def test_arbiter_joint_affinities_are_sklearns(small):
    """sklearn keeps the conditional affinities in float32 (2^-24 each, two per pair) and divides by their float32 sum (K
    roundings per row): (K + 4) 2^-24 relative."""
    index, dist, perplexity = small["index"].astype(np.int64), small["dist"], int(small["perplexity"])
    n, k = index.shape
    pc, beta = T.affinities64(dist, perplexity)
    assert np.abs(T.entropy_at(dist, beta)[1] - np.log(perplexity)).max() <= 1e-5 and np.abs(pc.sum(1) - 1).max() < 1e-12
    P = T.joint_P(index, pc)
    S = np.zeros((n, n))
    S[small["sk_row"].astype(np.int64), small["sk_col"].astype(np.int64)] = small["sk_val"]
    assert np.array_equal(P > 0, S > 0)
    rel = np.abs(P - S)[S > 0] / S[S > 0]
    print("joint affinities against sklearn's: max relative difference %.3e" % rel.max())
    assert rel.max() <= (k + 4) * 2.0 ** -24
    r, c, v = T.joint_P(index, pc, dense=False)
    assert np.array_equal(v, P[r, c]) and len(v) == int((P > 0).sum())


def test_fixture_records_what_the_generator_states(small):
    kl = small["sk_kl"]
    assert len(kl) == 5 and float(small["kl_margin"]) == 2 * (kl.max() - kl.min()) / kl.min() <= 0.5
    assert small["x"].shape == (600, 32) and small["sk_agree"].shape == (5,) and small["sk_agree"].min() > 0.9


@pytest.mark.parametrize("n,k", [(50, 7), (257, 16), (9, 8)])
def test_reverse_graph_is_the_exact_transpose(n, k):
    import torch
    from cet_pick_amd.utils.tsne import reverse_graph
    index = random_graph(n, k, seed=n)[0].astype(np.int32)
    index[0, :] = index[1, 0]                                # one row names the same destination k times
    ptr, edge = reverse_graph(torch.from_numpy(index))
    assert ptr.dtype == torch.int32 and edge.dtype == torch.int32 and tuple(ptr.shape) == (n + 1,) and tuple(edge.shape) == (n * k,)
    ptr, edge = ptr.numpy(), edge.numpy()
    assert ptr[0] == 0 and ptr[-1] == n * k and sorted(edge.tolist()) == list(range(n * k))
    flat = index.reshape(-1)
    for r in range(n):
        mine = edge[ptr[r]:ptr[r + 1]]
        assert mine.tolist() == np.nonzero(flat == r)[0].tolist()        # every edge into r, in ascending edge id
    with pytest.raises(ValueError):
        reverse_graph(torch.from_numpy(np.full((4, 2), 4, np.int32)))


def test_range_checks_refuse_what_the_kernels_refuse():
    """The size entry is host code (the library has to exist: build() is a no-op when it is built already); the Python checks
    raise before anything is launched, so they run without a GPU."""
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    from cet_pick_amd.utils.tsne import TSNE, check_range, n_neighbors
    ws = _lib.lib().mi_tsne_workspace_bytes
    assert ws(1031, 127, 0) > 0 and ws(17, 16, 0) > 0 and ws(100000, 91, 0) > 3 * 8 * 100000
    assert ws(1031, 128, 0) == 0                             # K of perplexity 43 (130) and of anything past 127
    assert ws(1031, 0, 0) == 0 and ws(16, 16, 0) == 0 and ws(1, 1, 0) == 0      # K >= 1, K <= N - 1
    assert ws(1031, 16, 33) == 0 and ws(1031, 16, -1) == 0 and ws(1031, 16, 32) > 0
    assert ws(1031, 16, 3) > ws(1031, 16, 1)
    assert n_neighbors(600, 5) == 16 and n_neighbors(17, 5) == 16 and n_neighbors(10, 5) == 9 and n_neighbors(10 ** 5, 42) == 127
    for bad in (1, 43, 0, 5.5):
        with pytest.raises(ValueError, match="2..42"):
            check_range(1000, bad)
    with pytest.raises(ValueError, match="perplexity \\+ 2"):
        check_range(6, 5)
    check_range(7, 5)
    check_range(44, 42)
    x = np.zeros((6, 4), np.float32)
    for p in (1, 43):
        with pytest.raises(ValueError, match="2..42"):
            TSNE(p, device="cpu").fit_transform(np.zeros((100, 4), np.float32))
    with pytest.raises(ValueError, match="perplexity \\+ 2"):
        TSNE(5, device="cpu").fit_transform(x)
    with pytest.raises(_lib.HipExtensionError):              # in range: and then there is no CPU path
        TSNE(5, device="cpu").fit_transform(np.zeros((100, 4), np.float32))


def test_update32_is_sklearns_step():
    y, g = np.array([[1.0, 2.0]], np.float32), np.array([[0.5, -0.5]], np.float32)
    v, gains = np.array([[0.25, 0.25]], np.float32), np.array([[1.0, 0.0125]], np.float32)
    y2, v2, g2 = T.update32(y, g, v, gains, 0.5, 2.0)
    assert g2.tolist() == [[np.float32(0.8), np.float32(0.0125) + np.float32(0.2)]]
    assert v2.tolist() == [[np.float32(0.5) * np.float32(0.25) - np.float32(2) * (np.float32(0.5) * g2[0, 0]),
                            np.float32(0.125) + np.float32(2) * (np.float32(0.5) * g2[0, 1])]]
    assert np.array_equal(y2, y + v2)
    assert T.update32(y, g, v, np.array([[0.012, 1.0]], np.float32), 0.5, 2.0)[2][0, 0] == np.float32(0.01)      # the floor


def test_plot_2d_tsne_mode(tmp_path, monkeypatch, capsys):
    """--mode tsne --num_neighbor 5 calls the map once (perplexity 5, seed 42) and writes both files; the default mode and
    --mode tsne without --num_neighbor call nothing new (Kmeans, the search and the map are stubs)."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args
    base = ["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"), "--k", "4", "--niter", "2"]
    assert parse(base).map_seed == 42 and parse(base).mode == "umap" and parse(base + ["--map_seed", "7"]).map_seed == 7
    x = T.make_blobs(40, 6, 3, seed=1)[0]
    np.savez(tmp_path / "in.npz", pred=x, name=np.array(["a"] * 40), coords=np.zeros((40, 3)))

    class Stub:
        def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
            self.k, self.niter = k, niter

        def train(self, p):
            self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

        def assign(self, p):
            return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]

    maps, searches = [], []

    def fake_map(projs, perplexity, seed, device):
        maps.append((perplexity, seed))
        y = np.random.RandomState(0).standard_normal((len(projs), 2)).astype(np.float32) * 30
        return np.zeros((len(projs), perplexity), np.int32), np.zeros((len(projs), perplexity), np.float32), y, 1.25, 999

    monkeypatch.setattr(KM, "Kmeans", Stub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "tsne_map", fake_map)
    monkeypatch.setattr(P, "knn_graph", lambda projs, k, device: searches.append(k) or (np.zeros((len(projs), k), np.int32),
                                                                                        np.zeros((len(projs), k), np.float32)))
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    emb = tmp_path / "o" / "embeddings_2d.npz"
    P.main(parse(base))
    P.main(parse(base + ["--mode", "tsne"]))
    out = capsys.readouterr().out
    assert not maps and not searches and not emb.exists() and out.count("--num_neighbor, --mode") == 2       # today's notice, twice
    P.main(parse(base + ["--num_neighbor", "5"]))
    assert not maps and searches == [5] and not emb.exists()
    capsys.readouterr()
    P.main(parse(base + ["--mode", "tsne", "--num_neighbor", "5"]))
    out = capsys.readouterr().out
    assert maps == [(5, 42)] and searches == [5]             # one map, and no second search
    z = np.load(emb)
    assert sorted(z.files) == ["kl", "n_iter", "perplexity", "seed", "y", "y01"]
    assert z["y"].shape == (40, 2) and z["y"].dtype == np.float32 and z["y01"].dtype == np.float32
    assert np.array_equal(z["y01"].min(0), [0, 0]) and np.array_equal(z["y01"].max(0), [1, 1])
    assert (int(z["perplexity"]), int(z["seed"]), int(z["n_iter"]), float(z["kl"])) == (5, 42, 999, 1.25)
    g = np.load(tmp_path / "o" / "knn_graph.npz")
    assert g["index"].shape == (40, 5) and int(g["k"]) == 5
    assert "embeddings_2d.npz" in out and "40 picks, perplexity 5, 999 iterations, KL 1.25" in out
    with pytest.raises(ValueError, match="2..42"):           # refused before the clustering starts
        P.main(parse(base + ["--mode", "tsne", "--num_neighbor", "43"]))
