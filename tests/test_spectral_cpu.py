"""The spectral-start arbiter (tests/spectral_ref.py) against its own invariants and the recorded fixture, the host helpers of
utils/spectral.py against it, the new options of UMAP and plot_2d, and the host side of plot_2d --umap_init spectral.  No GPU."""
import argparse
import contextlib

import numpy as np
import pytest

import spectral_ref as R
import tsne_ref as T

_cache = {}


def _graph(golden, which):
    if which not in _cache:
        n, K, seed = (int(v) for v in golden("spectral_small.npz")[which])
        x, _ = R.strip(n, seed)
        index, dist2 = R.knn(x, K - 1)
        wsym, mutual, eps = R.graph_tables(index, dist2, 500)
        _cache[which] = (x, index, dist2, R.dense_w(index, wsym, eps))
    return _cache[which]


@pytest.mark.parametrize("which", ["small", "strip"])
def test_reference_eigenpairs_and_fixture(golden, which):
    """The generator's asserts again, and the dense solve's residuals: one component, the recorded spectrum, gaps above the floor."""
    z = golden("spectral_small.npz")
    W = _graph(golden, which)[3]
    n = len(W)
    assert np.array_equal(W, W.T) and (np.diag(W) == 0).all() and (R.components(W) == 0).all()
    lam, v, gap = R.eigenpairs(W, 2)
    A, deg = R.normalised(W)
    assert np.abs(lam[:7] - z[which + "_lam"]).max() <= 1e-12 and np.abs(gap - z[which + "_gap"]).max() <= 1e-12
    assert gap.min() >= float(z["gap_floor"]) and abs(lam[0]) <= 1e-14
    res = np.linalg.norm((np.eye(n) - A) @ v - v * lam[1:3], axis=0)
    q0 = np.sqrt(deg) / np.linalg.norm(np.sqrt(deg))
    assert res.max() <= 1e-13 and np.abs(v.T @ q0).max() <= 1e-13 and np.abs(v.T @ v - np.eye(2)).max() <= 1e-13
    for a in range(2):
        assert v[np.argmax(np.abs(v[:, a])), a] > 0


def test_sign_rule_takes_the_lowest_index_on_ties():
    assert np.array_equal(R.sign_rule(np.array([0.5, -2.0, 2.0])), [-0.5, 2.0, -2.0])
    assert np.array_equal(R.sign_rule(np.array([0.5, 2.0, -2.0])), [0.5, 2.0, -2.0])
    assert np.array_equal(R.sign_rule(np.array([-1.0, 0.25])), [1.0, -0.25])


def test_centres_for_one_to_nine_components():
    from cet_pick_amd.utils import spectral as S
    want = {1: [[1, 0]], 2: [[1, 0], [-1, 0]], 3: [[1, 0], [0, 1], [-1, 0]], 4: [[1, 0], [0, 1], [-1, 0], [0, -1]]}
    rs = np.random.RandomState(3)
    for c in range(1, 10):
        z = rs.uniform(0, 2, (c, 5))
        centres = R.centres_of(c, 2, z)
        assert centres.shape == (c, 2)
        if c <= 4:
            assert np.array_equal(centres, np.array(want[c], np.float64)) and np.array_equal(S.fixed_centres(c, 2), centres)
        else:
            e, lam = R.eigh_centres(z, 2)
            assert np.abs(centres).max() == 1.0 and abs(lam[0]) <= 1e-14 and lam[1] > 1e-6
            for a in range(2):
                assert centres[np.argmax(np.abs(centres[:, a])), a] > 0
            assert len({tuple(np.round(r, 9)) for r in centres}) == c                   # no two components share a centre
            assert np.abs(S.eigh_centres(z, 2) - centres).max() <= 1e-12
        if c > 1:
            ranges = R.data_ranges(centres)
            assert (ranges > 0).all() and np.array_equal(ranges, S.data_ranges(centres))
            d = np.sqrt(((centres[:, None] - centres[None]) ** 2).sum(2))
            assert all(np.isclose(ranges[a], np.delete(d[a], a).min() / 2) for a in range(c))


def test_layout_of_several_components_stays_in_its_boxes():
    """Three blocks joined by nothing, one of them below the size limit: centres, boxes and the small block's uniform draws."""
    rs = np.random.RandomState(0)
    sizes, W = [12, 3, 9], np.zeros((24, 24))
    at = 0
    for m in sizes:
        B = np.triu(rs.uniform(0.1, 1.0, (m, m)), 1)
        W[at:at + m, at:at + m] = B + B.T
        at += m
    Y, info = R.layout(W, 2, seed=42)
    assert info["n_components"] == 3 and info["sizes"].tolist() == sizes and np.array_equal(np.unique(info["labels"]), [0, 12, 15])
    assert np.array_equal(info["centres"], [[1, 0], [0, 1], [-1, 0]]) and np.allclose(info["data_range"], np.sqrt(2) / 2)
    for a, m in enumerate(np.split(np.arange(24), [12, 15])):
        off = np.abs(Y[m] - info["centres"][a])
        assert off.max() <= info["data_range"][a] * (1 + 1e-12)
        if a != 1:
            assert np.isclose(off.max(), info["data_range"][a])
    assert np.array_equal(Y[12:15], np.random.RandomState(42).uniform(-info["data_range"][1], info["data_range"][1], (3, 2)) + [0, 1])


def test_start_lies_in_0_10_and_matches_the_product(golden):
    from cet_pick_amd.utils import spectral as S
    W = _graph(golden, "small")[3]
    Y = R.layout(W, 2, 42)[0]
    y0 = R.start(Y, 42)
    assert y0.dtype == np.float32 and y0.shape == (len(W), 2)
    assert np.array_equal(y0.min(0), [0, 0]) and np.array_equal(y0.max(0), [10, 10])
    assert S.umap_start(Y, 42).tobytes() == y0.tobytes()
    assert S.basis_size(600, 2) == 25 and S.basis_size(96, 2) == 10 and S.basis_size(10, 2) == 5 and S.basis_size(4, 2) == 3
    assert S.basis_size(600, 2, 2) == 4 and S.MAX_RESTARTS == 300 and S.MAX_COMPONENTS == 256


def test_umap_init_option():
    from cet_pick_amd.utils.umap import UMAP
    um = UMAP(15, init="spectral", device="cpu")
    assert um.init == "spectral" and um.init_ is None and um.n_components_ is None and um.eigenvalues_ is None
    assert UMAP(15, device="cpu").init == "random"
    with pytest.raises(ValueError, match="random, spectral"):
        UMAP(15, init="pca")


def test_plot_2d_umap_init(tmp_path, monkeypatch, capsys):
    """--umap_init spectral passes init="spectral" to the map and adds init, n_graph_components and eigenvalues to
    embeddings_2d.npz; the default command line calls the map as before and writes no new field (Kmeans and the map are stubs)."""
    import torch
    from cet_pick_amd import plot_2d as P
    from cet_pick_amd.utils import kmeans as KM
    parse = P.add_arguments(argparse.ArgumentParser()).parse_args
    base = ["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"), "--k", "4", "--niter", "2", "--mode", "umap",
            "--num_neighbor", "5"]
    assert parse(base).umap_init == "random" and parse(base + ["--umap_init", "spectral"]).umap_init == "spectral"
    with pytest.raises(SystemExit):
        parse(base + ["--umap_init", "pca"])
    x = T.make_blobs(40, 6, 3, seed=1)[0]
    np.savez(tmp_path / "in.npz", pred=x, name=np.array(["a"] * 40), coords=np.zeros((40, 3)))

    class Stub:
        def __init__(self, d, k, niter=300, seed=1234, device="cuda"):
            self.k, self.niter = k, niter

        def train(self, p):
            self.centroids, self.obj = p[:self.k].copy(), np.ones(self.niter, np.float32)

        def assign(self, p):
            return np.zeros((len(p), 1), np.float32), (np.arange(len(p)) % self.k).astype(np.int64)[:, None]

    calls = []

    def fake_map(projs, n_neighbors, min_dist, seed, device, **kw):
        calls.append(kw)
        y = np.random.RandomState(0).standard_normal((len(projs), 2)).astype(np.float32) * 7
        out = np.zeros((len(projs), n_neighbors), np.int32), np.zeros((len(projs), n_neighbors), np.float32), y, 500, 0.583, 1.334
        return out + (("spectral", 2, np.array([0.01, 0.04])),) if kw.get("init") == "spectral" else out

    monkeypatch.setattr(KM, "Kmeans", Stub)
    monkeypatch.setattr(torch.cuda, "device", lambda *a: contextlib.nullcontext())
    monkeypatch.setattr(P, "umap_map", fake_map)
    monkeypatch.setattr(P, "write_parquet", lambda *a: False)
    emb = tmp_path / "o" / "embeddings_2d.npz"
    old = ["a", "b", "min_dist", "n_epochs", "n_neighbors", "seed", "y", "y01"]
    P.main(parse(base))
    out = capsys.readouterr().out
    assert calls == [{}] and sorted(np.load(emb).files) == old and "--umap_init" not in out and "UMAP start" not in out
    P.main(parse(base + ["--umap_init", "spectral"]))
    out = capsys.readouterr().out
    z = np.load(emb)
    assert calls[-1] == {"init": "spectral"} and sorted(z.files) == sorted(old + ["init", "n_graph_components", "eigenvalues"])
    assert str(z["init"]) == "spectral" and int(z["n_graph_components"]) == 2 and z["eigenvalues"].tolist() == [0.01, 0.04]
    assert np.array_equal(z["y01"].min(0), [0, 0]) and np.array_equal(z["y01"].max(0), [1, 1])
    assert "UMAP start spectral (--umap_init spectral), 2 graph components" in out
