"""The k-means arbiter (tests/kmeans_ref.py) pinned to sklearn, the empty-cluster rule on hand-made counts, and the host side of
plot_2d / interactive_to_training_coords.  No GPU."""
import argparse
import os
import sys
import types

import numpy as np
import pytest

import kmeans_ref as R


@pytest.mark.parametrize("name", ["A", "C"])
def test_arbiter_matches_sklearn_lloyd(name):
    sk = pytest.importorskip("sklearn.cluster")
    N, d, k, spread = R.CASES[name]
    x = R.make(N, d, seed=7, spread=spread).astype(np.float64)
    c = x[R.init_rows(N, k)].copy()
    for _ in range(6):
        c, counts, labels, dist, served = R.lloyd_step(x, c)
        assert not served and (counts > 0).all()         # sklearn's own relocation rule never acts
    km = sk.KMeans(n_clusters=k, init=x[R.init_rows(N, k)].copy(), n_init=1, algorithm="lloyd", tol=0, max_iter=6).fit(x)
    final_labels, final_dist, _, _, _ = R.assign64(x, c)
    assert np.array_equal(km.labels_, final_labels)
    assert abs(km.inertia_ - final_dist.sum()) <= 1e-9 * final_dist.sum()


def test_split_rule_on_hand_made_counts():
    cent = np.arange(1, 25, dtype=np.float64).reshape(6, 4)
    counts = np.array([9, 0, 9, 0, 5, 0])
    c, n, served = R.split_rule(cent, counts)
    # cluster 1 takes from 0 (first of the two nines); cluster 3 from 2 (9 beats 5, 5, 4); cluster 5 from 0 or 4: 5 (index 0) ties 5
    assert served == [(1, 0), (3, 2), (5, 0)]
    assert n.tolist() == [3, 4, 5, 4, 5, 2] and n.sum() == counts.sum()
    e = R.EPS
    assert np.allclose(c[1], cent[0] * [1 + e, 1 - e, 1 + e, 1 - e], rtol=1e-15)
    assert np.allclose(c[3], cent[2] * [1 + e, 1 - e, 1 + e, 1 - e], rtol=1e-15)
    assert np.allclose(c[2], cent[2] * [1 - e, 1 + e, 1 - e, 1 + e], rtol=1e-15)
    once = cent[0] * [1 - e, 1 + e, 1 - e, 1 + e]          # cluster 0 gave twice
    assert np.allclose(c[5], once * [1 + e, 1 - e, 1 + e, 1 - e], rtol=1e-15)
    assert np.allclose(c[0], once * [1 - e, 1 + e, 1 - e, 1 + e], rtol=1e-15)
    assert np.array_equal(c[4], cent[4])


def _table(tmp_path, n=40):
    rs = np.random.RandomState(0)
    names = np.array(["t1", "t2"])[rs.randint(2, size=n)]
    coords = np.round(rs.rand(n, 3) * 300, 1)
    coords[::3] = np.floor(coords[::3])
    labels = rs.randint(5, size=n).astype(np.int32)
    return names, coords, labels


def _run_convert(inp, out, if_double=False, labels=None):
    from cet_pick_amd import interactive_to_training_coords as T
    return T.main(argparse.Namespace(input=str(inp), output=str(out), if_double=if_double, labels=labels))


def test_npz_to_table_to_the_semi_loader(tmp_path):
    from cet_pick_amd.datasets.semi_files import read_coord_list
    names, coords, labels = _table(tmp_path)
    coords = coords.astype(np.int64)
    np.savez(tmp_path / "kmeans_labels.npz", name=names, coords=coords, label=labels, assign=labels)
    out = tmp_path / "training_coordinates.txt"
    assert _run_convert(tmp_path / "kmeans_labels.npz", out, labels="1,3") == int(np.isin(labels, [1, 3]).sum())
    keep = np.isin(labels, [1, 3])
    got = read_coord_list(str(out), ["t1", "t2"])
    for t in ("t1", "t2"):
        assert np.array_equal(got[t], coords[keep & (names == t)].astype(np.int32))
    _run_convert(tmp_path / "kmeans_labels.npz", out, if_double=True)
    got = read_coord_list(str(out), ["t1", "t2"])
    for t in ("t1", "t2"):
        assert np.array_equal(got[t], (coords[names == t] * [1, 1, 2]).astype(np.int32))


def test_parquet_to_table_is_byte_identical_to_the_reference_arithmetic(tmp_path):
    pd = pytest.importorskip("pandas")
    pytest.importorskip("pyarrow")
    from cet_pick_amd import plot_2d as P
    names, coords, labels = _table(tmp_path)
    projs = np.random.RandomState(1).randn(len(names), 8).astype(np.float32)
    folder = tmp_path / "exported"
    folder.mkdir()
    assert P.write_parquet(str(folder / "a.parquet"), names, coords, projs, labels, 7000)
    df = pd.read_parquet(folder / "a.parquet")
    assert list(df.columns) == ["name", "coord", "embeddings", "label", "image"]
    assert isinstance(df["name"][0], str) and isinstance(df["image"][0], str)
    assert len(df["coord"][0]) == 3 and all(isinstance(v, str) for v in df["coord"][0])
    assert df["coord"][1].tolist() == [str(v) for v in coords[1]]
    assert np.asarray(df["embeddings"][0]).dtype == np.float32 and len(df["embeddings"][0]) == 8
    assert np.issubdtype(df["label"].dtype, np.integer)
    assert df["image"][3] == "http://localhost:7000/imgs/3.png"
    for dbl in (False, True):
        # the table the reference's arithmetic gives for the same rows: header, tabs, str(float(z) * 2)
        want = "\t".join(["image_name", "x_coord", "y_coord", "z_coord"]) + "\n"
        for n, (x, y, z) in zip(names, [[str(v) for v in c] for c in coords]):
            if dbl:
                z = str(float(z) * 2)
            want += "\t".join([n, x, y, z]) + "\n"
        out = tmp_path / ("t%d.txt" % dbl)
        _run_convert(folder, out, if_double=dbl)                         # a folder of *.parquet
        assert open(out, "rb").read() == want.encode()
        _run_convert(folder / "a.parquet", out, if_double=dbl)           # one file
        assert open(out, "rb").read() == want.encode()
    out = tmp_path / "sel.txt"
    assert _run_convert(folder, out, labels="2") == int((labels == 2).sum())
    assert "rec_path" not in open(sys.modules["cet_pick_amd.interactive_to_training_coords"].__file__).read()


def test_spectral_merge_is_called_with_the_reference_arguments(monkeypatch):
    from cet_pick_amd import plot_2d as P
    seen = {}

    class Stub:
        def __init__(self, **kw):
            seen["kw"] = kw

        def fit(self, c):
            seen["fit"] = c
            self.labels_ = np.arange(len(c)) % seen["kw"]["n_clusters"]

    sk, skc = types.ModuleType("sklearn"), types.ModuleType("sklearn.cluster")
    skc.SpectralClustering = Stub
    sk.cluster = skc
    monkeypatch.setitem(sys.modules, "sklearn", sk)
    monkeypatch.setitem(sys.modules, "sklearn.cluster", skc)
    c = np.random.RandomState(0).randn(16, 4).astype(np.float32)
    y = P.merge_centroids(c, 5)
    assert seen["kw"] == {"n_clusters": 5, "assign_labels": "discretize", "random_state": 0}
    assert seen["fit"] is c and np.array_equal(y, np.arange(16) % 5)
    monkeypatch.setitem(sys.modules, "sklearn.cluster", None)            # sklearn does not import
    with pytest.raises(RuntimeError, match="--n_cluster 0"):
        P.merge_centroids(c, 5)


def test_host_tensors_and_cpu_mode_raise(tmp_path):
    import torch
    from cet_pick_amd import _lib as L, hipops as H, plot_2d as P
    from cet_pick_amd.utils.kmeans import Kmeans
    x = torch.zeros(64, 8)
    with pytest.raises(L.HipExtensionError):
        H.kmeans_xnorm(x)
    with pytest.raises(L.HipExtensionError):
        H.kmeans_prep(x[:4])
    with pytest.raises(L.HipExtensionError):
        H.kmeans_assign(x, x[:, 0], torch.zeros(16, dtype=torch.uint8), 4)
    with pytest.raises(L.HipExtensionError):
        H.kmeans_update(x, torch.zeros(64, dtype=torch.int32), x[:4].clone())
    with pytest.raises(L.HipExtensionError):
        Kmeans(8, 4, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(L.HipExtensionError):
            Kmeans(8, 4)._device_x(x)
    np.savez(tmp_path / "in.npz", pred=np.zeros((8, 4), np.float32), name=np.array(["a"] * 8), coords=np.zeros((8, 3)))
    args = P.add_arguments(argparse.ArgumentParser()).parse_args(["--input", str(tmp_path / "in.npz"), "--path", str(tmp_path / "o"),
                                                                   "--gpus", "-1"])
    with pytest.raises(RuntimeError, match="--gpus -1"):
        P.main(args)
