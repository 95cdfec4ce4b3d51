"""Label spreading without a GPU: the restatement of tests/label_spread_ref.py against its own closed form and
against scikit-learn's LabelSpreading, the seed table's parser, and the refusals of propagate_labels and utils/label_spread.py
that are raised before the device is touched."""
import argparse
import os

import numpy as np
import pytest

import label_spread_ref as R


def _graph(name, mode=1):
    v = R.make(name)
    w = R.weights(v["index"], v["dist"], mode)[0]
    row_ptr, col, wsym, deg, val = R.sym_csr(v["index"], w)
    return v, R.dense(row_ptr, col, val), R.dense(row_ptr, col, wsym)


@pytest.mark.parametrize("name", ("v300c3", "hub", "dup", "split"))
def test_iteration_reaches_the_closed_form(name):
    v, S, _ = _graph(name)
    assert np.array_equal(S, S.T)                          # symmetric to the bit
    assert np.abs(np.linalg.eigvalsh(S)).max() <= 1 + 1e-12
    Y = R.one_hot(len(S), v["seed_index"], v["seed_class"], v["C"])
    alpha = 0.9
    F, it, res = R.iterate(S, Y, alpha, 1e-13)
    star = R.closed_form(S, Y, alpha)
    bound = alpha / (1 - alpha) * np.sqrt(F.size) * res + 1e-11
    assert np.abs(F - star).max() <= bound
    assert (star >= -1e-15).all()
    if name == "split":                                    # no seed in blob 1: nothing arrives there
        assert (star[v["blob"] == 1] == 0).all() and (F[v["blob"] == 1] == 0).all()
        assert (R.decide(F, 0.5)[0][v["blob"] == 1] == -1).all()


@pytest.mark.parametrize("name", ("v300c3", "v257"))
def test_sklearn_label_spreading_agrees(name):
    """the same affinity matrix through a callable kernel: label_distributions_ is the row-normalised F"""
    pytest.importorskip("sklearn")
    from sklearn.semi_supervised import LabelSpreading
    v, S, W = _graph(name)
    n, alpha = len(S), 0.8
    y = np.full(n, -1)
    y[v["seed_index"]] = v["seed_class"]
    model = LabelSpreading(kernel=lambda a, b: W, alpha=alpha, max_iter=5000, tol=1e-13)
    model.fit(np.zeros((n, 1)), y)
    assert list(model.classes_) == list(range(v["C"]))
    F = R.iterate(S, R.one_hot(n, v["seed_index"], v["seed_class"], v["C"]), alpha, 1e-15)[0]
    mass = F.sum(1, keepdims=True)
    assert (mass > 0).all()
    assert np.abs(model.label_distributions_ - F / mass).max() <= 1e-9
    assert np.array_equal(model.transduction_, R.decide(F, 0.0)[0])


def test_undecided_share_of_the_decision_variants():
    """what test_label_spread_gpu.py relies on, from the restatement alone"""
    for name in R.DECISION_VARIANTS:
        v, S, _ = _graph(name)
        star = R.closed_form(S, R.one_hot(len(S), v["seed_index"], v["seed_class"], v["C"]), 0.9)
        top = np.sort(star, 1)
        margin = top[:, -1] - top[:, -2]
        assert (margin <= 2 * 0.9 / 0.1 * np.sqrt(star.size) * 1e-10 + 1e-11).mean() <= 0.01, name


def test_planted_graph_has_no_edge_across_blobs():
    x, blob, index, dist, seed_index, seed_class = R.planted()
    assert (blob[index] == blob[:, None]).all()


def _table(tmp_path, text, name="seeds.txt"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    return path


def test_seed_table_parser(tmp_path):
    from cet_pick_amd.propagate_labels import read_seeds, tomo_ids
    head = "image_name\tx_coord\ty_coord\tz_coord"
    names, xyz, cls = read_seeds(_table(tmp_path, head + "\tclass\ntomoA\t1\t2.5\t30\t0\ntomoB\t4\t5\t6\t3\n"))
    assert list(names) == ["tomoA", "tomoB"] and cls.tolist() == [0, 3] and xyz.dtype == np.float64
    assert xyz.tolist() == [[1, 2.5, 30], [4, 5, 6]]
    # no fifth column: class 0; no header; --if_double halves z
    names, xyz, cls = read_seeds(_table(tmp_path, "tomoA\t1\t2\t30\ntomoA\t7\t8\t9\n"), if_double=True)
    assert cls.tolist() == [0, 0] and xyz.tolist() == [[1, 2, 15], [7, 8, 4.5]]
    names, xyz, cls = read_seeds(_table(tmp_path, head + "\ntomoA\t1\t2\t3\n"))
    assert len(names) == 1 and cls.tolist() == [0]
    for bad in ("tomoA\t1\t2\n", "tomoA\t1\t2\t3\t-1\n", "tomoA\t1\t2\t3\t1\ntomoA\t1\t2\t3\n", "tomoA\tx\t2\t3\n", head + "\n"):
        with pytest.raises(ValueError):
            read_seeds(_table(tmp_path, bad))
    pick_id, seed_id = tomo_ids(np.array(["b", "a", "b", "c"]), np.array(["c", "zz", "a", "0"]))
    assert pick_id.tolist() == [1, 0, 1, 2] and seed_id.tolist() == [2, -1, 0, -1] and seed_id.dtype == np.int32


def _args(tmp_path, **kw):
    from cet_pick_amd.propagate_labels import add_arguments
    n = 12
    inp = os.path.join(str(tmp_path), "all_output_info.npz")
    np.savez(inp, pred=np.zeros((n, 4), np.float32), name=np.array(["t"] * n), coords=np.zeros((n, 3), np.float32))
    argv = ["--input", inp, "--path", os.path.join(str(tmp_path), "out")]
    for k, v in kw.items():
        argv += ["--" + k] + ([] if v is True else [str(v)])
    return add_arguments(argparse.ArgumentParser()).parse_args(argv)


def _seed_npz(tmp_path, index, cls):
    path = os.path.join(str(tmp_path), "seeds.npz")
    np.savez(path, **{"index": np.asarray(index), "class": np.asarray(cls)})
    return path


def test_cli_refusals_before_the_device(tmp_path):
    from cet_pick_amd import propagate_labels as P
    with pytest.raises(RuntimeError, match="no CPU mode"):
        P.main(_args(tmp_path, seed_index=_seed_npz(tmp_path, [0, 1], [0, 1]), gpus=-1))
    with pytest.raises(ValueError, match="counter-examples"):
        P.main(_args(tmp_path, seed_index=_seed_npz(tmp_path, [0, 1, 2], [1, 1, 1])))
    with pytest.raises(ValueError, match="class 0 and of class 1"):
        P.main(_args(tmp_path, seed_index=_seed_npz(tmp_path, [0, 3, 0], [0, 1, 1])))
    with pytest.raises(ValueError, match="one of the two"):
        P.main(_args(tmp_path))
    graph = os.path.join(str(tmp_path), "knn_graph.npz")
    np.savez(graph, index=(np.arange(12)[:, None] + np.arange(1, 4)[None, :]) % 12)
    with pytest.raises(ValueError, match="holds no dist"):
        P.main(_args(tmp_path, seed_index=_seed_npz(tmp_path, [0, 1], [0, 1]), graph=graph))
    assert P.load_graph(graph, 12, "binary")[1] is None


def test_no_cpu_path():
    import torch
    from cet_pick_amd import _lib as L
    from cet_pick_amd.utils import label_spread as LS
    v = R.make("k1")
    with pytest.raises(L.HipExtensionError):
        LS.spread_graph(v["index"], v["dist"])
    with pytest.raises(L.HipExtensionError):
        LS.spread_graph(torch.from_numpy(v["index"]), torch.from_numpy(v["dist"]), device="cpu")
    with pytest.raises(L.HipExtensionError):
        LS.decide(torch.zeros(4, 2, dtype=torch.float64), 0.5)
    with pytest.raises(L.HipExtensionError):
        LS.match_seeds(np.zeros((3, 3)), np.zeros(3, np.int32), np.zeros((1, 3)), np.zeros(1, np.int32), 8.0)
    # damaged graphs are refused on the host, whatever the device
    bad = v["index"].copy()
    bad[3, 0] = len(bad)
    with pytest.raises(ValueError, match="outside"):
        LS.spread_graph(bad, v["dist"], device="cuda")
    bad[3, 0] = -1
    with pytest.raises(ValueError, match="outside"):
        LS.spread_graph(bad, v["dist"], device="cuda")
    with pytest.raises(ValueError, match="do not fit int32"):
        LS.spread_graph(np.broadcast_to(np.zeros(1, np.int32), (2 ** 16, 2 ** 15)), None, "binary", device="cuda")
    with pytest.raises(ValueError, match="needs the graph's distances"):
        LS.spread_graph(v["index"], None, "gauss", device="cuda")
    with pytest.raises(ValueError, match="class 0 and of class 1"):
        LS.seed_matrix(10, [1, 2, 1], [0, 1, 1], 2)
    assert LS.seed_matrix(4, [1, 1, 2], [0, 0, 1], 2).tolist() == [[0, 0], [1, 0], [0, 1], [0, 0]]
