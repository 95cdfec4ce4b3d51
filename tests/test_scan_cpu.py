"""The host side of the SCAN step: the float64 restatement of tests/scan_ref.py against the reference's own
values, the neighbour draws, the refusals of scan_main, the checkpoint layout and the class table's compatibility."""
import argparse
import os

import numpy as np
import pytest

import scan_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scan", "scan_small.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_the_reference_in_float64(golden, name):
    """1e-12 relative: every figure against its own size, a gradient against the largest gradient of its case (single
    elements of a softmax gradient are differences of near-equal numbers)."""
    a, b, nheads, up = R.case_inputs(name)
    stats, total = R.loss(a, b, nheads)
    want = golden[name + "_stats_f64"]
    assert stats.shape == want.shape == (nheads, 3)
    assert (np.abs(stats - want) <= 1e-12 * np.abs(want)).all()
    assert abs(total - float(golden[name + "_total_f64"])) <= 1e-12 * abs(float(golden[name + "_total_f64"]))
    da, db = R.grads(a, b, nheads, upstream=up)
    top = max(np.abs(golden[name + "_da_f64"]).max(), np.abs(golden[name + "_db_f64"]).max())
    assert np.abs(da - golden[name + "_da_f64"]).max() <= 1e-12 * top
    assert np.abs(db - golden[name + "_db_f64"]).max() <= 1e-12 * top


def test_cases_reach_the_clamp_the_floor_and_a_dead_class():
    a, b, nheads, _ = R.case_inputs("extreme")
    B = len(a)
    p, q = R.softmax(a.astype(np.float64).reshape(B, nheads, -1)), R.softmax(b.astype(np.float64).reshape(B, nheads, -1))
    s = (p * q).sum(-1)
    assert (s == 1.0).any() and (np.log(s) < -100).any() and ((s > 1e-30) & (s < 1e-12)).any()
    s32 = (R.softmax(a.reshape(B, nheads, -1)) * R.softmax(b.reshape(B, nheads, -1))).sum(-1)
    assert (s32 == 0).any()                                # float32 underflows where float64 does not
    a, _, nheads, _ = R.case_inputs("dead_class")
    assert (R.softmax(a.astype(np.float64).reshape(len(a), nheads, -1)).mean(0) < 1e-8).any()
    assert R.CASES["upstream"][4] != 1.0


def test_the_limits_are_stated_once():
    """MI_SCAN_CHUNK of the C header is the chunk of hipops and of the restatements, and the workspace functions (no device needed)
    answer 0 exactly outside hipops' limits: at a limit they count bytes, one past it and at 0 they refuse."""
    import re
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib as L, hipops as H
    import selflabel_ref
    header = open(os.path.join(os.path.dirname(HERE), "include", "cetpick_hip.h")).read()
    chunk = int(re.search(r"^#define MI_SCAN_CHUNK (\d+)$", header, re.M).group(1))
    assert H.SCAN_CHUNK == chunk and R.CHUNK == chunk and selflabel_ref.CHUNK is R.CHUNK
    lib = L.lib()
    C, NH, B = H.SCAN_MAX_CLASSES, H.SCAN_MAX_HEADS, H.SCAN_MAX_ROWS
    assert lib.mi_scan_loss_workspace_bytes(B, C, NH) > 0 and lib.mi_scan_loss_workspace_bytes(1, 1, 1) > 0
    assert lib.mi_scan_graph_eval_workspace_bytes(B + 1, C, NH) > 0 and lib.mi_scan_graph_eval_workspace_bytes(1, 1, 1) > 0
    assert lib.mi_scan_selflabel_workspace_bytes(B, C) > 0 and lib.mi_scan_selflabel_workspace_bytes(1, 1) > 0
    for b, c, h in ((B + 1, C, NH), (B, C + 1, NH), (B, C, NH + 1), (0, C, NH), (B, 0, NH), (B, C, 0)):
        assert lib.mi_scan_loss_workspace_bytes(b, c, h) == 0, (b, c, h)
        if b <= B:                                         # (the graph's rows are the picks: no batch limit)
            assert lib.mi_scan_graph_eval_workspace_bytes(b, c, h) == 0, (b, c, h)
        if h == NH:
            assert lib.mi_scan_selflabel_workspace_bytes(b, c) == 0, (b, c)


def test_neighbour_draws():
    from cet_pick_amd.utils.scan import draw_neighbours
    rng = np.random.default_rng(3)
    n, k, bs = 103, 5, 10
    index = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in range(n)]).astype(np.int32)
    anchor, neighbour = draw_neighbours(index, 317, 0, bs)
    R.check_draw(index, anchor, neighbour, bs)
    assert len(anchor) == 100 and anchor.dtype == neighbour.dtype == np.int64
    again = draw_neighbours(index, 317, 0, bs)
    assert np.array_equal(anchor, again[0]) and np.array_equal(neighbour, again[1])
    other = draw_neighbours(index, 317, 1, bs)
    R.check_draw(index, other[0], other[1], bs)
    assert not np.array_equal(anchor, other[0]) and not np.array_equal(neighbour, other[1])
    assert not np.array_equal(anchor, draw_neighbours(index, 318, 0, bs)[0])
    # over many epochs the pick itself and every neighbour column are drawn
    seen = set()
    table = np.concatenate([np.arange(n)[:, None], index], axis=1)
    for epoch in range(20):
        a, b = draw_neighbours(index, 317, epoch, bs)
        seen.update(np.argmax(table[a] == b[:, None], axis=1).tolist())
    assert seen == set(range(k + 1))
    with pytest.raises(ValueError, match="batch_size"):
        draw_neighbours(index, 317, 0, n + 1)


def _args(tmp_path, **over):
    from cet_pick_amd import scan_main
    argv = ["--input", str(tmp_path / "all_output_info.npz"), "--path", str(tmp_path / "out"), "--nclusters", "3"]
    args = scan_main.add_arguments(argparse.ArgumentParser()).parse_args(argv)
    for k, v in over.items():
        setattr(args, k, v)
    return args


def _write_input(tmp_path, n=12, d=4):
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "all_output_info.npz", pred=rng.standard_normal((n, d)).astype(np.float32),
             name=np.array(["tomo_%d" % (i % 2) for i in range(n)]), coords=rng.integers(0, 50, size=(n, 3)))


def test_scan_main_refusals(tmp_path):
    from cet_pick_amd import scan_main
    _write_input(tmp_path)
    with pytest.raises(RuntimeError, match=r"no CPU mode \(--gpus -1\)"):
        scan_main.main(_args(tmp_path, gpus="-1"))
    for bad in (0, 65):
        with pytest.raises(ValueError, match=r"--nclusters must be in 1\.\.64, got %d" % bad):
            scan_main.main(_args(tmp_path, nclusters=bad))
    for bad in (0, 17):
        with pytest.raises(ValueError, match=r"--nheads must be in 1\.\.16, got %d" % bad):
            scan_main.main(_args(tmp_path, nheads=bad))
    np.savez(tmp_path / "knn_graph.npz", index=np.zeros((11, 3), np.int32), dist=np.zeros((11, 3), np.float32), k=np.int32(3))
    with pytest.raises(ValueError, match=r"index of shape \(11, 3\), the input has 12 picks"):
        scan_main.main(_args(tmp_path, graph=str(tmp_path / "knn_graph.npz")))
    assert not (tmp_path / "out").exists()                 # refused before anything is written
    defaults = _args(tmp_path)
    assert (defaults.nheads, defaults.num_neighbor, defaults.num_epochs, defaults.batch_size, defaults.lr, defaults.weight_decay,
            defaults.entropy_weight, defaults.seed, defaults.min_conf) == (1, 20, 100, 1024, 1e-3, 1e-4, 2.0, 317, 0.0)


def test_checkpoint_layout(tmp_path):
    """scan_heads.pth, on a hand-made state: the reference's save_model_scan keys and its ClusteringModel names"""
    import torch
    from cet_pick_amd.utils import scan as S
    nheads, c, d = 3, 4, 7
    assert S.state_keys(nheads) == ["cluster_head.0.weight", "cluster_head.0.bias", "cluster_head.1.weight", "cluster_head.1.bias",
                                    "cluster_head.2.weight", "cluster_head.2.bias"]
    w, b = S.initial_heads(d, c, nheads, 317)
    assert tuple(w.shape) == (nheads * c, d) and tuple(b.shape) == (nheads * c,) and float(w.abs().max()) <= d ** -0.5
    assert torch.equal(w, S.initial_heads(d, c, nheads, 317)[0]) and not torch.equal(w, S.initial_heads(d, c, nheads, 318)[0])
    sd = {}
    for h in range(nheads):
        sd["cluster_head.%d.weight" % h], sd["cluster_head.%d.bias" % h] = w[h * c:(h + 1) * c].clone(), b[h * c:(h + 1) * c].clone()
    torch.save(S.checkpoint(sd, 7, None, -1.25, 2), tmp_path / "scan_heads.pth")
    ck = torch.load(tmp_path / "scan_heads.pth", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "best_loss_head", "epoch", "optimizer", "state_dict"]
    assert (ck["epoch"], ck["best_loss"], ck["best_loss_head"]) == (7, -1.25, 2)
    assert list(ck["state_dict"]) == S.state_keys(nheads)
    assert tuple(ck["state_dict"]["cluster_head.1.weight"].shape) == (c, d)
    assert tuple(ck["state_dict"]["cluster_head.1.bias"].shape) == (c,)


def test_host_tensors_are_refused():
    """no CPU fallback: logits on the host raise, with or without a GPU in the machine"""
    import torch
    from cet_pick_amd import _lib, hipops as H
    from cet_pick_amd.models.loss import SCANLoss
    z = torch.zeros(4, 3)
    with pytest.raises(_lib.HipExtensionError):
        SCANLoss()(z, z)
    with pytest.raises(_lib.HipExtensionError):
        H.scan_assign(z, 1)


def test_labels_file_feeds_interactive_to_training_coords(tmp_path):
    from cet_pick_amd import scan_main, interactive_to_training_coords as I
    n, c, nheads = 6, 3, 2
    names = np.array(["a", "a", "b", "b", "b", "c"])
    coords = np.arange(18).reshape(n, 3)
    label = np.array([[0, 1], [2, 1], [1, 0], [2, 2], [0, 0], [1, 2]], np.int32)
    conf = np.array([[.9, .9], [.8, .4], [.7, .9], [.6, .9], [.5, .9], [.4, .2]], np.float32)
    counts = np.array([[2, 2, 2], [2, 2, 2]], np.int32)
    out = scan_main.labels_file(names, coords, label, conf, 1, counts, np.zeros((nheads, 3)), np.full((n, c), 1 / 3), 0.5)
    assert sorted(out) == ["conf", "coords", "counts", "head", "label", "name", "prob", "stats"]
    assert out["label"].tolist() == [1, -1, 0, 2, 0, -1] and out["label"].dtype == np.int32 and int(out["head"]) == 1
    np.savez(tmp_path / "scan_labels.npz", **out)
    args = I.add_arguments(argparse.ArgumentParser()).parse_args(
        ["--input", str(tmp_path / "scan_labels.npz"), "--output", str(tmp_path / "coords.txt"), "--labels", "0,2"])
    assert I.main(args) == 3
    rows = [line.split("\t") for line in open(tmp_path / "coords.txt").read().splitlines()]
    assert rows == [list(I.HEADER), ["b", "6", "7", "8"], ["b", "9", "10", "11"], ["b", "12", "13", "14"]]
    args.labels = None                                     # every pick, the unlabelled ones too
    assert I.main(args) == n
