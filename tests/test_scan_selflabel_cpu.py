"""The host side of the graph evaluation and of the self-labelling step: the float64 restatement of
tests/selflabel_ref.py against the reference's own values, the conditions its cases are built to, the workspace functions (no device
needed), the refusals of scan_main and the numbering of the self-label draws."""
import argparse
import os

import numpy as np
import pytest

import selflabel_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "scan", "selflabel_small.npz")
SCORED = [n for n in sorted(R.SELFLABEL_CASES) if n != R.NONE_CASE]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", SCORED)
def test_selflabel_restatement_equals_the_reference_in_float64(golden, name):
    """1e-12 relative: the loss against its own size, the gradient against the largest gradient of its case; target, mask, count
    exactly."""
    weak, strong, threshold, balance, up = R.selflabel_inputs(name)
    r = R.selflabel(weak, strong, threshold, balance, upstream=up)
    want = float(golden["sl_%s_loss_f64" % name])
    assert abs(r["loss"] - want) <= 1e-12 * abs(want)
    want = golden["sl_%s_grad_f64" % name]
    assert r["grad"].shape == want.shape == weak.shape
    assert np.abs(r["grad"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(r["target"], golden["sl_%s_target" % name]) and np.array_equal(r["mask"], golden["sl_%s_mask" % name])
    assert np.array_equal(r["count"], golden["sl_%s_count" % name])
    assert r["info"].tolist() == [int(r["mask"].sum()), int((r["count"] > 0).sum()), len(weak)]


@pytest.mark.parametrize("name", sorted(R.GRAPH_CASES))
def test_graph_restatement_equals_the_reference_in_float64(golden, name):
    logits, index, nheads, with_self = R.graph_inputs(name)
    stats, best = R.graph_eval(logits, index, nheads, with_self)
    want = golden["gr_%s_stats_f64" % name]
    assert stats.shape == want.shape == (nheads, 3)
    assert (np.abs(stats - want) <= 1e-12 * (1.0 + np.abs(want))).all()        # (a total near zero is a difference of two figures)
    assert best == int(golden["gr_%s_best" % name])


def test_selflabel_cases_meet_their_conditions():
    shapes = {R.SELFLABEL_CASES[n][:2] for n in R.SELFLABEL_CASES}
    assert {b for b, _ in shapes} >= {1, 2, 255, 256, 257, 515} and {c for _, c in shapes} >= {1, 2, 3, 33, 64}
    assert sorted(R.SELFLABEL_CASES)[-1] == R.NONE_CASE
    for name in R.SELFLABEL_CASES:
        weak, strong, threshold, balance, up = R.selflabel_inputs(name)
        r = R.selflabel(weak, strong, threshold, balance)
        assert 0.0 <= threshold < 1.0
        assert (np.abs(r["pmax"] - threshold) > R.MARGIN).all(), name          # no row near the threshold
        top = np.sort(weak, axis=1)[:, ::-1]
        assert weak.shape[1] == 1 or (top[:, 0] > top[:, 1]).all(), name       # no row with two equal maxima
        assert (r["info"][0] == 0) == (name == R.NONE_CASE), name
        assert np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all()
    assert R.selflabel(*R.selflabel_inputs("every_row")[:4])["info"][0] == R.SELFLABEL_CASES["every_row"][0]
    assert R.selflabel(*R.selflabel_inputs("one_row")[:4])["info"][0] == 1
    r = R.selflabel(*R.selflabel_inputs("absent_class")[:4])
    assert r["count"][0] == 0 and r["weight"][0] == 1.0 and (r["count"][1:] > 0).all() and (r["weight"][1:] != 1.0).all()
    assert R.selflabel(*R.selflabel_inputs("x30_wrong")[:4])["loss"] > 50
    assert R.selflabel(*R.selflabel_inputs("pm200")[:4])["loss"] > 100
    assert R.SELFLABEL_CASES["upstream"][5] == -2.5
    none = R.selflabel(*R.selflabel_inputs(R.NONE_CASE)[:4])
    assert none["loss"] == 0.0 and not none["grad"].any() and none["info"][0] == 0
    unbalanced = R.selflabel(*R.selflabel_inputs("b515_c3_unbalanced")[:4])
    assert (unbalanced["weight"] == 1.0).all() and unbalanced["denom"] == unbalanced["info"][0]


def test_graph_cases_meet_their_conditions(golden):
    cases = R.GRAPH_CASES.values()
    assert {c[0] for c in cases} >= {2, 255, 257, 515} and {c[1] for c in cases} >= {1, 5, 20}
    assert {c[2] for c in cases} >= {1, 3, 16} and {c[3] for c in cases} >= {1, 2, 33, 64}
    assert {c[5] for c in cases} == {True, False}
    dev = max([R.norm_value(golden["gr_%s_stats_f32" % n], golden["gr_%s_stats_f64" % n]) for n in R.GRAPH_CASES]
              + [R.norm_value(golden["sl_%s_loss_f32" % n], golden["sl_%s_loss_f64" % n]) for n in SCORED])
    for name in R.GRAPH_CASES:
        logits, index, nheads, with_self = R.graph_inputs(name)
        n = len(logits)
        assert index.min() >= 0 and index.max() < n and (index != np.arange(n)[:, None]).all()
        stats, _ = R.graph_eval(logits, index, nheads, with_self)
        assert R.best_gap(stats) > 100 * 4 * dev * (1 + np.abs(stats[:, 0]).max()), name      # `best` can be asserted on every case
    logits, index, nheads, _ = R.graph_inputs("dead_class")
    assert (R.softmax(logits.astype(np.float64).reshape(len(logits), nheads, -1)).mean(0)[0] < 1e-8).any()
    stats, _ = R.graph_eval(*R.graph_inputs("close_heads"))
    assert 1e-3 < R.best_gap(stats) / np.abs(stats[:, 0]).max() < 1e-1         # the totals part in the second or third digit
    # the pick itself in front of its row is one more pair per pick
    logits, index, nheads, _ = R.graph_inputs("n515_k5_h3_c33")
    assert not np.allclose(R.graph_eval(logits, index, nheads, True)[0][:, 1], R.graph_eval(logits, index, nheads, False)[0][:, 1])


def test_workspace_functions_need_no_device():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib as L
    lib = L.lib()
    for n, c, h in ((0, 3, 1), (4, 0, 1), (4, 65, 1), (4, 3, 0), (4, 3, 17), (2 ** 31, 3, 1)):
        assert lib.mi_scan_graph_eval_workspace_bytes(n, c, h) == 0
    assert lib.mi_scan_graph_eval_workspace_bytes(2 ** 31 - 1, 64, 16) > 8 * (2 ** 31 - 1) * 64 * 16
    assert lib.mi_scan_graph_eval_workspace_bytes(257, 3, 2) >= 8 * (257 * 6 + 2 * 2 * 64 + 2 * 2)
    for b, c in ((0, 3), (65537, 3), (4, 0), (4, 65)):
        assert lib.mi_scan_selflabel_workspace_bytes(b, c) == 0
    assert lib.mi_scan_selflabel_workspace_bytes(65536, 64) >= 8 * 2 * 256
    assert lib.mi_scan_selflabel_workspace_bytes(1, 1) >= 16


def _args(tmp_path, **over):
    from cet_pick_amd import scan_main
    argv = ["--input", str(tmp_path / "all_output_info.npz"), "--path", str(tmp_path / "out"), "--nclusters", "3"]
    args = scan_main.add_arguments(argparse.ArgumentParser()).parse_args(argv)
    for k, v in over.items():
        setattr(args, k, v)
    return args


def test_scan_main_refuses_a_threshold_outside_its_range(tmp_path):
    from cet_pick_amd import scan_main
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "all_output_info.npz", pred=rng.standard_normal((12, 4)).astype(np.float32),
             name=np.array(["tomo_%d" % (i % 2) for i in range(12)]), coords=rng.integers(0, 50, size=(12, 3)))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"--selflabel_threshold must be in \[0, 1\)"):
            scan_main.main(_args(tmp_path, selflabel_epochs=2, selflabel_threshold=bad))
    with pytest.raises(ValueError, match=r"--selflabel_epochs must be >= 0"):
        scan_main.main(_args(tmp_path, selflabel_epochs=-1))
    assert not (tmp_path / "out").exists()                 # refused before anything is written
    d = _args(tmp_path)
    assert (d.select_head, d.selflabel_epochs, d.selflabel_threshold, d.selflabel_lr, d.no_class_balancing) == ("epoch", 0, 0.99, 1e-4, False)
    with pytest.raises(SystemExit):
        scan_main.add_arguments(argparse.ArgumentParser()).parse_args(["--input", "a", "--path", "b", "--nclusters", "3",
                                                                      "--select_head", "loss"])


def test_selflabel_draws_continue_the_epoch_numbering():
    from cet_pick_amd.utils.scan import draw_neighbours, selflabel_draws
    rng = np.random.default_rng(3)
    n, k, bs = 53, 4, 10
    index = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in range(n)]).astype(np.int32)
    draws = list(selflabel_draws(index, 317, 30, 3, bs))
    assert [e for e, _, _ in draws] == [30, 31, 32]
    for epoch, anchor, strong in draws:
        want = draw_neighbours(index, 317, epoch, bs)
        assert np.array_equal(anchor, want[0]) and np.array_equal(strong, want[1])
    clustering = [draw_neighbours(index, 317, e, bs)[0] for e in range(30)]
    assert not any(np.array_equal(draws[0][1], a) for a in clustering)        # no clustering epoch's pairs again
    assert list(selflabel_draws(index, 317, 30, 0, bs)) == []


def test_host_tensors_are_refused():
    """no CPU fallback: logits on the host raise, with or without a GPU in the machine"""
    import torch
    from cet_pick_amd import _lib, hipops as H
    from cet_pick_amd.models.loss import ConfidenceBasedCE
    z = torch.zeros(4, 3)
    with pytest.raises(_lib.HipExtensionError):
        ConfidenceBasedCE(0.5, True)(z, z)
    with pytest.raises(_lib.HipExtensionError):
        H.scan_graph_eval(z, torch.zeros(4, 2, dtype=torch.int32), 1)
