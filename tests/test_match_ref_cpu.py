"""The host side of the pick scoring (no GPU): the arbiter of tests/test_match_gpu.py against scipy, the rigidity of its
generated inputs, and precision_recall_curve and both scripts' files against the reference's own output on the golden split
(tests/golden/eval, written by gen_golden_eval.py)."""
import argparse
import os
import shutil

import numpy as np
import pytest

import match_ref as M

EVAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval")
SIZES = [(0, 5), (5, 0), (1, 1), (1, 9), (7, 3), (3, 7), (63, 65), (64, 64), (65, 63), (300, 257)]


@pytest.mark.parametrize("P,T", SIZES)
def test_rigid_generator_is_rigid_and_restatement_equals_scipy(P, T):
    preds, targets = M.rigid_case(P, T, seed=P * 1000 + T)
    assert preds.shape == (P, 3) and targets.shape == (T, 3)
    assert M.is_rigid(preds, targets, M.RIGID_RADIUS)
    want, got = M.solve_scipy(preds, targets, M.RIGID_RADIUS), M.solve_f64(preds, targets, M.RIGID_RADIUS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert M.check_valid(preds, targets, M.RIGID_RADIUS, *got[:2]) == want[2]
    if min(P, T) > 2:
        assert (want[0] >= 0).sum() > 0 and want[2] < 0


def test_is_rigid_sees_a_tie():
    preds, targets = np.array([[0, 0, 0], [4, 0, 0]], float), np.array([[2, 0, 0]], float)     # both picks at distance 2
    assert not M.is_rigid(preds, targets, 3)
    assert M.is_rigid(preds + [[0, 0, 0], [1, 0, 0]], targets, 3)


@pytest.mark.parametrize("P,T,box,radius", [(40, 40, 12, 5), (33, 47, 14, 4), (47, 33, 14, 4), (60, 60, 40, 10)])
def test_restatement_reaches_scipys_optimum_on_crowded_inputs(P, T, box, radius):
    preds, targets = M.crowded(P, T, box, seed=P + T)
    p2t, dist, total = M.solve_f64(preds, targets, radius)
    assert total == M.solve_scipy(preds, targets, radius)[2]          # integer costs: exact
    assert M.check_valid(preds, targets, radius, p2t, dist) == total


def test_precision_recall_curve_buckets_and_nan():
    from cet_pick_amd.evaluation.metrics import precision_recall_curve
    hit = np.array([1, 0, 1, 1, 0, 0], np.float32)
    score = np.array([.9, .9, .5, .7, .5, .1], np.float32)
    pr, re, th, avpr = precision_recall_curve(hit, score, N=4)
    assert np.array_equal(th, np.array([.9, .7, .5, .1], np.float32))
    assert np.array_equal(pr, [1 / 2, 2 / 3, 3 / 5, 3 / 6]) and np.array_equal(re, [1 / 4, 2 / 4, 3 / 4, 3 / 4])
    assert avpr == (1 / 2 + 2 / 3 + 3 / 5) / 4
    assert precision_recall_curve(hit, score)[3] == (1 / 2 + 2 / 3 + 3 / 5) / 3


def _blocks(path):
    """header, {image: its lines in order} of a merged table"""
    lines = open(path).read().splitlines()
    out = {}
    for ln in lines[1:]:
        out.setdefault(ln.split("\t")[0], []).append(ln)
    return lines[0], out


def _merge(tmp_path):
    from cet_pick_amd import merge_output
    work = str(tmp_path / "out")
    shutil.copytree(os.path.join(EVAL, "inputs", "picks"), work)
    return work, merge_output.main(argparse.Namespace(path=work, out="all_coords.txt"))


def test_merge_output_equals_the_references_file(tmp_path):
    work, merged = _merge(tmp_path)
    header, blocks = _blocks(merged)
    want_header, want = _blocks(os.path.join(EVAL, "expected", "all_coords.txt"))
    assert header == want_header == "image_name\tx_coord\tz_coord\ty_coord\tscore"
    assert blocks == want and list(blocks) == sorted(blocks)          # the reference's file order is the directory's
    n_in = sum(len(open(os.path.join(work, f)).read().splitlines()) for f in ("tomo_a.txt", "tomo_b.txt", "tomo_d.txt"))
    assert sum(map(len, blocks.values())) == n_in - 3                  # the first line of every file is dropped
    from cet_pick_amd import merge_output
    merge_output.main(argparse.Namespace(path=work, out="all_coords.txt"))     # the output file is not merged into itself
    assert _blocks(merged) == (header, blocks)


@pytest.mark.parametrize("images", ["target", "union"])
def test_precision_recall_files_equal_the_references(tmp_path, images, capsys):
    from cet_pick_amd import precision_recall_curve as S
    work, merged = _merge(tmp_path)
    args = S.add_arguments(argparse.ArgumentParser()).parse_args(
        ["--predicted", merged, "--targets", os.path.join(EVAL, "inputs", "targets.txt"), "--path", work, "-r",
         str(M.RIGID_RADIUS), "--images", images, "--out", "pr.txt", "--stats", "stats.txt", "--folder", "run_" + images, "--w",
         os.path.join(work, "overall.txt")])
    S.main(args, match_batch=M.match_batch_scipy)
    S.main(args, match_batch=M.match_batch_scipy)                      # --w is appended to
    exp = lambda name: open(os.path.join(EVAL, "expected", name)).read()      # noqa: E731
    assert open(os.path.join(work, "pr.txt")).read() == exp("pr_%s.txt" % images)
    assert open(os.path.join(work, "stats.txt")).read() == exp("stats_%s.txt" % images)
    line = [ln for ln in exp("overall.txt").splitlines() if ln.startswith("run_" + images + "\t")]
    assert open(os.path.join(work, "overall.txt")).read().splitlines() == line * 2
    # stdout: the auprc to the last digit.  The reference's mae is nan on this split (its running mean divides 0 by 0 when the
    # first image of its set has no match); ours takes the images in sorted order and tomo_a has matches
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("# auprc=")]
    assert len(out) == 2 and out[0].split(", mae=")[0] == exp("stdout_%s.txt" % images).split(", mae=")[0]
    assert np.isfinite(float(out[0].split(", mae=")[1]))


def test_golden_split_is_rigid():
    import pandas as pd
    t = pd.read_csv(os.path.join(EVAL, "inputs", "targets.txt"), sep="\t")
    for name in ("tomo_a", "tomo_b"):
        p = np.loadtxt(os.path.join(EVAL, "inputs", "picks", name + ".txt"))[1:, [0, 2, 1]]
        assert len(p) <= 40
        assert M.is_rigid(p, t.loc[t.image_name == name][["x_coord", "y_coord", "z_coord"]].values, M.RIGID_RADIUS)


def test_workspace_query_refuses_sizes_over_the_limit():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib, hipops
    size = _lib.lib().mi_match_workspace_bytes
    assert hipops.MATCH_MAX_POINTS == 4096
    assert size(1, 4096, 4096) > 0 and size(16, 900, 600) > 0 and size(3, 0, 0) > 0
    assert size(1, 4097, 10) == 0 and size(1, 10, 4097) == 0 and size(-1, 1, 1) == 0
