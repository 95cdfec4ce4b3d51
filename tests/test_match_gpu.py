"""mi_match_coordinates (csrc/match.hip) through hipops against scipy's optimum (tests/match_ref.py): identical assignment,
distances and cost on rigid inputs, the optimal cost and a valid matching on inputs whose optimum is not unique."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_ref as M

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(0, 5), (5, 0), (1, 1), (1, 9), (7, 3), (3, 7), (63, 65), (64, 64), (65, 63), (300, 257), (1025, 40)]


def run(images, radius):
    """images: [(preds, targets)] -> [(pred_to_target, dist, total)] from ONE launch"""
    from cet_pick_amd import hipops
    po = np.concatenate([[0], np.cumsum([len(p) for p, _ in images])])
    to = np.concatenate([[0], np.cumsum([len(t) for _, t in images])])
    dev = lambda rows: torch.as_tensor(np.concatenate(rows, 0).reshape(-1, 3)).cuda()      # noqa: E731
    p2t, dist, total = hipops.match_coordinates(dev([p for p, _ in images]), dev([t for _, t in images]), po, to, radius)
    p2t, dist, total = p2t.cpu().numpy(), dist.cpu().numpy(), total.cpu().numpy()
    return [(p2t[po[i]:po[i + 1]], dist[po[i]:po[i + 1]], float(total[i])) for i in range(len(images))]


def rigid(P, T):
    preds, targets = M.rigid_case(P, T, seed=P * 1000 + T)
    assert M.is_rigid(preds, targets, M.RIGID_RADIUS)
    return preds, targets


@pytest.mark.parametrize("P,T", SIZES)
def test_rigid_inputs_match_scipy_exactly(P, T):
    preds, targets = rigid(P, T)
    (p2t, dist, total), = run([(preds, targets)], M.RIGID_RADIUS)
    want = M.solve_scipy(preds, targets, M.RIGID_RADIUS)
    assert total == want[2]
    assert np.array_equal(p2t, want[0])
    assert np.array_equal(dist, want[1])


@pytest.mark.parametrize("P,T,box,radius", [(256, 256, (40, 40, 40), 10), (2000, 1500, (512, 512, 128), 5)])
def test_optimal_cost_and_validity_where_the_optimum_is_not_unique(P, T, box, radius):
    rng = np.random.default_rng(P)
    preds, targets = (rng.integers(0, box, (n, 3)).astype(np.float64) for n in (P, T))
    (p2t, dist, total), = run([(preds, targets)], radius)
    want = M.solve_scipy(preds, targets, radius)[2]
    assert want < 0
    assert total == want                                               # integer costs: exact in double
    assert M.check_valid(preds, targets, radius, p2t, dist) == want


def test_batch_equals_single_launches():
    images = [rigid(P, T) for P, T in [(300, 257), (0, 5), (65, 63), (1025, 40), (0, 0), (7, 3)]]
    images[2] = M.crowded(65, 63, 14, seed=3)                            # one whose optimum is not unique
    batch = run(images, M.RIGID_RADIUS)
    for img, got in zip(images, batch):
        (one,) = run([img], M.RIGID_RADIUS)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1]) and got[2] == one[2]
        assert got[2] == M.solve_scipy(img[0], img[1], M.RIGID_RADIUS)[2]


def test_non_integer_coordinates():
    """The returned pairs' cost, re-summed in numpy, within 1e-9 * sum|cost| of scipy's (loose over the <= 4096 * 2^-52
    rounding of the sums)."""
    rng = np.random.default_rng(11)
    preds, targets = rng.random((500, 3)) * 60, rng.random((430, 3)) * 60
    (p2t, dist, total), = run([(preds, targets)], 2.5)
    want = M.solve_scipy(preds, targets, 2.5)[2]
    got = M.check_valid(preds, targets, 2.5, p2t, dist)
    print("non-integer coordinates: |re-summed - scipy| / sum|cost| = %.3e, kernel's own total off by %.3e"
          % (abs(got - want) / abs(want), abs(total - want) / abs(want)))
    assert want < 0 and abs(got - want) <= 1e-9 * abs(want)
    assert abs(total - want) <= 1e-9 * abs(want)


def test_over_the_limit_raises_and_launches_nothing():
    from cet_pick_amd import _lib, hipops
    preds, targets = torch.zeros(4097, 3, dtype=torch.float64, device="cuda"), torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.HipExtensionError):
        hipops.match_coordinates(preds, targets, [0, 4097], [0, 2], 3)
    with pytest.raises(_lib.HipExtensionError):
        hipops.match_coordinates(targets, preds, [0, 2], [0, 4097], 3)
    # the C entry itself, with a workspace that is large enough: refused on the host, the outputs stay as they were
    p2t = torch.full((4099,), 7, dtype=torch.int32, device="cuda")
    dist, total = torch.full((4099,), 7.0, dtype=torch.float64, device="cuda"), torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    po, to = np.array([0, 2, 4099], np.int32), np.array([0, 1, 2], np.int32)
    rc = _lib.lib().mi_match_coordinates(_lib.ptr(torch.zeros(4099, 3, dtype=torch.float64, device="cuda")), _lib.ptr(targets),
                                         po.ctypes.data, to.ctypes.data, 2, 3.0, _lib.ptr(p2t), _lib.ptr(dist), _lib.ptr(total),
                                         _lib.ptr(ws), ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert bool((p2t == 7).all()) and bool((dist == 7).all()) and bool((total == 7).all())


def test_evaluation_interface():
    from cet_pick_amd.evaluation import match_coordinates
    preds, targets = rigid(63, 65)
    assignment, dist = match_coordinates(targets, preds, M.RIGID_RADIUS)
    want = M.solve_scipy(preds, targets, M.RIGID_RADIUS)
    assert assignment.dtype == np.float32 and dist.dtype == np.float64
    assert np.array_equal(assignment, (want[0] >= 0).astype(np.float32)) and np.array_equal(dist, want[1])


def _scripts(work, targets_file, images, module_runner):
    args = ["--predicted", os.path.join(work, "all_coords.txt"), "--targets", targets_file, "--path", work, "-r",
            str(M.RIGID_RADIUS), "--images", images, "--out", "pr.txt", "--stats", "stats.txt", "--folder", "run", "--w",
            os.path.join(work, "overall.txt")]
    return module_runner(["--path", work, "--out", "all_coords.txt"], args)


def _as_modules(merge_args, pr_args):
    env = dict(os.environ, PYTHONPATH=REPO)
    for mod, a in (("cet_pick_amd.merge_output", merge_args), ("cet_pick_amd.precision_recall_curve", pr_args)):
        out = subprocess.run([sys.executable, "-m", mod] + a, cwd=REPO, env=env, check=True, capture_output=True, text=True,
                             timeout=300).stdout
    return out


def _in_process(merge_args, pr_args, match_batch=None):
    import argparse
    import contextlib
    import io
    from cet_pick_amd import merge_output, precision_recall_curve as S
    merge_output.main(merge_output.add_arguments(argparse.ArgumentParser()).parse_args(merge_args))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        S.main(S.add_arguments(argparse.ArgumentParser()).parse_args(pr_args), match_batch=match_batch)
    return buf.getvalue()


def _in_process_arbiter(merge_args, pr_args):
    return _in_process(merge_args, pr_args, M.match_batch_scipy)


def _read(work):
    return [open(os.path.join(work, f)).read() for f in ("pr.txt", "stats.txt", "overall.txt")]


def test_scripts_end_to_end_on_a_rigid_split(tmp_path):
    rng = np.random.default_rng(5)
    works = [str(tmp_path / "gpu"), str(tmp_path / "host")]
    targets_file = str(tmp_path / "targets.txt")
    for w in works:
        os.makedirs(w)
    with open(targets_file, "w") as tf:
        tf.write("image_name\tx_coord\ty_coord\tz_coord\n")
        for name, (P, T) in (("t0", (120, 90)), ("t1", (40, 77)), ("t2", (300, 31))):
            preds, targets = rigid(P, T)
            tf.writelines("%s\t%d\t%d\t%d\n" % (name, x, y, z) for x, y, z in targets.astype(int))
            rows = ["%d\t%d\t%d\t%.2f\n" % (x, z, y, s) for (x, y, z), s in zip(preds.astype(int), rng.integers(1, 30, P) / 100.0)]
            for w in works:
                open(os.path.join(w, name + ".txt"), "w").writelines(rows)
    out_gpu = _scripts(works[0], targets_file, "target", _as_modules)
    out_host = _scripts(works[1], targets_file, "target", _in_process_arbiter)
    assert _read(works[0]) == _read(works[1])                          # every numeric column to the last printed digit
    assert out_gpu.strip().splitlines()[-1] == out_host.strip().splitlines()[-1] and out_gpu.startswith("# auprc=")


@pytest.mark.parametrize("images", ["target", "union"])
def test_scripts_on_the_references_golden_split(tmp_path, images):
    import shutil
    eval_dir = os.path.join(REPO, "tests", "golden", "eval")
    work = str(tmp_path / "out")
    shutil.copytree(os.path.join(eval_dir, "inputs", "picks"), work)
    _scripts(work, os.path.join(eval_dir, "inputs", "targets.txt"), images, _in_process)       # the device's matcher
    exp = lambda name: open(os.path.join(eval_dir, "expected", name)).read()      # noqa: E731
    pr, stats, overall = _read(work)
    assert pr == exp("pr_%s.txt" % images) and stats == exp("stats_%s.txt" % images)
    assert overall.replace("run\t", "run_%s\t" % images) in exp("overall.txt")
