"""Golden files of the scoring scripts, by RUNNING the reference's own merge_output.py and precision_recall_curve.py on a
small made-up split.  Run with the reference checkout's root in CET_PICK_REFERENCE:
    CET_PICK_REFERENCE=/path/to/reference PYTHONDONTWRITEBYTECODE=1 python tests/golden/eval/gen_golden_eval.py

The split (inputs/): four images built from rigid components (tests/match_ref.py), at most 40 picks each, scores from ten
values so that many tie; `tomo_c` has targets and no picks, `tomo_d` picks and no targets.  The pick files are what test.py
writes (x<TAB>z<TAB>y<TAB>score, no header), so the reference's merge drops the first pick of each.
Outputs (expected/): all_coords.txt, and for --images target and union the curve, the stats file and the stdout line, plus the
overall file both runs appended to.  Only inputs and outputs are kept; nothing of the reference's text is.
"""
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import match_ref as M  # noqa: E402

SIZES = {"tomo_a": (38, 30), "tomo_b": (25, 33), "tomo_c": (0, 12), "tomo_d": (9, 0)}     # picks, targets
RADIUS = M.RIGID_RADIUS


def write_inputs(root):
    os.makedirs(os.path.join(root, "picks"), exist_ok=True)
    rng = np.random.default_rng(2024)
    with open(os.path.join(root, "targets.txt"), "w") as tf:
        tf.write("image_name\tx_coord\ty_coord\tz_coord\n")
        for k, (name, (P, T)) in enumerate(sorted(SIZES.items())):
            preds, targets = M.rigid_case(P, T, seed=100 + k)
            for x, y, z in targets.astype(int):
                tf.write("%s\t%d\t%d\t%d\n" % (name, x, y, z))
            if P:
                with open(os.path.join(root, "picks", name + ".txt"), "w") as pf:
                    for (x, y, z), s in zip(preds.astype(int), rng.integers(1, 11, P) / 10.0):
                        pf.write("%d\t%d\t%d\t%.1f\n" % (x, z, y, s))


def main():
    ref = os.environ["CET_PICK_REFERENCE"]
    inputs, expected = os.path.join(HERE, "inputs"), os.path.join(HERE, "expected")
    for d in (inputs, expected):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    write_inputs(inputs)
    work = os.path.join(HERE, "_work")
    shutil.rmtree(work, ignore_errors=True)
    shutil.copytree(os.path.join(inputs, "picks"), work)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    run = lambda script, *a: subprocess.run([sys.executable, os.path.join(ref, "cet_pick", script)] + list(a), env=env,  # noqa: E731
                                            check=True, capture_output=True, text=True).stdout
    run("merge_output.py", "--path", work, "--out", "all_coords.txt")
    shutil.copy(os.path.join(work, "all_coords.txt"), expected)
    for images in ("target", "union"):
        out = run("precision_recall_curve.py", "--predicted", os.path.join(work, "all_coords.txt"), "--targets",
                  os.path.join(inputs, "targets.txt"), "--path", work, "-r", str(RADIUS), "--images", images, "--out",
                  "pr_%s.txt" % images, "--stats", "stats_%s.txt" % images, "--folder", "run_" + images, "--w",
                  os.path.join(work, "overall.txt"))
        with open(os.path.join(expected, "stdout_%s.txt" % images), "w") as f:
            f.write("".join(line + "\n" for line in out.splitlines() if line.startswith("# auprc")))
        for name in ("pr_%s.txt" % images, "stats_%s.txt" % images):
            shutil.copy(os.path.join(work, name), expected)
    shutil.copy(os.path.join(work, "overall.txt"), expected)
    shutil.rmtree(work)


if __name__ == "__main__":
    main()
