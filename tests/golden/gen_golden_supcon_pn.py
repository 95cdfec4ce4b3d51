"""Golden values of the --pn contrastive term -> supcon_pn_small.npz, by IMPORTING the reference's `SupConLossV2_more`
(models/loss.py:759-818) and running it on the CPU, in float64, at N = 48, dim 16.  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_supcon_pn.py
Importing gen_golden brings its package stubs and the reference onto sys.path.  The fixture holds, per case, both views' features,
the labels, thresh, T and the loss; the inputs are tests/supcon_pn_ref.py::case_inputs."""
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (stubs + sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import supcon_pn_ref as R  # noqa: E402

N, DIM = 48, 16
CASES = (("binary", 0.85, 0.07), ("mixed", 0.85, 0.07), ("mixed", 0.3, 0.5), ("binary", 0.3, 0.5))


def gen():
    from cet_pick.models import loss as RL
    out = {"cases": np.asarray(len(CASES))}
    for k, (kind, thresh, T) in enumerate(CASES):
        f, f_cr, lab = R.case_inputs(N, DIM, thresh, kind)
        opt = SimpleNamespace(thresh=thresh, device=torch.device("cpu"))
        loss = RL.SupConLossV2_more(T)(lab, None, None, f.double(), f_cr.double(), opt)
        out.update({"f_%d" % k: f.numpy(), "f_cr_%d" % k: f_cr.numpy(), "labels_%d" % k: lab.numpy(),
                    "thresh_%d" % k: np.asarray(thresh), "T_%d" % k: np.asarray(T), "loss_%d" % k: np.asarray(float(loss))})
        print(kind, thresh, T, float(loss))
    G.save("supcon_pn_small.npz", **out)


if __name__ == "__main__":
    gen()
