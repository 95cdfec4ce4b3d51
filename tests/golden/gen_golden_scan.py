"""Golden values of the SCAN loss -> scan/scan_small.npz, by IMPORTING the reference's `SCANLoss` (models/loss.py:87-119) and
running it on the CPU, head by head, in float64 and in float32, with torch's autograd for the gradients.  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_scan.py
Importing gen_golden brings its package stubs (cv2, torchvision, skimage, mrcfile: packages the reference's loss.py reaches through
its imports and SCANLoss never touches) and the reference onto sys.path.  The fixture holds results only: per case of
tests/scan_ref.py::CASES the per-head (total, consistency, entropy), the sum of the totals, and the gradients of upstream x that
sum with respect to both logits tensors, each once in float64 (`*_f64`) and once in float32 (`*_f32`).  The logits are
tests/scan_ref.py::case_inputs(name)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (stubs + sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import scan_ref as R  # noqa: E402


def run(crit, a, b, nheads, up, dtype):
    a = torch.from_numpy(a).to(dtype).requires_grad_(True)
    b = torch.from_numpy(b).to(dtype).requires_grad_(True)
    c = a.shape[1] // nheads
    rows = [crit(a[:, h * c:(h + 1) * c], b[:, h * c:(h + 1) * c]) for h in range(nheads)]
    total = sum(r[0] for r in rows)                        # TomoSCANLoss: the heads' totals added in order
    (total * up).backward()
    stats = torch.stack([torch.stack(r) for r in rows]).detach().numpy()
    return stats, total.detach().numpy(), a.grad.numpy(), b.grad.numpy()


def gen():
    from cet_pick.models import loss as RL
    crit = RL.SCANLoss(entropy_weight=R.ENTROPY_WEIGHT)
    out = {}
    for name in sorted(R.CASES):
        a, b, nheads, up = R.case_inputs(name)
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            stats, total, da, db = run(crit, a, b, nheads, up, dtype)
            out.update({"%s_stats_%s" % (name, tag): stats, "%s_total_%s" % (name, tag): total,
                        "%s_da_%s" % (name, tag): da, "%s_db_%s" % (name, tag): db})
        print(name, out[name + "_total_f64"], out[name + "_total_f32"])
    os.makedirs(os.path.join(HERE, "scan"), exist_ok=True)
    G.save(os.path.join("scan", "scan_small.npz"), **out)


if __name__ == "__main__":
    gen()
