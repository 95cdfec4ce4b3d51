"""match_coordinates of the reference (evaluation/algorithms.py:6-21) on the device: csrc/match.hip through hipops.

The cost of a pair is min(d2 - radius ** 3, 0): the CUBE of the radius, as the reference has it, so `-r 10` accepts pairs
closer than sqrt(1000) = 31.6 voxels.  The optimal total cost is unique; the assignment is not where sums tie.
"""
import numpy as np
import torch

from .. import hipops


def match_coordinates_batch(targets, preds, radius, device="cuda"):
    """One launch for many images: targets and preds are equally long lists of (n, 3) arrays, one pair per image.
    Returns a list of (assignment float32 (P,), dist float64 (P,)) and the (n_img,) float64 optimal costs.
    assignment[i] == 1 where pick i is matched; dist is meaningful only there (the only place the reference's caller reads
    it): elsewhere it is 0, where the reference leaves the distance of a pairing that did not count."""
    if len(targets) != len(preds):
        raise ValueError("one target table and one pick table per image")
    # row-major copies: a table's column selection arrives column-major
    ts = [np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 3)) for t in targets]
    ps = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3)) for p in preds]
    po = np.concatenate([[0], np.cumsum([len(p) for p in ps])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int64)
    cat = lambda rows: torch.as_tensor(np.concatenate(rows, 0) if rows else np.zeros((0, 3))).to(device)  # noqa: E731
    p2t, dist, total = hipops.match_coordinates(cat(ps), cat(ts), po, to, radius)
    p2t, dist, total = p2t.cpu().numpy(), dist.cpu().numpy(), total.cpu().numpy()
    out = []
    for i in range(len(ps)):
        sl = slice(int(po[i]), int(po[i + 1]))
        out.append(((p2t[sl] >= 0).astype(np.float32), dist[sl].copy()))
    return out, total


def match_coordinates(targets, preds, radius):
    """(assignment float32 (P,), dist float64 (P,)) for one image; see match_coordinates_batch."""
    return match_coordinates_batch([targets], [preds], radius)[0][0]
