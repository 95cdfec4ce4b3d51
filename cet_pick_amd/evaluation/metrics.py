"""precision_recall_curve of the reference (evaluation/metrics.py:6-46): plumbing, numpy on the host."""
import numpy as np


def precision_recall_curve(target, pred, N=None):
    """(pr, re, threshold, avpr) over the picks sorted by falling score.  Picks of equal score share one bucket (k entries,
    r hits); precision 0 / 0 counts as 1; avpr = sum over buckets of precision * hits / n, n = N or the number of hits.
    As in the reference the scores and hits are float32 and the running number of hits is a float32 sum."""
    target = np.asarray(target, dtype=np.float32)
    pred = np.asarray(pred, dtype=np.float32)
    n = target.sum() if N is None else N
    order = np.argsort(-pred, kind="stable")
    score, hit = -(-pred[order]), target[order]
    if len(score) == 0:
        raise ValueError("no picks to score")
    last = np.ones(len(score), dtype=bool)                 # last entry of every bucket of equal scores
    last[:-1] = score[:-1] != score[1:]
    pp = np.flatnonzero(last) + 1                          # predicted positives down to each bucket
    tp = np.cumsum(hit)[last].astype(int)                  # true positives down to each bucket
    r = np.diff(np.concatenate([[0], tp]))
    with np.errstate(invalid="ignore", divide="ignore"):
        pr = tp / pp
    pr[np.isnan(pr)] = 1
    avpr = np.sum(pr * r) / n
    re = tp / n
    return pr, re, score[last], avpr
