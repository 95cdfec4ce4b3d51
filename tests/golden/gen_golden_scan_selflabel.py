"""Golden values of the graph evaluation and of the self-labelling loss -> scan/selflabel_small.npz, by IMPORTING the reference
(`ConfidenceBasedCE`, `MaskedCrossEntropyLoss`: models/loss.py:15-66; `scan_evaluate`: trains/eval_utils.py:74-102) and running it
on the CPU in float64 and in float32, with torch's autograd for the gradients.  Run:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_scan_selflabel.py
Importing gen_golden brings its package stubs and the reference onto sys.path (as gen_golden_scan.py).  The fixture holds results
only; the inputs are tests/selflabel_ref.py::selflabel_inputs(name) and graph_inputs(name).
  sl_{name}_loss_{f64,f32}, sl_{name}_grad_{f64,f32}: the unbalanced cases through ConfidenceBasedCE(t, False) as a whole; the
      balanced ones through the reference's MaskedCrossEntropyLoss with the weight vector formed HERE exactly as ConfidenceBasedCE
      forms it (1 / (counts.float() / n) - its own line puts the vector on a CUDA device and cannot run on a CPU) from the
      reference's own target and mask lines.  The last case has no confident row: the reference raises, nothing is stored.
  sl_{name}_target, _mask, _count: what the float64 run found (exact)
  gr_{name}_stats_{f64,f32} (H, 3): total, consistency, entropy of scan_evaluate per head; gr_{name}_best: its lowest_loss_head
The input conditions the tests rely on are asserted here: no row's largest probability within 1e-4 of its case's threshold, no row
with two equal maxima, n >= 1 in every case but the last, and the two lowest totals of every graph case well apart."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (stubs + sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import selflabel_ref as R  # noqa: E402


def check_selflabel_inputs(name, weak, threshold):
    p = R.softmax(weak.astype(np.float64))
    top = np.sort(weak, axis=1)[:, ::-1]
    assert (np.abs(p.max(1) - threshold) > R.MARGIN).all(), name
    assert weak.shape[1] == 1 or (top[:, 0] > top[:, 1]).all(), name
    n = int((p.max(1) > threshold).sum())
    assert (n == 0) == (name == R.NONE_CASE), (name, n)


def run_selflabel(RL, weak, strong, threshold, balance, up, dtype):
    weak = torch.from_numpy(weak).to(dtype)
    strong = torch.from_numpy(strong).to(dtype).requires_grad_(True)
    if not balance:
        loss = RL.ConfidenceBasedCE(threshold, False)(weak, strong)
        max_prob, target = torch.max(torch.softmax(weak, dim=1), dim=1)
        mask = max_prob > threshold
    else:
        max_prob, target = torch.max(torch.nn.Softmax(dim=1)(weak), dim=1)       # ConfidenceBasedCE.forward, its lines
        mask = max_prob > threshold
        target_masked = torch.masked_select(target, mask.squeeze())
        n = target_masked.size(0)
        idx, counts = torch.unique(target_masked, return_counts=True)
        freq = 1 / (counts.float() / n)
        weight = torch.ones(weak.shape[1])
        weight[idx] = freq
        loss = RL.MaskedCrossEntropyLoss()(strong, target, mask, weight=weight.to(dtype), reduction="mean")
    (loss * up).backward()
    count = np.bincount(target[mask].numpy(), minlength=weak.shape[1])
    return loss.detach().numpy(), strong.grad.numpy(), target.numpy().astype(np.int32), mask.numpy().astype(np.uint8), count


def run_graph(scan_evaluate, logits, index, nheads, with_self, dtype):
    n = logits.shape[0]
    z = torch.from_numpy(logits).to(dtype).reshape(n, nheads, -1)
    neighbors = torch.from_numpy(R.table(index, with_self))
    res = scan_evaluate([{"probabilities": torch.softmax(z[:, h], dim=1), "neighbors": neighbors} for h in range(nheads)])
    stats = np.array([[o["total_loss"], o["consistency"], o["entropy"]] for o in res["scan"]], np.float64)
    return stats, int(res["lowest_loss_head"])


def gen():
    from cet_pick.models import loss as RL
    from cet_pick.trains.eval_utils import scan_evaluate
    out = {}
    for name in sorted(R.SELFLABEL_CASES):
        weak, strong, threshold, balance, up = R.selflabel_inputs(name)
        check_selflabel_inputs(name, weak, threshold)
        if name == R.NONE_CASE:
            for dtype in (torch.float64, torch.float32):
                try:
                    run_selflabel(RL, weak, strong, threshold, balance, up, dtype)
                except ValueError as e:
                    print(name, "the reference raises:", e)
                else:
                    raise AssertionError("the reference was expected to raise on an all-zero mask")
            continue
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            loss, grad, target, mask, count = run_selflabel(RL, weak, strong, threshold, balance, up, dtype)
            out.update({"sl_%s_loss_%s" % (name, tag): loss, "sl_%s_grad_%s" % (name, tag): grad})
            if tag == "f64":
                out.update({"sl_%s_target" % name: target, "sl_%s_mask" % name: mask, "sl_%s_count" % name: count})
            else:                                          # the float32 run sees the same rows and classes
                assert np.array_equal(target, out["sl_%s_target" % name]) and np.array_equal(mask, out["sl_%s_mask" % name]), name
        print(name, "threshold %.6f n %d" % (threshold, int(out["sl_%s_mask" % name].sum())), out["sl_%s_loss_f64" % name],
              out["sl_%s_loss_f32" % name])
    for name in sorted(R.GRAPH_CASES):
        logits, index, nheads, with_self = R.graph_inputs(name)
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            stats, best = run_graph(scan_evaluate, logits, index, nheads, with_self, dtype)
            out["gr_%s_stats_%s" % (name, tag)] = stats.astype(np.float64 if tag == "f64" else np.float32)
            if tag == "f64":
                out["gr_%s_best" % name] = np.int32(best)
        print(name, out["gr_%s_stats_f64" % name][:, 0], "best", int(out["gr_%s_best" % name]),
              "gap %.3g" % R.best_gap(out["gr_%s_stats_f64" % name]))
    # the tests' figure bound is 4 x the largest float32 deviation below; `best` needs the two lowest totals 100 bounds apart
    dev = max([R.norm_value(out["gr_%s_stats_f32" % n], out["gr_%s_stats_f64" % n]) for n in R.GRAPH_CASES]
              + [R.norm_value(out["sl_%s_loss_f32" % n], out["sl_%s_loss_f64" % n]) for n in R.SELFLABEL_CASES if n != R.NONE_CASE])
    print("float32 deviation of the figures %.3e" % dev)
    for name in sorted(R.GRAPH_CASES):
        stats = out["gr_%s_stats_f64" % name]
        assert R.best_gap(stats) > 100 * 4 * dev * (1 + np.abs(stats[:, 0]).max()), (name, R.best_gap(stats))
    os.makedirs(os.path.join(HERE, "scan"), exist_ok=True)
    G.save(os.path.join("scan", "selflabel_small.npz"), **out)


if __name__ == "__main__":
    gen()
