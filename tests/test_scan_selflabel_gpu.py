"""csrc/scan_selflabel.hip through hipops.scan_graph_eval / scan_selflabel_loss against the float64 restatement of
tests/selflabel_ref.py, and the steps after SCAN's clustering end to end (ScanHeads.evaluate / .selflabel, scan_main --select_head
graph --selflabel_epochs).

Tolerance.  Measured on the reference, not on the kernel: over the cases of selflabel_ref the largest deviation of the reference's
own float32 run on the CPU (tests/golden/scan/selflabel_small.npz `*_f32`) from its float64 values, a figure v normalised as
|dv| / (1 + |v|), a gradient as max |dg| / max |g| of its case; the tests allow 4 x that (another float32 summation order is as
valid as torch's).  target, mask, count, info and best are exact.  (DESIGN.md 4.27 has the figures.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_ref as SR
import selflabel_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "scan", "selflabel_small.npz")
SCORED = [n for n in sorted(R.SELFLABEL_CASES) if n != R.NONE_CASE]


@pytest.fixture(scope="module")
def bounds():
    g = np.load(GOLDEN)
    dev_v = max([R.norm_value(g["gr_%s_stats_f32" % n], g["gr_%s_stats_f64" % n]) for n in R.GRAPH_CASES]
                + [R.norm_value(g["sl_%s_loss_f32" % n], g["sl_%s_loss_f64" % n]) for n in SCORED])
    dev_g = max(R.norm_grad(g["sl_%s_grad_f32" % n], g["sl_%s_grad_f64" % n]) for n in SCORED)
    print("reference float32 deviation: figures %.3e, gradients %.3e" % (dev_v, dev_g))
    assert 0 < dev_v < 1e-5 and 0 < dev_g < 1e-5          # a float32 rounding, not a broken fixture
    return 4 * dev_v, 4 * dev_g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_selflabel(name):
    from cet_pick_amd import hipops as H
    weak, strong, threshold, balance, up = R.selflabel_inputs(name)
    tw, ts = dev(weak).requires_grad_(True), dev(strong).requires_grad_(True)
    loss, info, count, target, mask = H.scan_selflabel(tw, ts, threshold, balance)
    (loss * up).backward()
    assert tw.grad is None                                 # target and mask are not differentiable
    return loss.detach(), ts.grad, info, count, target, mask


@pytest.mark.parametrize("name", sorted(R.SELFLABEL_CASES))
def test_selflabel_loss_and_gradient(bounds, name):
    import torch
    bound_v, bound_g = bounds
    weak, strong, threshold, balance, up = R.selflabel_inputs(name)
    want = R.selflabel(weak, strong, threshold, balance, upstream=up)
    loss, grad, info, count, target, mask = run_selflabel(name)
    assert loss.dtype == grad.dtype == torch.float32 and loss.dim() == 0 and tuple(grad.shape) == weak.shape
    assert (info.dtype, count.dtype, target.dtype, mask.dtype) == (torch.int32, torch.int32, torch.int32, torch.uint8)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert np.array_equal(target.cpu().numpy(), want["target"]) and np.array_equal(mask.cpu().numpy(), want["mask"])
    assert np.array_equal(count.cpu().numpy(), want["count"]) and info.cpu().tolist() == want["info"].tolist()
    ev = R.norm_value(loss.cpu().numpy(), want["loss"])
    eg = R.norm_grad(grad.cpu().numpy(), want["grad"])
    print("scan_selflabel %s: loss error / bound %.3f, gradient error / bound %.3f" % (name, ev / bound_v, eg / bound_g))
    assert ev <= bound_v
    assert eg <= bound_g
    if name == R.NONE_CASE:                                # no confident row: nothing divided, nothing moves
        assert float(loss) == 0.0 and not grad.any() and int(info[0]) == 0
    if name == "b255_c1":                                  # one class: every probability is 1
        assert float(loss) == 0.0 and not grad.any()


def test_modules_have_the_reference_signatures(bounds):
    import torch
    from cet_pick_amd.models.loss import ConfidenceBasedCE, MaskedCrossEntropyLoss
    for name in ("b515_c3", "b515_c3_unbalanced"):
        weak, strong, threshold, balance, _ = R.selflabel_inputs(name)
        want = R.selflabel(weak, strong, threshold, balance)
        ts = dev(strong).requires_grad_(True)
        loss = ConfidenceBasedCE(threshold, balance)(dev(weak), ts)
        loss.backward()
        assert R.norm_value(float(loss.detach()), want["loss"]) <= bounds[0] and R.norm_grad(ts.grad.cpu().numpy(), want["grad"]) <= bounds[1]
        weight = torch.from_numpy(want["weight"].astype(np.float32)).cuda() if balance else None
        masked = MaskedCrossEntropyLoss()(dev(strong), dev(want["target"]).long(), dev(want["mask"]).bool(), weight, reduction="mean")
        assert float(masked) == float(loss.detach())
    weak, strong, threshold, balance, _ = R.selflabel_inputs(R.NONE_CASE)
    with pytest.raises(ValueError, match="all zeros"):
        ConfidenceBasedCE(threshold, balance)(dev(weak), dev(strong))
    with pytest.raises(ValueError, match="all zeros"):
        MaskedCrossEntropyLoss()(dev(strong), torch.zeros(len(strong), dtype=torch.long, device="cuda"),
                                 torch.zeros(len(strong), dtype=torch.bool, device="cuda"), None)


@pytest.mark.parametrize("name", sorted(R.GRAPH_CASES))
def test_graph_eval(bounds, name):
    import torch
    from cet_pick_amd import hipops as H
    logits, index, nheads, with_self = R.graph_inputs(name)
    want, want_best = R.graph_eval(logits, index, nheads, with_self)
    stats, best = H.scan_graph_eval(dev(logits), dev(index), nheads, with_self=with_self)
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (nheads, 3) and best.dtype == torch.int32 and tuple(best.shape) == (1,)
    assert bool(torch.isfinite(stats).all())
    ev = R.norm_value(stats.cpu().numpy(), want)
    print("scan_graph_eval %s: figures error / bound %.3f" % (name, ev / bounds[0]))
    assert ev <= bounds[0]
    assert R.best_gap(want) > 100 * bounds[0] * (1 + np.abs(want[:, 0]).max())          # every case is built to that
    assert int(best) == want_best


def test_an_exact_tie_goes_to_the_lowest_head():
    from cet_pick_amd import hipops as H
    logits, index, _, _ = R.graph_inputs("n257_k1_c64_noself")
    stats, best = H.scan_graph_eval(dev(np.tile(logits, (1, 3))), dev(index), 3, with_self=False)
    assert int(best) == 0 and float(stats[0, 0]) == float(stats[1, 0]) == float(stats[2, 0])


@pytest.mark.parametrize("name", ["b515_c3", "pm200", "b257_c33", R.NONE_CASE])
def test_selflabel_same_input_same_bytes(name):
    import torch
    first, second = run_selflabel(name), run_selflabel(name)
    for x, y in zip(first, second):
        assert torch.equal(x, y)


def test_assign_and_selflabel_share_one_argmax_and_one_softmax():
    """mi_scan_assign (scan_loss.hip) and the self-label forward on the same weak logits, one index_select'ed batch: B = 257 is two
    chunks with a ragged last chunk and a ragged wave, C = 33 leaves off-lanes, H = 1.  At threshold 0 every row is confident
    (its largest probability is above 0 for any finite logits), so the targets are the labels; conf is the label's entry of prob
    bit for bit; and two equal maxima go to the lower class at both entry points."""
    import torch
    from cet_pick_amd import hipops as H
    rng = np.random.default_rng(257)
    pool = dev((2.0 * rng.standard_normal((400, 33))).astype(np.float32))
    weak = pool.index_select(0, dev(rng.permutation(400)[:257]))
    strong = weak + 0.5 * dev(rng.standard_normal((257, 33)).astype(np.float32))
    label, conf, _, prob = H.scan_assign(weak, 1, with_prob=True)
    _, _, _, target, mask = H.scan_selflabel(weak, strong, 0.0)
    assert tuple(target.shape) == (257,) and torch.equal(target, label[:, 0]) and bool((mask == 1).all())
    assert torch.equal(conf, prob.gather(1, label.long()))
    tied = weak.clone()
    tied[256, 3] = tied[256, 17] = tied[256].max() + 1.0   # the ragged chunk's row: classes 3 and 17 equal, above the rest
    assert int(np.argmax(tied[256].cpu().numpy())) == 3 and float(tied[256, 3]) == float(tied[256, 17])
    assert int(H.scan_assign(tied, 1)[0][256, 0]) == 3
    assert int(H.scan_selflabel(tied, strong, 0.0)[3][256]) == 3


@pytest.mark.parametrize("name", ["n515_k5_h3_c33", "n257_k20_h16_c2", "x30"])
def test_graph_eval_same_input_same_bytes(name):
    import torch
    from cet_pick_amd import hipops as H
    logits, index, nheads, with_self = R.graph_inputs(name)
    first = H.scan_graph_eval(dev(logits), dev(index), nheads, with_self=with_self)
    second = H.scan_graph_eval(dev(logits), dev(index), nheads, with_self=with_self)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_refusals():
    """outside the limits nothing is launched: the wrappers raise, and the entries themselves answer with a bad-argument status"""
    import torch
    from cet_pick_amd import hipops as H, _lib as L
    refused = (ValueError, L.HipExtensionError)
    idx = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(refused):
        H.scan_graph_eval(torch.zeros(4, 65, device="cuda"), idx, 1)                     # C = 65
    with pytest.raises(refused):
        H.scan_graph_eval(torch.zeros(4, 17, device="cuda"), idx, 17)                    # H = 17
    with pytest.raises(refused):
        H.scan_graph_eval(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 65, dtype=torch.int32, device="cuda"), 1)      # k = 65
    with pytest.raises(refused):
        H.scan_graph_eval(torch.zeros(4, 3, device="cuda"), torch.zeros(3, 2, dtype=torch.int32, device="cuda"), 1)
    with pytest.raises(refused):
        H.scan_graph_eval(torch.zeros(4, 3, device="cuda"), idx.long(), 1)
    with pytest.raises(ValueError, match="outside 0..3"):
        H.scan_graph_eval(torch.zeros(4, 3, device="cuda"), idx + 4, 1)                  # the table is checked here, not on the device
    with pytest.raises(ValueError, match="outside 0..3"):
        H.scan_graph_eval(torch.zeros(4, 3, device="cuda"), idx - 1, 1)
    with pytest.raises(refused):
        H.scan_selflabel_loss(torch.zeros(4, 65, device="cuda"), torch.zeros(4, 65, device="cuda"), 0.5)
    with pytest.raises(refused):
        H.scan_selflabel_loss(torch.zeros(65537, 1, device="cuda"), torch.zeros(65537, 1, device="cuda"), 0.5)     # B = 65537
    with pytest.raises(refused):
        H.scan_selflabel_loss(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 2, device="cuda"), 0.5)
    with pytest.raises(refused):
        H.scan_selflabel_loss(torch.zeros(4, 6, device="cuda")[:, ::2], torch.zeros(4, 3, device="cuda"), 0.5)
    lib = L.lib()
    buf = torch.zeros(4096, device="cuda")
    p = L.ptr(buf)
    for n, c, h, k in ((4, 65, 1, 2), (4, 3, 17, 2), (4, 3, 1, 65), (4, 3, 1, 0), (0, 3, 1, 2)):
        assert lib.mi_scan_graph_eval(p, n, c, h, p, k, 1, p, p, p, 4096, L.stream()) == -1
    for b, c in ((4, 65), (65537, 3), (0, 3), (4, 0)):
        assert lib.mi_scan_selflabel_fwd(p, p, b, c, 0.5, 1, p, p, p, p, p, p, p, 4096, L.stream()) == -1
        assert lib.mi_scan_selflabel_bwd(p, b, c, 1, p, p, p, p, p, p, p, L.stream()) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                   # nothing ran


# The float64 restatement's own loops (scan_ref.train, then selflabel_ref.selflabel_train on the head graph_eval chooses: the same
# draws, the same start, Adam) on these blobs - 30 clustering epochs with lr 0.03, batch 100, weight decay 1e-4, seed 317, then 10
# self-label epochs at threshold 0.9 with lr 1e-4, 0.01 or 0.03 - keep every blob in one class of its own; every pick is
# confident from the first self-label epoch on.
E2E = dict(num_epochs=30, batch_size=100, lr=0.03, weight_decay=1e-4)
SELFLABEL = dict(num_epochs=10, batch_size=100, lr=0.01, threshold=0.9)


def test_blobs_end_to_end(bounds, tmp_path):
    import torch
    from cet_pick_amd import hipops as H
    from cet_pick_amd.utils import scan as S
    x, blob = SR.blobs()
    t = dev(x)
    index = H.knn_search(t, t, 5, metric="l2", exclude_self=True)[0].cpu().numpy()
    heads = S.ScanHeads(16, 3, nheads=2, seed=317)
    heads.fit(x, index, entropy_weight=2.0, **E2E)
    # the head the restatement chooses from the device's own logits
    logits = heads._logits(heads._embeddings(x)).detach().cpu().numpy()
    want_stats, want_best = R.graph_eval(logits, index, 2, with_self=True)
    stats = heads.evaluate(x, index)
    assert stats.shape == (2, 3) and R.norm_value(stats, want_stats) <= bounds[0]
    assert heads.best_loss_head == want_best and heads.best_loss == float(stats[want_best, 0])
    one, sl = heads.selflabel(x, index, heads.best_loss_head, balance=True, **SELFLABEL)
    assert sl.shape == (10, 3) and np.isfinite(sl).all() and (sl[:, 1] > 0).all() and (sl[:, 1] <= 1).all()
    assert (one.nheads, one.epoch, one.best_loss_head) == (1, 40, 0) and list(one.state_dict()) == S.state_keys(1)
    assert heads.nheads == 2 and heads.epoch == 30         # the clustering heads are left as they were
    label = one.predict(x)[0]
    assert SR.blobs_separated(label[:, 0], blob)
    # the same self-labelling in float64 on the host ends in the same classes
    sd = heads.state_dict()
    w0, b0 = sd["cluster_head.%d.weight" % want_best].cpu().numpy(), sd["cluster_head.%d.bias" % want_best].cpu().numpy()
    w, b, sl64 = R.selflabel_train(x, index, w0, b0, S.selflabel_draws, 317, 30, 10, 100, SELFLABEL["lr"], 0.9, True)
    assert SR.blobs_separated(SR.assign(x.astype(np.float64) @ w.T + b, 1)[0][:, 0], blob)
    assert np.abs(sl[:, 1:] - sl64[:, 1:]).max() <= 1e-6   # the same picks are confident, the same classes present (counts / 300 in fp32)


def test_scan_main_select_head_graph_selflabel_and_load_model(bounds, tmp_path):
    import torch
    from cet_pick_amd.utils import scan as S
    x, blob = SR.blobs()
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["t%d" % (i % 2) for i in range(len(x))]),
             coords=np.arange(3 * len(x)).reshape(-1, 3))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "cet_pick_amd.scan_main", "--input", str(tmp_path / "all_output_info.npz"), "--nclusters", "3",
            "--num_neighbor", "5"]
    out = tmp_path / "out"
    run = subprocess.run(base + ["--path", str(out), "--nheads", "2", "--num_epochs", "30", "--batch_size", "100", "--lr", "0.03",
                                 "--select_head", "graph", "--selflabel_epochs", "10", "--selflabel_threshold", "0.9",
                                 "--selflabel_lr", "0.01"], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("scan_main: epoch ") == 30 and run.stdout.count("scan_main: self-label epoch ") == 10
    for f in ("scan_heads.pth", "scan_labels.npz", "scan_heads_selflabel.pth", "scan_labels_selflabel.npz"):
        assert os.path.exists(out / f), f
    # the clustering step's files, with the graph's figures and the graph's head
    lab = np.load(out / "scan_labels.npz")
    assert sorted(lab.files) == ["conf", "coords", "counts", "head", "label", "name", "prob", "stats"]
    heads = S.ScanHeads.load(out / "scan_heads.pth")
    index = SR.knn_l2(x, 5)
    logits = heads._logits(heads._embeddings(x)).detach().cpu().numpy()
    want_stats, want_best = R.graph_eval(logits, index, 2, with_self=True)
    assert int(lab["head"]) == heads.best_loss_head == want_best
    assert lab["stats"].shape == (2, 3) and np.isfinite(lab["stats"]).all() and R.norm_value(lab["stats"], want_stats) <= bounds[0]
    # the self-labelled head
    sl = np.load(out / "scan_labels_selflabel.npz")
    assert sorted(sl.files) == sorted(lab.files + ["selflabel_stats"])
    assert sl["selflabel_stats"].shape == (10, 3) and sl["selflabel_stats"].dtype == np.float32
    assert (sl["selflabel_stats"][:, 1] > 0).all() and (sl["selflabel_stats"][:, 1] <= 1).all()
    assert int(sl["head"]) == 0 and sl["counts"].shape == (1, 3) and sl["stats"].shape == (1, 3) and sl["label"].shape == (300,)
    assert SR.blobs_separated(sl["label"], blob)
    ck = torch.load(out / "scan_heads_selflabel.pth", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "best_loss_head", "epoch", "optimizer", "state_dict"]
    assert (ck["epoch"], ck["best_loss_head"]) == (40, 0) and list(ck["state_dict"]) == S.state_keys(1)
    # --load_model reads it as one head and reproduces the labels; with --select_head graph its stats are figures, not NaN
    out2 = tmp_path / "out2"
    run = subprocess.run(base + ["--path", str(out2), "--nheads", "1", "--load_model", str(out / "scan_heads_selflabel.pth"),
                                 "--select_head", "graph"], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    lab2 = np.load(out2 / "scan_labels.npz")
    assert np.array_equal(lab2["label"], sl["label"]) and np.array_equal(lab2["conf"], sl["conf"])
    assert np.array_equal(lab2["stats"], sl["stats"]) and np.isfinite(lab2["stats"]).all()
    assert not os.path.exists(out2 / "scan_heads.pth") and not os.path.exists(out2 / "scan_heads_selflabel.pth")
