"""csrc/scan_loss.hip through hipops.scan_loss / scan_assign against the float64 restatement of tests/scan_ref.py, and the SCAN
step end to end (utils/scan.ScanHeads, python -m cet_pick_amd.scan_main).

Tolerance.  Measured on the reference, not on the kernel: over the cases of scan_ref.CASES the largest deviation of the reference's
own float32 SCANLoss on the CPU (tests/golden/scan/scan_small.npz `*_f32`) from its float64 values, a figure v normalised as
|dv| / (1 + |v|), a gradient as max |dg| / max |g| over both gradient tensors of its case; the tests allow 4 x that (another float32
summation order is as valid as torch's).  With the golden file as it is: figures 1.74e-7 -> 7.0e-7, gradients 8.2e-7 -> 3.3e-6
(DESIGN.md 4.25)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "scan", "scan_small.npz")


@pytest.fixture(scope="module")
def bounds():
    g = np.load(GOLDEN)
    dev_v = max(max(R.norm_value(g[n + "_stats_f32"], g[n + "_stats_f64"]), R.norm_value(g[n + "_total_f32"], g[n + "_total_f64"]))
                for n in R.CASES)
    dev_g = max(R.norm_grad((g[n + "_da_f32"], g[n + "_db_f32"]), (g[n + "_da_f64"], g[n + "_db_f64"])) for n in R.CASES)
    print("reference float32 deviation: figures %.3e, gradients %.3e" % (dev_v, dev_g))
    assert 0 < dev_v < 1e-5 and 0 < dev_g < 1e-5          # a float32 rounding, not a broken fixture
    return 4 * dev_v, 4 * dev_g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_loss(name):
    from cet_pick_amd import hipops as H
    a, b, nheads, up = R.case_inputs(name)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    loss, stats = H.scan_loss(ta, tb, nheads, R.ENTROPY_WEIGHT)
    (loss * up).backward()
    return loss.detach(), stats.detach(), ta.grad, tb.grad


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_loss_and_gradients(bounds, name):
    import torch
    bound_v, bound_g = bounds
    a, b, nheads, up = R.case_inputs(name)
    loss, stats, da, db = run_loss(name)
    assert stats.dtype == loss.dtype == da.dtype == torch.float32 and tuple(stats.shape) == (nheads, 3) and loss.dim() == 0
    assert not stats.requires_grad
    want_stats, want_total = R.loss(a, b, nheads)
    want_grads = R.grads(a, b, nheads, upstream=up)
    for t in (loss, stats, da, db):
        assert bool(torch.isfinite(t).all())
    ev = max(R.norm_value(stats.cpu().numpy(), want_stats), R.norm_value(loss.cpu().numpy(), np.float64(want_total)))
    eg = R.norm_grad((da.cpu().numpy(), db.cpu().numpy()), want_grads)
    print("scan_loss %s: figures error / bound %.3f, gradients error / bound %.3f" % (name, ev / bound_v, eg / bound_g))
    assert ev <= bound_v
    assert eg <= bound_g
    if name == "chunk_less_c1":                            # one class: every probability is 1 and nothing moves
        assert not da.any() and not db.any() and not stats.any()


def test_single_head_module_has_the_reference_signature(bounds):
    from cet_pick_amd.models.loss import SCANLoss, MultiHeadSCANLoss
    a, b, nheads, _ = R.case_inputs("upstream")
    c = a.shape[1] // nheads
    total, consistency, entropy = SCANLoss(entropy_weight=R.ENTROPY_WEIGHT)(dev(a[:, :c]), dev(b[:, :c]))
    want, _ = R.loss(a[:, :c], b[:, :c], 1)
    assert R.norm_value(np.array([float(total), float(consistency), float(entropy)]), want[0]) <= bounds[0]
    both, stats = MultiHeadSCANLoss(nheads)(dev(a), dev(b))
    assert float(stats[0, 0]) == float(total) and R.norm_value(float(both), np.float64(R.loss(a, b, nheads)[1])) <= bounds[0]


@pytest.mark.parametrize("name", ["chunks_c3", "extreme", "chunk_more_h16"])
def test_same_input_same_bytes(name):
    import torch
    first, second = run_loss(name), run_loss(name)
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [1, R.CHUNK + 1, 70000])
def test_assign(bounds, n):
    from cet_pick_amd import hipops as H
    nheads, c = 3, 5
    rng = np.random.default_rng(n)
    z = rng.standard_normal((n, nheads, c)).astype(np.float32)
    best = rng.integers(0, c, size=(n, nheads))
    np.put_along_axis(z, best[..., None], z.max(-1, keepdims=True) + 1.0, axis=-1)       # a margin of 1 over the second logit
    z[0, 1, :] = [0.25, 1.5, -1.0, 1.5, 1.5]                                             # an exact tie: the lowest index, 1
    z = z.reshape(n, nheads * c)
    want_label, want_conf, want_counts, want_prob = R.assign(z, nheads)
    assert want_label[0, 1] == 1
    label, conf, counts, prob = H.scan_assign(dev(z), nheads, with_prob=True)
    assert tuple(label.shape) == tuple(conf.shape) == (n, nheads) and tuple(counts.shape) == (nheads, c)
    assert np.array_equal(label.cpu().numpy(), want_label)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and int(counts.sum()) == n * nheads
    ec, ep = R.norm_value(conf.cpu().numpy(), want_conf), R.norm_value(prob.cpu().numpy(), want_prob)
    print("scan_assign n = %d: conf error / bound %.3f, prob error / bound %.3f" % (n, ec / bounds[0], ep / bounds[0]))
    assert ec <= bounds[0] and ep <= bounds[0]
    label2, conf2, counts2, none = H.scan_assign(dev(z), nheads)
    assert none is None and np.array_equal(label2.cpu().numpy(), want_label) and np.array_equal(counts2.cpu().numpy(), want_counts)
    assert np.array_equal(conf2.cpu().numpy(), conf.cpu().numpy())


def test_refusals():
    """outside the limits nothing is launched: the wrappers raise, and the entries themselves answer with a bad-argument status"""
    import torch
    from cet_pick_amd import hipops as H, _lib as L
    refused = (ValueError, L.HipExtensionError)
    z = torch.zeros(4, 65, device="cuda")
    with pytest.raises(refused):
        H.scan_loss(z, z, 1)                               # C = 65
    with pytest.raises(refused):
        H.scan_assign(z, 1)
    z = torch.zeros(4, 17, device="cuda")
    with pytest.raises(refused):
        H.scan_loss(z, z, 17)                              # H = 17
    z = torch.zeros(0, 3, device="cuda")
    with pytest.raises(refused):
        H.scan_loss(z, z, 1)                               # B = 0
    with pytest.raises(refused):
        H.scan_assign(z, 1)
    z = torch.zeros(4, 6, device="cuda")[:, ::2]
    with pytest.raises(refused):
        H.scan_loss(z, z, 1)                               # not contiguous
    with pytest.raises(refused):
        H.scan_loss(torch.zeros(4, 3, device="cuda"), z, 1)
    with pytest.raises(refused):
        H.scan_assign(z, 1)
    with pytest.raises(refused):
        H.scan_loss(torch.zeros(65537, 1, device="cuda"), torch.zeros(65537, 1, device="cuda"), 1)
    lib = L.lib()
    for b, c, h in ((4, 65, 1), (4, 1, 17), (0, 3, 1), (65537, 3, 1), (4, 0, 1), (4, 3, 0)):
        assert lib.mi_scan_loss_workspace_bytes(b, c, h) == 0
    assert lib.mi_scan_loss_workspace_bytes(65536, 64, 16) > 0
    buf = torch.zeros(4096, device="cuda")
    p = L.ptr(buf)
    for b, c, h in ((4, 65, 1), (4, 1, 17), (0, 3, 1)):
        assert lib.mi_scan_loss_fwd(p, p, b, c, h, 2.0, p, p, p, p, 4096, L.stream()) == -1
        assert lib.mi_scan_loss_bwd(p, p, b, c, h, 2.0, p, p, p, p, L.stream()) == -1
        assert lib.mi_scan_assign(p, b, c, h, p, p, None, p, L.stream()) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                   # nothing ran


# The float64 restatement's own training loop (scan_ref.train: the same draws, the same start, Adam) on these blobs with
# lr 0.03, batch 100, weight decay 1e-4, seed 317 gives every blob one class of the best head, the three classes different, after
# 5 epochs, and after 10, 15, 20, 30 and 40 (both heads from epoch 15 on).  The test trains 30 epochs: at most half are needed.
E2E = dict(num_epochs=30, batch_size=100, lr=0.03, weight_decay=1e-4)
E2E_RESTATEMENT_EPOCHS = 15


def _graph(x, k):
    from cet_pick_amd import hipops as H
    t = dev(x)
    return H.knn_search(t, t, k, metric="l2", exclude_self=True)[0].cpu().numpy()


def test_blobs_end_to_end(tmp_path):
    import torch
    from cet_pick_amd.utils import scan as S
    assert 2 * E2E_RESTATEMENT_EPOCHS <= E2E["num_epochs"]
    x, blob = R.blobs()
    assert x.shape == (300, 16)
    index = _graph(x, 5)
    assert np.array_equal(index, R.knn_l2(x, 5))
    heads = S.ScanHeads(16, 3, nheads=2, seed=317)
    assert list(heads.state_dict()) == S.state_keys(2)
    assert heads.state_dict()["cluster_head.1.weight"].data_ptr() == heads.lin.weight[3:6].data_ptr()       # a slice, not a copy
    history = heads.fit(x, index, entropy_weight=2.0, **E2E)
    assert history.shape == (30, 2, 3) and np.isfinite(history).all()
    assert heads.best_loss_head == int(np.argmin(history[-1][:, 0])) and heads.best_loss == float(history[-1][:, 0].min())
    label, conf, counts = heads.predict(x)
    assert R.blobs_separated(label[:, heads.best_loss_head], blob)
    assert counts[heads.best_loss_head].tolist() == [100, 100, 100]
    # the same training in float64 on the host ends in the same classes
    w0, b0 = S.initial_heads(16, 3, 2, 317)
    w, b, hist64 = R.train(x, index, w0.numpy(), b0.numpy(), 2, S.draw_neighbours, 317, E2E_RESTATEMENT_EPOCHS, 100, 0.03, 1e-4)
    want = R.assign(x.astype(np.float64) @ w.T + b, 2)[0]
    assert R.blobs_separated(want[:, int(np.argmin(hist64[-1][:, 0]))], blob)
    # checkpoint round trip
    heads.save(tmp_path / "heads.pth")
    again = S.ScanHeads.load(tmp_path / "heads.pth")
    assert (again.epoch, again.best_loss_head, again.best_loss) == (30, heads.best_loss_head, heads.best_loss)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in heads.state_dict().items())
    assert np.array_equal(again.predict(x)[0], label)


def test_scan_main_writes_its_files_and_load_model_reproduces_the_labels(tmp_path):
    import torch
    x, blob = R.blobs()
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["t%d" % (i % 2) for i in range(len(x))]),
             coords=np.arange(3 * len(x)).reshape(-1, 3))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "cet_pick_amd.scan_main", "--input", str(tmp_path / "all_output_info.npz"), "--nclusters", "3",
            "--nheads", "2", "--num_neighbor", "5"]
    out = tmp_path / "out"
    run = subprocess.run(base + ["--path", str(out), "--num_epochs", "30", "--batch_size", "100", "--lr", "0.03"], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("scan_main: epoch ") == 30 and "picks per class: " in run.stdout.splitlines()[-1]
    assert os.path.exists(out / "scan_heads.pth") and os.path.exists(out / "scan_labels.npz")
    lab = np.load(out / "scan_labels.npz")
    assert sorted(lab.files) == ["conf", "coords", "counts", "head", "label", "name", "prob", "stats"]
    assert lab["label"].shape == (300,) and lab["prob"].shape == (300, 3) and lab["counts"].shape == (2, 3) and lab["stats"].shape == (2, 3)
    assert R.blobs_separated(lab["label"], blob)
    ck = torch.load(out / "scan_heads.pth", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_loss", "best_loss_head", "epoch", "optimizer", "state_dict"] and ck["epoch"] == 30
    assert ck["best_loss_head"] == int(lab["head"])
    out2 = tmp_path / "out2"
    run = subprocess.run(base + ["--path", str(out2), "--load_model", str(out / "scan_heads.pth")], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    lab2 = np.load(out2 / "scan_labels.npz")
    assert np.array_equal(lab2["label"], lab["label"]) and np.array_equal(lab2["conf"], lab["conf"])
    assert not os.path.exists(out2 / "scan_heads.pth")
