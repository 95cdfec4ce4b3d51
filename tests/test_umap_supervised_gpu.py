"""The label-supervised UMAP map on the MI355X (csrc/umap.hip: um_rowmax_kernel, um_supervise_kernel; utils/umap.py; plot_2d
--label_map) against the float64 arbiter tests/umap_sup_ref.py, on the graphs of test_umap_gpu.py.

Bands.  rowmax: s = wsym f is one double product of the device's own fp32 wsym and the host's factor, and a maximum rounds
nothing, so the device's value is the arbiter's up to the one rounding of that product, 2^-53 relative; IEEE multiplication
leaves no choice in that rounding, so equality is asserted.  wsup: values in [0, 1], one fp32 rounding (at most 2^-25) plus the
double noise of six operations (at most 12 2^-53, test_umap_supervised_cpu.py): |wsup - wsup64| <= 2^-24.  eps: the double formula on
the device's own fp32 wsup and wmax, bit for bit.  Epochs: the summed band of test_umap_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spectral_ref as S
import test_umap_gpu as G
import tsne_ref as T
import umap_ref as U
import umap_sup_ref as R

pytestmark = pytest.mark.gpu

REPO = G.REPO
N_EPOCHS = G.N_EPOCHS
CASES = [("smallest", "mod3", 0.5), ("hub", "mod3", 0.5), ("hub", "distinct", 0.5), ("hub", "mod3", 1.0), ("hub", "distinct", 1.0),
         ("wide", "mod3", 0.5)]
LISTED = ["a", "b", "far_dist", "label", "min_dist", "n_epochs", "n_neighbors", "seed", "target_weight", "y", "y01"]
_cache = {}


def _labels(n, which):
    if which == "distinct":
        return np.arange(n)
    label = np.arange(n) % 3
    label[[1, 4, 11, n - 2]] = -1                            # a handful of unknown ones
    return label


def _setup(name, which, tw):
    """The supervised tables of a case as the device made them, once per case."""
    key = (name, which, tw)
    if key not in _cache:
        import torch
        from cet_pick_amd import hipops as H
        g = G._setup(name)
        ti, rev_ptr, rev_edge, _, _ = g["dev"]
        label = _labels(g["N"], which)
        f = R.factors(tw)
        wsym, lab = G._dev(g["wsym"]), G._dev(label.astype(np.int32))
        rowmax = H.umap_rowmax(ti, wsym, lab, rev_ptr, rev_edge, *f)
        out = H.umap_supervise(ti, wsym, lab, rowmax, *f, N_EPOCHS)
        first = out[0].cpu().numpy().copy()
        wmax = out[0].max().reshape(1)
        wsup, eps = H.umap_supervise(ti, wsym, lab, rowmax, *f, N_EPOCHS, wmax=wmax, out=out)
        torch.cuda.synchronize()
        _cache[key] = dict(g=g, label=label, f=f, rowmax=rowmax.cpu().numpy(), first=first, wmax=float(wmax.item()),
                           wsup=wsup.cpu().numpy(), eps=eps.cpu().numpy(), dev_eps=eps, dev=(ti, wsym, lab, rowmax))
    return _cache[key]


@pytest.mark.parametrize("name,which,tw", CASES)
def test_rowmax_equals_float64(name, which, tw):
    s = _setup(name, which, tw)
    g = s["g"]
    m64 = R.supervise64(g["index"], g["wsym"], s["label"], *s["f"])[1]
    got = s["rowmax"]
    dev = np.abs(got - m64).max() / max(m64.max(), 2.0 ** -1000)
    print("%s %s tw %g: rowmax %.6g .. %.6g, %d zero rows, deviation max %.3g relative (one rounding: 2^-53 = %.3g)"
          % (name, which, tw, got.min(), got.max(), (got == 0).sum(), dev, 2.0 ** -53))
    assert got.dtype == np.float64 and got.shape == (g["N"],) and np.array_equal(got, m64)
    if name == "hub":
        ptr, _ = U.reverse_lists(g["index"])
        assert ptr[1] - ptr[0] > 64 and ptr[g["N"]] - ptr[g["N"] - 1] == 0      # two strides of the lanes; no reverse edge
        if tw == 0.5:
            assert got[0] > 0 and got[g["N"] - 1] > 0
    if (which, tw) == ("distinct", 1.0):
        assert (got == 0).all()


@pytest.mark.parametrize("name,which,tw", CASES)
def test_supervise_matches_float64(name, which, tw):
    s = _setup(name, which, tw)
    g = s["g"]
    n, k = g["index"].shape
    wsup64 = R.supervise64(g["index"], g["wsym"], s["label"], *s["f"])[0]
    err = np.abs(s["wsup"] - wsup64).max() / 2.0 ** -24
    # a graph without an edge left (all distinct at target_weight 1) has wmax 0, where the arbiter's formula is 0 / 0: the
    # kernel's rule for a weight that is not positive, +inf, stands in
    want = U.spacing64(s["wsup"], s["wmax"], N_EPOCHS) if s["wmax"] > 0 else np.full(s["wsup"].shape, np.inf)
    print("%s %s tw %g: |wsup - wsup64| max %.4f of 2^-24, wmax %.8g, %d of %d edges zero, %d pruned (plain: %d), eps equal %s"
          % (name, which, tw, err, s["wmax"], (s["wsup"] == 0).sum(), n * k, np.isinf(want).sum(), np.isinf(g["eps"]).sum(),
             np.array_equal(s["eps"], want)))
    assert s["wsup"].dtype == np.float32 and s["wsup"].shape == (n, k) and err <= 1.0
    assert s["wmax"] == s["wsup"].max() and s["wmax"] == (1.0 if (wsup64 > 0).any() else 0.0)
    assert s["eps"].dtype == np.float64 and np.array_equal(s["eps"], want)
    assert np.array_equal(s["first"], s["wsup"])                                 # both launches
    i, j = np.repeat(np.arange(n), k), g["index"].reshape(-1)
    flat = s["wsup"].reshape(-1)
    at = {(a, b): e for e, (a, b) in enumerate(zip(i.tolist(), j.tolist()))}
    back = np.array([at.get((b, a), -1) for a, b in zip(i.tolist(), j.tolist())])
    assert np.array_equal(back >= 0, g["mutual"].reshape(-1)) and (back >= 0).sum() > 0
    assert flat[back >= 0].tobytes() == flat[back[back >= 0]].tobytes()          # a mutual pair carries one value, bit for bit
    li, lj = s["label"][i], s["label"][j]
    cross = (li != lj) & (li >= 0) & (lj >= 0)
    assert cross.any()
    if tw == 1.0:
        assert (flat[cross] == 0).all() and np.isinf(s["eps"].reshape(-1)[cross]).all()
    else:
        assert (flat[cross] > 0).any() and not np.array_equal(s["eps"], g["eps"])


@pytest.mark.parametrize("name", list(G.SHAPES))
def test_five_epochs_on_the_supervised_schedule(name):
    """test_umap_gpu.test_five_epochs_in_a_row with the supervised spacings: the epoch kernel walks the new schedule."""
    import torch
    from cet_pick_amd import hipops as H
    s = _setup(name, "mod3", 0.5)
    g = s["g"]
    ti, rev_ptr, rev_edge, mutual, _ = g["dev"]
    a, b = U.find_ab(0.5)
    Y = G._positions(g)[0]
    y, y2 = G._dev(Y), torch.empty(g["N"], 2, device="cuda")
    ref, plain, bound, fired = Y, Y, 0.0, 0
    for n in range(248, 253):
        H.umap_epoch(y, y2, ti, rev_ptr, rev_edge, mutual, s["dev_eps"], n, N_EPOCHS, a, b, G.SEEDS[0])
        y, y2 = y2, y
        y64, n_terms, abs_terms = U.epoch_terms64(ref, g["inc"], s["eps"], n, N_EPOCHS, a, b, G.SEEDS[0])
        bound = bound + G._bound(y64, n_terms, abs_terms, n)
        ref = y64.astype(np.float32)
        plain = U.epoch64(plain, g["inc"], g["eps"], n, N_EPOCHS, a, b, G.SEEDS[0]).astype(np.float32)
        fired += int(n_terms.sum())
    got = y.cpu().numpy()
    ratio = (np.abs(got.astype(np.float64) - ref) / bound).max()
    print("%s: five epochs on the supervised spacings, %d terms, error max %.4f of the summed bound, %d of %d values equal; the plain "
          "schedule's chain differs in %d values" % (name, fired, ratio, (got == ref).sum(), got.size, (plain != ref).sum()))
    assert ratio <= 1.0 and fired > 0 and not np.array_equal(got, Y) and not np.array_equal(plain, ref)


def test_bad_arguments_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    s = _setup("smallest", "mod3", 0.5)
    ti, wsym, lab, rowmax = s["dev"]
    _, rev_ptr, rev_edge, _, _ = s["g"]["dev"]
    f = s["f"]
    for bad in (lab[:-1].contiguous(), lab.long(), lab.cpu(), lab.reshape(-1, 1)):
        with pytest.raises(L.HipExtensionError):
            H.umap_rowmax(ti, wsym, bad, rev_ptr, rev_edge, *f)
        with pytest.raises(L.HipExtensionError):
            H.umap_supervise(ti, wsym, bad, rowmax, *f, N_EPOCHS)
    with pytest.raises(L.HipExtensionError):
        H.umap_supervise(ti, wsym, lab, rowmax.float(), *f, N_EPOCHS)
    with pytest.raises(L.HipExtensionError):
        H.umap_supervise(ti, wsym, lab, rowmax[:-1].contiguous(), *f, N_EPOCHS)
    with pytest.raises(L.HipExtensionError):
        H.umap_rowmax(ti, wsym.double(), lab, rev_ptr, rev_edge, *f)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.umap_supervise(ti, wsym, lab, rowmax, *f, 0)
    with pytest.raises(L.HipExtensionError, match="unsupported"):                # N < k + 2: nothing is launched
        H.umap_rowmax(ti[:16].contiguous(), wsym[:16].contiguous(), lab[:16].contiguous(), rev_ptr[:17].contiguous(),
                      rev_edge[:16 * 15].contiguous(), *f)
    lib = L.lib()
    n, k = ti.shape
    null, st = L.ptr(None), L.stream()
    assert lib.mi_umap_rowmax(L.ptr(ti), L.ptr(wsym), null, L.ptr(rev_ptr), L.ptr(rev_edge), n, k, f[0], f[1], L.ptr(rowmax), st) == -1
    out = torch.empty_like(wsym)
    assert lib.mi_umap_supervise(L.ptr(ti), L.ptr(wsym), L.ptr(lab), null, n, k, f[0], f[1], null, N_EPOCHS, L.ptr(out), null, st) == -1
    wmax = torch.ones(1, device="cuda")                      # spacings asked for, and nowhere to write them
    assert lib.mi_umap_supervise(L.ptr(ti), L.ptr(wsym), L.ptr(lab), L.ptr(rowmax), n, k, f[0], f[1], L.ptr(wmax), N_EPOCHS, L.ptr(out),
                                 null, st) == -1


# end to end -------------------------------------------------------------------------------------------------------------------
BLOBS = dict(N=600, d=16, n_clusters=6, seed=600, sep=0.7)  # overlapping classes: see test_supervised_map_keeps_the_classes_together


def _graph(um, x):
    import torch
    xd = torch.from_numpy(x).cuda()
    return xd, um.graph(xd)


def test_fit_transform_with_labels_on_the_fixture(golden):
    from cet_pick_amd.utils.umap import UMAP
    z = golden("tsne_small.npz")
    x, label = z["x"], z["label"].astype(np.int64)
    um = UMAP(15, seed=42)
    xd, graph = _graph(um, x)
    Y = um.fit_transform(xd, graph=graph, y=label)
    assert Y.shape == (600, 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and um.n_epochs_ == 500
    assert um.supervised_ is True and um.far_dist_ == 5.0 and um.init_ == "random"
    again = UMAP(15, seed=42).fit_transform(xd, graph=graph, y=label)
    assert again.tobytes() == Y.tobytes(), "two fits differ"
    plain_um = UMAP(15, seed=42)
    plain = plain_um.fit_transform(xd, graph=graph)
    assert plain_um.supervised_ is False and plain_um.far_dist_ is None and not np.array_equal(plain, Y)
    agree, agree_plain = T.neighbour_agreement(Y, label), T.neighbour_agreement(plain, label)
    print("fixture: neighbour agreement %.4f supervised, %.4f plain" % (agree, agree_plain))
    assert agree >= agree_plain


def test_supervised_map_keeps_the_classes_together():
    """The fixture's six blobs are far apart and the plain map already has agreement 1.0 there, so the comparison is made on
    600 points in six blobs of unit spread whose centres are 0.7 N(0, 1) draws in 16 dimensions: the float64 arbiter gives the
    plain map 0.7717 and the supervised map 1.0000 on that set (umap_ref.fit64, umap_sup_ref.fit64, K = 15, seed 42)."""
    from cet_pick_amd.utils.umap import UMAP
    x, label = T.make_blobs(BLOBS["N"], BLOBS["d"], BLOBS["n_clusters"], seed=BLOBS["seed"], sep=BLOBS["sep"])
    um = UMAP(15, seed=42)
    xd, graph = _graph(um, x)
    Y = um.fit_transform(xd, graph=graph, y=label)
    plain = UMAP(15, seed=42).fit_transform(xd, graph=graph)
    agree, agree_plain = T.neighbour_agreement(Y, label), T.neighbour_agreement(plain, label)
    print("blobs at spread %.2f: neighbour agreement %.4f supervised, %.4f plain" % (BLOBS["sep"], agree, agree_plain))
    assert np.isfinite(Y).all() and agree >= agree_plain


@pytest.mark.parametrize("tw", [0.5, 1.0])
def test_spectral_start_from_the_supervised_graph(golden, tw):
    from cet_pick_amd.utils.umap import UMAP
    z = golden("tsne_small.npz")
    x, label = z["x"], z["label"].astype(np.int64)
    um = UMAP(15, seed=42, init="spectral", target_weight=tw)
    xd, graph = _graph(um, x)
    Y = um.fit_transform(xd, graph=graph, y=label)
    assert np.isfinite(Y).all() and um.init_ in ("spectral", "random") and um.supervised_ and um.far_dist_ == R.far_dist(tw)
    index, dist = graph[0][:, :14].contiguous(), graph[1][:, :14].contiguous()
    import torch
    _, _, _, eps, wsup = um.setup(index, dist, 500, with_wsym=True, label=torch.from_numpy(label.astype(np.int32)).cuda())
    comp = S.components(S.dense_w(index.cpu().numpy(), wsup.cpu().numpy(), eps.cpu().numpy()))
    n_comp = len(np.unique(comp))
    print("target_weight %g: start %s, %d graph components (arbiter %d), %d classes" % (tw, um.init_, um.n_components_, n_comp,
                                                                                       len(np.unique(label))))
    assert um.n_components_ == n_comp
    if tw == 1.0:
        assert n_comp >= len(np.unique(label))
        assert all(len(np.unique(label[comp == c])) == 1 for c in np.unique(comp))           # no component holds two classes


def test_plot_2d_writes_the_label_map(tmp_path):
    N, d = 300, 16
    x = T.make_blobs(N, d, 4, seed=9)[0]
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["tomo_a", "tomo_b"])[rs.randint(2, size=N)],
             coords=rs.randint(20, 400, size=(N, 3)).astype(np.int64))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for sub, extra in (("plain", []), ("labels", ["--label_map"])):
        out = tmp_path / sub
        r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path", str(out),
                            "--n_cluster", "0", "--k", "8", "--niter", "5", "--mode", "umap", "--num_neighbor", "15"] + extra, cwd=REPO,
                           env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[sub] = (out, r.stdout)
    out, log = outs["labels"]
    assert not (outs["plain"][0] / "embeddings_2d_labels.npz").exists() and "supervised" not in outs["plain"][1]
    assert (out / "embeddings_2d.npz").read_bytes() == (outs["plain"][0] / "embeddings_2d.npz").read_bytes()
    assert (out / "all_colors.npy").read_bytes() == (outs["plain"][0] / "all_colors.npy").read_bytes()
    e = np.load(out / "embeddings_2d_labels.npz")
    assert sorted(e.files) == LISTED
    assert np.array_equal(e["label"], np.load(out / "kmeans_labels.npz")["label"]) and e["label"].dtype == np.int32
    assert e["y"].shape == (N, 2) and e["y"].dtype == np.float32 and np.isfinite(e["y"]).all()
    assert np.array_equal(e["y01"].min(0), [0, 0]) and np.array_equal(e["y01"].max(0), [1, 1])
    assert (int(e["n_neighbors"]), int(e["seed"]), int(e["n_epochs"]), float(e["min_dist"])) == (15, 42, 500, 0.5)
    assert (float(e["target_weight"]), float(e["far_dist"])) == (0.5, 5.0)
    assert not np.array_equal(e["y"], np.load(out / "embeddings_2d.npz")["y"])
    assert log.count("label-supervised UMAP map of 300 picks in %d classes, n_neighbors 15" % len(np.unique(e["label"]))) == 1
