"""csrc/umap.hip and utils/umap.py on the MI355X against the float64 arbiter tests/umap_ref.py.

K below is UMAP's n_neighbors, which counts the point itself: the tables have K - 1 columns.  The band of the epoch checks is
umap_ref.band64(terms) = (terms + 64) 2^-53 of the sum of the magnitudes of a vertex's terms, times alpha, plus the one fp32
rounding of the stored position."""
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_ref
import tsne_ref as T
import umap_ref as U
import vis3d_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EPOCHS = 500
SHAPES = {"smallest": (17, 16), "hub": (300, 14), "wide": (150, 71)}      # N, K; wide: 70 columns, a full batch of 64 lanes and 6
SEEDS = (42, (7 << 32) | 5)                                 # the second one reaches the key's high word
_cache = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _planted_rows(dist2):
    """rows 5..8 of a table of squared distances: all zero; three leading zeros (duplicate picks); all equal; one far outlier"""
    k = dist2.shape[1]
    dist2 = dist2.copy()
    dist2[5] = 0.0
    dist2[6, :3] = 0.0
    dist2[7] = 2.25
    dist2[8] = np.linspace(1.0, 2.0, k) * 1e8
    return dist2


def _setup(name):
    """The graph of a shape, its device tables and what the device made of them, once per shape: index (N, K - 1) int64, dist2,
    (rho, sigma, w), (wsym, mutual, eps), the device tensors the epoch takes, and the arbiter's incident lists of the device's
    `mutual`."""
    if name not in _cache:
        import torch
        from cet_pick_amd import hipops as H
        from cet_pick_amd.utils.tsne import reverse_graph
        N, K = SHAPES[name]
        # wide: one blob, so that the columns past the first 64 hold live edges (with three, they all lead to another blob
        # and are pruned)
        x = T.make_blobs(N, 12, 1 if name == "wide" else 3, seed=N)[0]
        if name == "hub":
            x[N - 1] += 100.0                                # nobody's neighbour: a vertex without reverse edges
        index, dist2 = H.knn_search(_dev(x), _dev(x), K, metric="l2", exclude_self=True)
        index, dist2 = index[:, :K - 1].cpu().numpy().astype(np.int64), dist2[:, :K - 1].cpu().numpy()
        if name == "hub":
            dist2 = _planted_rows(dist2)
            for r in range(20, 120):                         # vertex 0 becomes a hub: more reverse edges than a wave has lanes
                if 0 not in index[r]:
                    index[r, -1] = 0
            assert (index == 0).sum() > 64 and (index == N - 1).sum() == 0
            assert all(len(set(row)) == K - 1 and i not in row for i, row in enumerate(index.tolist()))
        d = U.distances(dist2)
        mean_all = d.sum() / (N * K)
        ti, td = _dev(index.astype(np.int32)), _dev(dist2)
        rho, sigma, w = H.umap_smooth_knn(td, mean_all)
        rev_ptr, rev_edge = reverse_graph(ti)
        out = H.umap_union(ti, w, rev_ptr, rev_edge, N_EPOCHS)
        first = [t.cpu().numpy().copy() for t in out[:2]]
        wmax = out[0].max().reshape(1)
        wsym, mutual, eps = H.umap_union(ti, w, rev_ptr, rev_edge, N_EPOCHS, wmax=wmax, out=out)
        torch.cuda.synchronize()
        g = dict(N=N, K=K, index=index, dist2=dist2, mean_all=mean_all, rho=rho.cpu().numpy(), sigma=sigma.cpu().numpy(),
                 w=w.cpu().numpy(), wsym=wsym.cpu().numpy(), mutual=mutual.cpu().numpy().astype(bool), eps=eps.cpu().numpy(),
                 first=first, wmax=float(wmax.item()), dev=(ti, rev_ptr, rev_edge, mutual, eps))
        g["inc"] = U.incident(index, g["mutual"])
        _cache[name] = g
    return _cache[name]


# smooth distances -------------------------------------------------------------------------------------------------------------
def _check_smooth(dist2, K, what):
    from cet_pick_amd import hipops as H
    N = len(dist2)
    mean_all = U.distances(dist2).sum() / (N * K)
    rho, sigma, w = (t.cpu().numpy() for t in H.umap_smooth_knn(_dev(dist2), mean_all))
    r64, s64, w64 = U.smooth64(dist2, mean_all)
    assert rho.dtype == sigma.dtype == w.dtype == np.float32 and w.shape == dist2.shape
    e_s = (np.abs(sigma - s64) / s64).max()
    e_w = np.abs(w - w64).max() / ((K + 8) * 2.0 ** -24)
    print("%s N=%d K=%d: rho exact %s, sigma relative error max %.3e (bound 1e-5), |w - w64| max %.4f of (K + 8) 2^-24, sigma %.3e .. "
          "%.3e" % (what, N, K, np.array_equal(rho, r64), e_s, e_w, sigma.min(), sigma.max()))
    assert np.array_equal(rho.astype(np.float64), r64)
    assert np.isfinite(sigma).all() and e_s <= 1e-5
    assert np.isfinite(w).all() and e_w <= 1.0
    return rho, sigma, w


def test_smooth_knn_on_a_full_table():
    """N = K + 1: every other point is a neighbour."""
    g = _setup("smallest")
    assert g["dist2"].shape == (17, 15)
    _check_smooth(g["dist2"], 16, "smallest")


def test_smooth_knn_with_both_lane_halves():
    """K - 1 = 126 columns: lane c holds columns c and c + 64."""
    from cet_pick_amd import hipops as H
    x = _dev(T.make_blobs(200, 12, 3, seed=200)[0])
    dist2 = H.knn_search(x, x, 127, metric="l2", exclude_self=True)[1][:, :126].cpu().numpy()
    _check_smooth(dist2, 127, "wide")


def test_smooth_knn_with_planted_rows():
    g = _setup("hub")
    rho, sigma, w = _check_smooth(g["dist2"], 14, "planted")
    d = U.distances(g["dist2"])
    assert rho[5] == 0 and (w[5] == 1).all() and sigma[5] == np.float32(1e-3 * g["mean_all"])      # all zero: the table's mean
    assert rho[6] == d[6, 3] > 0 and (w[6, :4] == 1).all() and (w[6, 4:] < 1).all()                # rho skips the zeros
    assert rho[7] == 1.5 and (w[7] == 1).all() and sigma[7] == np.float32(1e-3 * (19.5 / 14))    # all equal: the row's mean
    assert rho[8] == 1e4 and w[8, 0] == 1 and w[8, -1] > 0 and sigma[8] > 100                      # the outlier's own scale


# union ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_union_matches_float64(name):
    g = _setup(name)
    N, k = g["index"].shape
    wsym64, mutual64, _, _ = U.union64(g["index"], g["w"], N_EPOCHS)
    assert np.array_equal(g["mutual"], mutual64) and 0 < mutual64.sum() < N * k
    e_w = np.abs(g["wsym"] - wsym64).max() / (4 * 2.0 ** -24)
    want = U.spacing64(g["wsym"], g["wmax"], N_EPOCHS)          # the double formula on the device's own fp32 wsym and wmax
    print("%s: |wsym - wsym64| max %.4f of 4 2^-24, wmax %.8g, %d of %d edges pruned, eps equal %s"
          % (name, e_w, g["wmax"], np.isinf(want).sum(), N * k, np.array_equal(g["eps"], want)))
    assert e_w <= 1.0 and g["wmax"] == g["wsym"].max()
    assert g["eps"].dtype == np.float64 and np.array_equal(g["eps"], want)
    assert np.array_equal(g["first"][0], g["wsym"]) and np.array_equal(g["first"][1].astype(bool), g["mutual"])     # both launches
    if name == "hub":
        ptr, _ = U.reverse_lists(g["index"])
        assert ptr[1] - ptr[0] > 64 and ptr[N] - ptr[N - 1] == 0 and np.isinf(want).sum() > 0
    if name == "wide":                                       # the lanes' second pass over the columns meets live edges
        assert k == 70 and np.isfinite(want[:, 64:]).any()


# epoch ------------------------------------------------------------------------------------------------------------------------
def _positions(g):
    """umap-learn's start with coincident points planted: the two ends of an edge that fires every epoch, and a group that
    negatives drawn by its own members fall into."""
    N = g["N"]
    Y = U.start(N, 3)
    i = int(np.argmax((g["eps"][:, 0] == 1.0) & (np.arange(N) > 12)))
    group = [1, 2, 5, 9] if N < 100 else list(range(130, min(160, N)))
    Y[group] = Y[group[0]]
    Y[g["index"][i, 0]] = Y[i]
    return Y, i, group


def _epoch(g, Y, n, seed, a, b):
    import torch
    from cet_pick_amd import hipops as H
    yin = _dev(Y)
    out = H.umap_epoch(yin, torch.empty_like(yin), *g["dev"], n, N_EPOCHS, a, b, seed)
    return out.cpu().numpy()


def _bound(y64, n_terms, abs_terms, n):
    alpha = 1.0 - (n - 1.0) / N_EPOCHS
    return 2.0 ** -24 * np.abs(y64) + alpha * (U.band64(n_terms)[:, None] * abs_terms)


@pytest.mark.parametrize("name", list(SHAPES))
def test_epoch_matches_float64(name):
    g = _setup(name)
    a, b = U.find_ab(0.5)
    Y, i_edge, group = _positions(g)
    vert, slot, other, edge = g["inc"]
    hits = 0
    for n in (1, 2, 250, 500):
        outs = []
        for seed in SEEDS:
            got = _epoch(g, Y, n, seed, a, b)
            y64, n_terms, abs_terms = U.epoch_terms64(Y, g["inc"], g["eps"], n, N_EPOCHS, a, b, seed)
            ratio = (np.abs(got - y64) / _bound(y64, n_terms, abs_terms, n)).max()
            f = U.fires(n, g["eps"].reshape(-1)[edge])
            neg = U.negatives(vert[f], slot[f], n, g["N"], seed)
            same = (Y[neg] == Y[vert[f]][:, None, :]).all(2) & (neg != vert[f][:, None])
            hits += int(same.sum())
            print("%s N=%d K=%d epoch %d seed %d: %d firings, terms per vertex up to %d, error max %.4f of its bound, %d negatives on "
                  "a coincident point" % (name, g["N"], g["K"], n, seed, f.sum(), n_terms.max(), ratio, same.sum()))
            assert got.dtype == np.float32 and np.isfinite(got).all() and ratio <= 1.0
            assert f[(vert == i_edge) & (slot == 0)].all()                        # the planted d2 = 0 edge fires
            assert _epoch(g, Y, n, seed, a, b).tobytes() == got.tobytes(), "two launches differ"
            outs.append(got)
        assert not np.array_equal(outs[0], outs[1]), "the seed does not reach the negatives"
        assert f.sum() > 0
    assert hits > 0
    if name == "hub":                                        # the hub's reverse list runs over more than one pass of the lanes
        assert (vert == 0).sum() > 64 + g["K"] - 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_five_epochs_in_a_row(name):
    """Five epochs on the device against five of the arbiter from the same start; the arbiter's positions are rounded to fp32
    after every epoch, as the device stores them, and the band is the sum of the five epochs' bands."""
    import torch
    from cet_pick_amd import hipops as H
    g = _setup(name)
    a, b = U.find_ab(0.5)
    Y = _positions(g)[0]
    y, y2 = _dev(Y), torch.empty(g["N"], 2, device="cuda")
    ref, bound = Y, 0.0
    for n in range(248, 253):
        H.umap_epoch(y, y2, *g["dev"], n, N_EPOCHS, a, b, SEEDS[0])
        y, y2 = y2, y
        y64, n_terms, abs_terms = U.epoch_terms64(ref, g["inc"], g["eps"], n, N_EPOCHS, a, b, SEEDS[0])
        bound = bound + _bound(y64, n_terms, abs_terms, n)
        ref = y64.astype(np.float32)
    got = y.cpu().numpy()
    ratio = (np.abs(got.astype(np.float64) - ref) / bound).max()
    print("%s: five epochs, error max %.4f of the summed bound, %d of %d values equal" % (name, ratio, (got == ref).sum(), got.size))
    assert ratio <= 1.0 and not np.array_equal(got, Y)


def test_unsupported_arguments_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    g = _setup("smallest")
    y = torch.zeros(17, 2, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.umap_smooth_knn(torch.zeros(200, 128, device="cuda"), 1.0)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.umap_smooth_knn(torch.zeros(16, 15, device="cuda"), 1.0)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.umap_epoch(y, torch.empty_like(y), *g["dev"], 501, N_EPOCHS, 1.0, 1.0, 0)
    with pytest.raises(L.HipExtensionError, match="alias"):
        H.umap_epoch(y, y, *g["dev"], 1, N_EPOCHS, 1.0, 1.0, 0)
    with pytest.raises(L.HipExtensionError):
        H.umap_epoch(y.cpu(), torch.empty_like(y), *g["dev"], 1, N_EPOCHS, 1.0, 1.0, 0)


# end to end -------------------------------------------------------------------------------------------------------------------
def test_fit_transform_on_the_fixture(golden):
    from sklearn.manifold import trustworthiness
    from cet_pick_amd.utils.umap import UMAP
    z, rec = golden("tsne_small.npz"), golden("umap_small.npz")
    x, label = z["x"], z["label"].astype(np.int64)
    um = UMAP(int(rec["n_neighbors"]), min_dist=float(rec["min_dist"]), seed=42)
    Y = um.fit_transform(x)
    assert Y.shape == (600, 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and um.n_epochs_ == 500
    assert np.abs(np.array([um.a_, um.b_]) / rec["ab"] - 1).max() <= 1e-6
    again = UMAP(int(rec["n_neighbors"]), min_dist=float(rec["min_dist"]), seed=42).fit_transform(x)
    assert again.tobytes() == Y.tobytes(), "two fits differ"
    agree, trust = T.neighbour_agreement(Y, label), float(trustworthiness(x, Y, n_neighbors=5))
    print("agreement %.4f (the sequential loop's %s, the synchronous arbiter's %.4f), trustworthiness %.4f (sequential %s, margin "
          "%.4f, synchronous arbiter %.4f), extent %s" % (agree, np.round(rec["seq_agree"], 4).tolist(), float(rec["sync_agree"]), trust,
                                                         np.round(rec["seq_trust"], 4).tolist(), float(rec["trust_margin"]),
                                                         float(rec["sync_trust"]), np.round(np.ptp(Y, axis=0), 2).tolist()))
    assert agree >= rec["seq_agree"].min()
    assert trust >= rec["seq_trust"].min() - float(rec["trust_margin"])


def test_plot_2d_writes_the_umap_map(tmp_path):
    N, d = 300, 16
    x = T.make_blobs(N, d, 4, seed=9)[0]
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["tomo_a", "tomo_b"])[rs.randint(2, size=N)],
             coords=rs.randint(20, 400, size=(N, 3)).astype(np.int64))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "map"
    r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path", str(out),
                        "--n_cluster", "0", "--k", "8", "--niter", "5", "--mode", "umap", "--num_neighbor", "15"], cwd=REPO, env=env,
                       timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    e = np.load(out / "embeddings_2d.npz")
    assert sorted(e.files) == ["a", "b", "min_dist", "n_epochs", "n_neighbors", "seed", "y", "y01"]
    assert e["y"].shape == (N, 2) and e["y"].dtype == np.float32 and np.isfinite(e["y"]).all()
    assert np.array_equal(e["y01"].min(0), [0, 0]) and np.array_equal(e["y01"].max(0), [1, 1])
    assert (int(e["n_neighbors"]), int(e["seed"]), int(e["n_epochs"]), float(e["min_dist"])) == (15, 42, 500, 0.5)
    assert "UMAP map of 300 picks, n_neighbors 15" in r.stdout
    colours = np.load(out / "all_colors.npy")
    assert colours.shape == (N, 3) and colours.dtype == np.uint8
    assert np.array_equal(colours, vis3d_ref.sample_colours(e["y01"], vis3d_ref.default_colormap()))
    g = np.load(out / "knn_graph.npz")
    assert g["index"].shape == (N, 15)
    knn_ref.check_knn(x, x, 15, "l2", g["index"], g["dist"], True, what="plot_2d --mode umap")
