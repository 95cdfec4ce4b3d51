"""csrc/spectral.hip and utils/spectral.py on the MI355X against the float64 arbiter tests/spectral_ref.py.

Bounds.  A sum of n terms in double: (n + 64) 2^-53 of the sum of the terms' magnitudes (umap_ref.band64).  An eigenvector whose
residual is <= tol and whose eigenvalue is `gap` from the rest of the spectrum: |v - v_ref|_2 <= 2 tol / gap (Davis-Kahan; the gap
is the float64 reference's, recorded in the fixture or computed by the arbiter).  K is UMAP's n_neighbors; the tables have K - 1
columns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spectral_ref as R
import tsne_ref as T
import umap_ref as U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
_cache = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _upload(index, wsym, eps, mutual):
    """The six device tables (index, wsym, eps, mutual, rev_ptr, rev_edge) of host tables."""
    from cet_pick_amd.utils.tsne import reverse_graph
    ti = _dev(np.asarray(index, np.int32))
    rev_ptr, rev_edge = reverse_graph(ti)
    return (ti, _dev(np.asarray(wsym, np.float32)), _dev(np.asarray(eps, np.float64)), _dev(np.asarray(mutual, np.uint8)), rev_ptr, rev_edge)


def _weight(i, j):
    """A symmetric fp32 weight in (0, 1] for a hand-made edge."""
    return np.float32(0.1 + ((i * j + i + j) % 17) / 20.0)


def _hand_made(n, k, edges):
    """Tables (index, wsym, eps, mutual) of n vertices with k columns whose LIVE directed edges are `edges`; the other columns
    hold edges with eps = +inf to the next vertices that the row does not name yet.  mutual = 1 where the opposite edge is live."""
    live = set(edges)
    rows = [[j for (i, j) in edges if i == v] for v in range(n)]
    index, eps, mutual, wsym = np.zeros((n, k), np.int64), np.full((n, k), np.inf), np.zeros((n, k), np.uint8), np.zeros((n, k), np.float32)
    for v, row in enumerate(rows):
        assert len(row) <= k and len(set(row)) == len(row) and v not in row
        fill = [u % n for u in range(v + 1, v + n) if u % n not in row][:k - len(row)]
        for c, j in enumerate(row + fill):
            index[v, c] = j
            if c < len(row):
                eps[v, c], mutual[v, c], wsym[v, c] = 1.0 + (v + j) % 3, (j, v) in live, _weight(v, j)
            else:
                wsym[v, c] = 0.5                              # a pruned edge keeps its weight; only eps says it is out
    return index, wsym, eps, mutual


def _path(ids):
    return [(ids[t], ids[t + 1]) for t in range(len(ids) - 1)]


def _component_graphs():
    rs = np.random.RandomState(5)
    zig = [v for t in range(100) for v in (t, 199 - t)]                                # 0, 199, 1, 198, ...: ids against the path
    hub = [(v, 50) for v in range(100) if v != 50] + _path(list(range(100, 130))) + _path(list(range(130, 150))) + [(149, 130)]
    g65 = _path(list(rs.permutation(40))) + _path(list(40 + rs.permutation(25)))
    g70 = _path(list(rs.permutation(64))) + _path(list(64 + rs.permutation(6)))
    lone = _path([0, 1, 2, 3]) + [(2, 1)] + _path([5, 6, 7]) + [(7, 4)]                 # 4 joins 5..7 by a reverse edge alone
    return {"zigzag path": (200, 2, _path(zig)), "random path": (200, 2, _path(list(rs.permutation(200)))), "hub": (150, 3, hub),
            "N=65": (65, 2, g65), "N=70": (70, 2, g70), "lone reverse and pruned": (9, 3, lone)}


@pytest.mark.parametrize("name", list(_component_graphs()))
def test_components_match_scipy(name):
    from cet_pick_amd import hipops as H
    n, k, edges = _component_graphs()[name]
    index, wsym, eps, mutual = _hand_made(n, k, edges)
    g = _upload(index, wsym, eps, mutual)
    label, sweeps = H.graph_components(g[0], g[2], g[3], g[4], g[5])
    want = R.components(R.dense_w(index, wsym, eps))
    again, sweeps2 = H.graph_components(g[0], g[2], g[3], g[4], g[5])
    print("%s: N=%d, %d components, %d sweeps" % (name, n, len(np.unique(want)), sweeps))
    assert label.dtype.is_floating_point is False and np.array_equal(label.cpu().numpy(), want)
    assert np.array_equal(again.cpu().numpy(), want) and sweeps2 == sweeps
    if name == "hub":
        assert (index[np.isfinite(eps)] == 50).sum() > 64 and np.array_equal(np.unique(want), [0, 100, 130])
    if name == "lone reverse and pruned":                    # 8 is reached by pruned edges only; 4 by the lone edge 7 -> 4
        assert want.tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 8] and (index[np.isinf(eps)] == 8).any()
    if "path" in name:
        assert (want == 0).all() and sweeps >= 3


def _search_graph(key, x, K):
    """The search and union of x on the device, once per key: the device tables, and the arbiter's dense W of them."""
    if key not in _cache:
        from cet_pick_amd import hipops as H
        from cet_pick_amd.utils.umap import UMAP
        index, dist = H.knn_search(_dev(x), _dev(x), K, metric="l2", exclude_self=True)
        index, dist = index[:, :K - 1].contiguous(), dist[:, :K - 1].contiguous()
        rev_ptr, rev_edge, mutual, eps, wsym = UMAP(K).setup(index, dist, 500, with_wsym=True)
        g = (index, wsym, eps, mutual, rev_ptr, rev_edge)
        W = R.dense_w(index.cpu().numpy(), wsym.cpu().numpy(), eps.cpu().numpy())
        assert np.array_equal(W, W.T) and (R.components(W) == 0).all()
        _cache[key] = dict(x=x, K=K, g=g, W=W, graph=(index, dist))
    return _cache[key]


def _strip_graph(golden, which):
    """A strip of the fixture."""
    n, K, seed = (int(v) for v in golden("spectral_small.npz")[which])
    return _search_graph(which, R.strip(n, seed)[0], K)


def _wide_graph():
    """150 points in one blob with 70 columns: the lanes take the forward edges in a full batch of 64 and one of 6."""
    return _search_graph("wide", T.make_blobs(150, 12, 1, seed=150)[0], 71)


def _hub_graph():
    if "hub" not in _cache:
        n, k, edges = _component_graphs()["hub"]
        t = _hand_made(n, k, edges)
        _cache["hub"] = dict(g=_upload(*t), W=R.dense_w(t[0], t[1], t[2]))
    return _cache["hub"]


@pytest.mark.parametrize("which", ["small", "strip", "hub", "wide"])
def test_degree_and_spmv_match_float64(golden, which):
    import torch
    from cet_pick_amd import hipops as H
    s = _hub_graph() if which == "hub" else _wide_graph() if which == "wide" else _strip_graph(golden, which)
    g, W = s["g"], s["W"]
    n = len(W)
    deg, dis = H.spectral_degree(*g)
    count = (W > 0).sum(1)
    A, deg64 = R.normalised(W)
    e_deg = (np.abs(deg.cpu().numpy() - deg64) / np.maximum(U.band64(count) * deg64, 1e-300)).max()
    dis64 = np.where(deg64 > 0, 1.0 / np.sqrt(np.maximum(deg64, 1e-300)), 0.0)
    e_dis = (np.abs(dis.cpu().numpy() - dis64) / np.maximum(U.band64(count) * dis64, 1e-300)).max()
    assert e_deg <= 1.0 and e_dis <= 1.0 and H.spectral_degree(*g)[0].cpu().numpy().tobytes() == deg.cpu().numpy().tobytes()
    x = np.random.RandomState(n).standard_normal(n)
    for row0, nrows in ((0, n), (37, n - 50)):
        sl = slice(row0, row0 + nrows)
        y = H.spectral_spmv(*g, dis, _dev(x[sl]), row0=row0)
        got = y.cpu().numpy()
        want = A[sl, sl] @ x[sl]
        bound = U.band64((W[sl, sl] > 0).sum(1)) * (np.abs(A[sl, sl]) @ np.abs(x[sl]))
        ratio = (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
        print("%s rows %d..%d: degree error max %.4f of its bound, product error max %.4f of its bound" % (which, row0, row0 + nrows, e_deg, ratio))
        assert got.dtype == np.float64 and np.isfinite(got).all() and ratio <= 1.0 and np.abs(want).max() > 0
        assert H.spectral_spmv(*g, dis, _dev(x[sl]), torch.empty_like(y), row0=row0).cpu().numpy().tobytes() == got.tobytes()
    if which == "hub":
        assert count.max() > 64 and (count == 1).any()
    if which == "wide":
        assert g[0].shape == (150, 70) and count.max() > 64
        assert np.isfinite(g[2][:, 64:].cpu().numpy()).any()     # the lanes' second pass over the columns meets live edges


@pytest.mark.parametrize("n,m", [(n, m) for n in (96, 333, 600) for m in (1, 3, 64, 65, 130) if m <= n])
def test_orth_matches_float64(n, m):
    """m orthonormal vectors of length n (there are no 130 of length 96)."""
    from cet_pick_amd import hipops as H
    rs = np.random.RandomState(1000 * n + m)
    Q = np.ascontiguousarray(np.linalg.qr(rs.standard_normal((n, m)))[0].T)
    w = rs.standard_normal(n) + 3.0 * Q[0]
    tQ, tw = _dev(Q), _dev(w)
    c = H.spectral_orth(tQ, tw).cpu().numpy()
    w1 = tw.cpu().numpy()
    ratio = (np.abs(c - Q @ w) / (U.band64(n) * (np.abs(Q) @ np.abs(w)))).max()
    e_up = (np.abs(w1 - (w - Q.T @ c)) / (U.band64(m) * (np.abs(w) + np.abs(Q.T) @ np.abs(c)))).max()
    tw2 = _dev(w)
    assert H.spectral_orth(tQ, tw2).cpu().numpy().tobytes() == c.tobytes() and tw2.cpu().numpy().tobytes() == w1.tobytes()
    assert H.spectral_dots(tQ, _dev(w)).cpu().numpy().tobytes() == c.tobytes()
    H.spectral_orth(tQ, tw)
    left = np.abs(Q @ tw.cpu().numpy()).max() / (64 * 2.0 ** -53 * np.linalg.norm(w))
    print("m=%d n=%d: coefficient error max %.4f of its bound, update error max %.4f of its bound, |Q^T w| after two passes %.4f of "
          "64 2^-53 |w|" % (m, n, ratio, e_up, left))
    assert ratio <= 1.0 and e_up <= 1.0 and left <= 1.0
    s = rs.standard_normal(m)
    y = H.spectral_combine(tQ, _dev(s), _dev(np.full(n, np.nan)))                     # beta = 0: w is not read
    assert (np.abs(y.cpu().numpy() + Q.T @ s) <= U.band64(m) * (np.abs(Q.T) @ np.abs(s))).all()


def test_bad_sizes_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    g = _hub_graph()["g"]
    dis = H.spectral_degree(*g)[1]
    x = torch.zeros(100, dtype=torch.float64, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.spectral_spmv(*g, dis, x, row0=51)                                          # 51 + 100 > 150 rows
    with pytest.raises(L.HipExtensionError, match="alias"):
        H.spectral_spmv(*g, dis, x, x)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.spectral_dots(torch.zeros(4097, 8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda"))
    Q = torch.zeros(3, 100, dtype=torch.float64, device="cuda")
    with pytest.raises(L.HipExtensionError, match="bad argument"):
        H.spectral_orth(Q, Q[1])
    with pytest.raises(L.HipExtensionError):
        H.spectral_dots(Q.float(), x)
    assert L.lib().mi_spectral_workspace_bytes(0, 100) == 0 and L.lib().mi_spectral_workspace_bytes(3, 5000) == 3 * 3 * 8


@pytest.mark.parametrize("which", ["small", "strip"])
def test_solver_matches_the_dense_solve(golden, which):
    from cet_pick_amd.utils.spectral import spectral_layout
    z = golden("spectral_small.npz")
    s = _strip_graph(golden, which)
    n = len(s["W"])
    lam, v_ref, gap_here = R.eigenpairs(s["W"], 2)
    gap = z[which + "_gap"]
    assert np.abs(lam[:7] - z[which + "_lam"]).max() <= 1e-4 and np.abs(gap_here / gap - 1).max() <= 1e-2     # the device's graph
    deg64 = R.normalised(s["W"])[1]
    q0 = np.sqrt(deg64) / np.linalg.norm(np.sqrt(deg64))
    runs = {}
    for what, kw in (("default basis", {}), ("basis 8", dict(max_basis=8))):
        Y, info = spectral_layout(*s["g"], dim=2, seed=42, tol=TOL, **kw)
        v = Y.cpu().numpy()
        e_lam, e_v = np.abs(info["eigenvalues"] - lam[1:3]), np.linalg.norm(v - v_ref, axis=0)
        cross = max(np.abs(v.T @ q0).max(), abs(v[:, 0] @ v[:, 1]), np.abs((v * v).sum(0) - 1).max())
        print("%s N=%d, %s: %d vectors, %d steps, %d restarts, residuals %s, |lam - ref| %s, |v - ref| %s of bounds %s, products %.2e"
              % (which, n, what, info["basis"], info["steps"], info["restarts"], info["residuals"], e_lam, e_v, 2 * TOL / gap, cross))
        assert info["converged"] and info["n_components"] == 1 and Y.dtype.is_floating_point and v.dtype == np.float64
        assert info["residuals"].max() <= TOL and e_lam.max() <= TOL and (e_v <= 2 * TOL / gap).all() and cross <= 1e-12
        for a in range(2):
            assert v[np.argmax(np.abs(v[:, a])), a] > 0
        again = spectral_layout(*s["g"], dim=2, seed=42, tol=TOL, **kw)[0].cpu().numpy()
        assert again.tobytes() == v.tobytes(), "two solves differ"
        runs[what] = info
    assert runs["basis 8"]["basis"] == 8 and runs["basis 8"]["restarts"] >= 2 and runs["default basis"]["basis"] == (10 if n == 96 else 25)


def _pieces(sizes, places, k, seed):
    """Separate pieces (tight strips of `sizes` points around `places` in the first two data coordinates; a size below 4 is a
    complete graph), each with its own k-column graph, under one random numbering of all vertices."""
    rs = np.random.RandomState(seed)
    n = sum(sizes)
    number = rs.permutation(n)                                # piece-local vertex at + i is vertex number[at + i]
    index, eps = np.zeros((n, k), np.int64), np.full((n, k), np.inf)
    wsym, mutual, x = np.full((n, k), 0.5, np.float32), np.zeros((n, k), np.uint8), np.zeros((n, 32), np.float32)
    at = 0
    for p, (m, place) in enumerate(zip(sizes, places)):
        xp = 0.02 * R.strip(m, seed + p)[0]
        xp[:, :2] += np.asarray(place, np.float32)
        mine = number[at:at + m]
        x[mine] = xp
        if m > k + 1:
            ip, d2 = R.knn(xp, k)
            wp, mp, ep = R.graph_tables(ip, d2, 500)
            index[mine], wsym[mine], mutual[mine], eps[mine] = mine[ip], wp, mp, ep
        else:
            for i in range(m):
                others = [mine[j] for j in range(m) if j != i]
                fill = [v for v in range(n) if v not in mine][:k - len(others)]
                index[mine[i]] = others + fill
                eps[mine[i], :len(others)], wsym[mine[i], :len(others)], mutual[mine[i], :len(others)] = 1.0, 1.0, 1
        at += m
    return index, wsym, eps, mutual, x


CASES = {"three": ([48, 40, 36], [(0, 0), (50, 0), (0, 50)]),
         "seven": ([30, 34, 3, 38, 42, 31, 36], [(0, 0), (1.1, 0.2), (0.3, 1.3), (2.0, 1.2), (-0.9, 0.8), (1.2, -1.1), (-0.4, -1.2)])}


@pytest.mark.parametrize("case", list(CASES))
def test_several_components(case):
    from cet_pick_amd.utils.spectral import spectral_layout
    sizes, places = CASES[case]
    index, wsym, eps, mutual, x = _pieces(sizes, places, 7, seed=11)
    W = R.dense_w(index, wsym, eps)
    Yr, ref = R.layout(W, 2, seed=42, x=x)
    Y, info = spectral_layout(*_upload(index, wsym, eps, mutual), dim=2, seed=42, tol=TOL, x=_dev(x))
    Y = Y.cpu().numpy()
    c = len(sizes)
    assert info["converged"] and info["n_components"] == ref["n_components"] == c and np.array_equal(info["labels"], ref["labels"])
    assert sorted(info["sizes"].tolist()) == sorted(sizes) and np.array_equal(info["sizes"], ref["sizes"])
    if c <= 4:
        assert np.array_equal(info["centres"], ref["centres"]) and np.array_equal(info["centres"], [[1, 0], [0, 1], [-1, 0]])
        centre_err = 0.0
    else:
        members = [np.nonzero(ref["labels"] == l)[0] for l in np.unique(ref["labels"])]
        lam_c = R.eigh_centres(np.stack([x[m].astype(np.float64).mean(0) for m in members]), 2)[1]
        assert min(lam_c[1] - lam_c[0], lam_c[2] - lam_c[1], lam_c[3] - lam_c[2]) >= 1e-3      # the centres' own eigenvectors are distinct
        centre_err = 1e-9                                     # two float64 eigh of matrices one rounding apart, gaps >= 1e-3
        assert np.abs(info["centres"] - ref["centres"]).max() <= centre_err
    assert np.abs(info["data_range"] - ref["data_range"]).max() <= 2 * centre_err
    for a, l in enumerate(np.unique(ref["labels"])):
        m = np.nonzero(ref["labels"] == l)[0]
        box = np.abs(Y[m] - info["centres"][a]).max() / info["data_range"][a]
        assert box <= 1 + 1e-12, "component %d leaves its box" % a
        if len(m) < 4:
            assert np.abs(Y[m] - Yr[m]).max() <= 3 * centre_err
            continue
        gap, s_ref = ref["gap"][a], ref["scale"][a]
        vmax = np.abs(Yr[m] - ref["centres"][a]).max() / s_ref
        e_scale = abs(info["scale"][a] / s_ref - 1)
        e_y = np.linalg.norm(Y[m] - Yr[m], axis=0)
        bound = s_ref * (2 * TOL / gap + (2 * TOL / gap.min()) / vmax) + 3 * centre_err * np.sqrt(len(m))
        print("%s component %d (%d vertices): scale error %.2e, |Y - ref| %s of bounds %s, box %.6f" % (case, a, len(m), e_scale, e_y, bound, box))
        assert e_scale <= (2 * TOL / gap.min()) / vmax + 2 * centre_err / ref["data_range"][a] and (e_y <= bound).all()
    again = spectral_layout(*_upload(index, wsym, eps, mutual), dim=2, seed=42, tol=TOL, x=_dev(x))[0].cpu().numpy()
    assert again.tobytes() == Y.tobytes()


def test_whole_fit_from_the_spectral_start(golden, capsys):
    from sklearn.manifold import trustworthiness
    from cet_pick_amd.utils.umap import UMAP
    z, rec = golden("spectral_small.npz"), golden("umap_small.npz")
    s = _strip_graph(golden, "strip")
    x = s["x"]
    um = UMAP(s["K"], min_dist=float(z["min_dist"]), seed=int(z["seed"]), init="spectral")
    Y = um.fit_transform(x)
    assert Y.shape == (600, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
    assert um.init_ == "spectral" and um.n_components_ == 1 and um.n_epochs_ == 500
    assert np.abs(um.eigenvalues_ - z["strip_lam"][1:3]).max() <= 1e-4
    again = UMAP(s["K"], min_dist=float(z["min_dist"]), seed=int(z["seed"]), init="spectral").fit_transform(x)
    assert again.tobytes() == Y.tobytes(), "two fits differ"
    capsys.readouterr()
    rand = UMAP(s["K"], min_dist=float(z["min_dist"]), seed=int(z["seed"]))
    Yr = rand.fit_transform(x)
    forced = UMAP(s["K"], min_dist=float(z["min_dist"]), seed=int(z["seed"]), init="spectral", spectral_options=dict(max_restarts=0, max_basis=4))
    Yf = forced.fit_transform(x)
    out = capsys.readouterr().out
    assert rand.init_ == "random" and forced.init_ == "random" and forced.n_components_ == 1
    assert out.count("\n") == 1 and "the spectral start did not converge" in out and Yf.tobytes() == Yr.tobytes()
    trust, trust_r = float(trustworthiness(x, Y, n_neighbors=5)), float(trustworthiness(x, Yr, n_neighbors=5))
    print("trustworthiness %.4f from the spectral start (float64 reference %.4f, margin %.4f), %.4f from the random start (float64 "
          "reference %.4f)" % (trust, float(z["trust_spectral"]), float(rec["trust_margin"]), trust_r, float(z["trust_random"])))
    assert trust >= float(z["trust_spectral"]) - float(rec["trust_margin"])


def test_plot_2d_with_the_spectral_start(tmp_path):
    N, d = 300, 16
    x = T.make_blobs(N, d, 4, seed=9)[0]
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["tomo_a", "tomo_b"])[rs.randint(2, size=N)],
             coords=rs.randint(20, 400, size=(N, 3)).astype(np.int64))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "map"
    r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path", str(out),
                        "--n_cluster", "0", "--k", "8", "--niter", "5", "--mode", "umap", "--num_neighbor", "15", "--umap_init", "spectral"],
                       cwd=REPO, env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for f in ("embeddings_2d.npz", "all_colors.npy", "knn_graph.npz"):
        assert (out / f).exists(), f
    e = np.load(out / "embeddings_2d.npz")
    assert sorted(e.files) == sorted(["a", "b", "min_dist", "n_epochs", "n_neighbors", "seed", "y", "y01", "init", "n_graph_components",
                                      "eigenvalues"])
    assert str(e["init"]) in ("spectral", "random") and int(e["n_graph_components"]) >= 1 and e["eigenvalues"].dtype == np.float64
    assert e["y"].shape == (N, 2) and np.isfinite(e["y"]).all() and e["y01"].min() >= 0 and e["y01"].max() <= 1
    assert "UMAP start %s (--umap_init spectral)" % str(e["init"]) in r.stdout
    assert np.load(out / "all_colors.npy").shape == (N, 3)
