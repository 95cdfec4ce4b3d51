"""csrc/tsne.hip and utils/tsne.py on the MI355X against the float64 arbiter tests/tsne_ref.py.

The band of the gradient checks is tsne_ref.band(N) = (L + 16) 2^-24 with L = min(128, N): the worst case of the longest fp32
accumulation chain of the kernels (a tile of 128 points) plus 16 roundings for one term and its 1-ulp reciprocal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_ref
import tsne_ref as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"smallest": (17, 5), "odd": (257, 5), "wide": (1031, 42)}          # N, perplexity; K = min(N - 1, 3 P + 1)
_cache = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(name):
    """(index (N, K) int64, dist (N, K) f32, p (N, K) f32, beta (N,) f32) of make_blobs through knn_search and tsne_affinities,
    and the device tensors the gradient takes; made once per shape."""
    if name not in _cache:
        from cet_pick_amd import hipops as H
        from cet_pick_amd.utils.tsne import n_neighbors, reverse_graph
        N, perp = SHAPES[name]
        x = _dev(T.make_blobs(N, 24, 4, seed=N)[0])
        index, dist = H.knn_search(x, x, n_neighbors(N, perp), metric="l2", exclude_self=True)
        p, beta = H.tsne_affinities(dist, perp)
        rev_ptr, rev_edge = reverse_graph(index)
        _cache[name] = dict(N=N, perp=perp, K=index.shape[1], index=index.cpu().numpy().astype(np.int64), dist=dist.cpu().numpy(),
                            p=p.cpu().numpy(), beta=beta.cpu().numpy(), dev=(index, p, rev_ptr, rev_edge))
        _cache[name]["P"] = T.joint_P(_cache[name]["index"], _cache[name]["p"])
    return _cache[name]


def _hand_rows(K):
    """all distances equal; the first three zero; distances from 1e-6 to 1e6"""
    return np.stack([np.full(K, 3.5), np.concatenate([np.zeros(3), np.arange(1, K - 2)]), np.logspace(-6, 6, K)]).astype(np.float32)


# affinities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "wide"])
def test_affinities_hit_the_perplexity(name):
    """For every row, with beta the returned fp32 value and P64 = entropy_at(dist, beta) in float64: |H(P64) - ln P| <= 2e-5
    (sklearn's stopping tolerance plus the same again for the fp32 cast of beta), |p - P64| <= 2^-22 P64 + 1e-38, row sums
    within K 2^-24, all finite.  The entropy of a row lies between ln(number of smallest distances) and ln K whatever beta
    is, so a row of K equal distances cannot reach ln P: it is held to the exact uniform 1 / K instead."""
    from cet_pick_amd import hipops as H
    g = _graph(name)
    K, perp = g["K"], g["perp"]
    dist = np.concatenate([g["dist"], _hand_rows(K)])
    assert (np.diff(dist, axis=1) >= 0).all()
    p, beta = H.tsne_affinities(_dev(dist), perp)
    p, beta = p.cpu().numpy(), beta.cpu().numpy()
    assert p.dtype == np.float32 and beta.dtype == np.float32 and np.isfinite(p).all() and np.isfinite(beta).all() and (beta > 0).all()
    P64, Hrow = T.entropy_at(dist, beta)
    reachable = (dist == dist[:, :1]).sum(1) < perp
    assert (~reachable).sum() == 1 and not reachable[len(g["dist"])]
    e_h = np.abs(Hrow - np.log(perp))[reachable]
    e_p = np.abs(p - P64) / (2.0 ** -22 * P64 + 1e-38)
    e_s = np.abs(p.astype(np.float64).sum(1) - 1)
    print("%s: N=%d K=%d P=%d: |H - ln P| max %.3e (bound 2e-5), |p - P64| max %.3f of its bound, row sum error max %.3e (bound %.3e), "
          "beta %.3e .. %.3e" % (name, len(dist), K, perp, e_h.max(), e_p.max(), e_s.max(), K * 2.0 ** -24, beta.min(), beta.max()))
    assert e_h.max() <= 2e-5
    assert e_p.max() <= 1.0
    assert e_s.max() <= K * 2.0 ** -24
    assert (p[len(g["dist"])] == np.float32(1.0 / K)).all()


# gradient ---------------------------------------------------------------------------------------------------------------------
def _gradient(g, Y, exaggeration, n_split):
    from cet_pick_amd import hipops as H
    grad, z, kl = H.tsne_gradient(_dev(Y), *g["dev"], exaggeration=exaggeration, n_split=n_split)
    return grad.cpu().numpy(), z.cpu().numpy(), kl.cpu().numpy()


def _check_gradient(g, Y, what):
    N, b = g["N"], T.band(g["N"])
    for exaggeration in (12.0, 1.0):
        want, Z, KL, scale, klscale = T.grad_kl64(Y, g["P"], exaggeration)
        for n_split in (0, 1, 3):
            grad, z, kl = _gradient(g, Y, exaggeration, n_split)
            again = _gradient(g, Y, exaggeration, n_split)
            e_g = (np.abs(grad - want) / (b * scale[:, None])).max()
            e_z, e_k = abs(float(z[0]) - Z) / (b * Z), abs(float(kl[0]) - KL) / (b * klscale)
            print("%s N=%d K=%d exaggeration %g n_split %d: gradient error max %.4f band, Z %.4f band, KL %.4f band (band = %.3e, "
                  "Z = %.6g, KL = %.6g)" % (what, N, g["K"], exaggeration, n_split, e_g, e_z, e_k, b, Z, KL))
            assert np.isfinite(grad).all() and e_g <= 1.0 and e_z <= 1.0 and e_k <= 1.0
            assert all(a.tobytes() == c.tobytes() for a, c in zip((grad, z, kl), again)), "two runs differ"


@pytest.mark.parametrize("sigma", [1e-4, 10.0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradient_matches_float64(name, sigma):
    g = _graph(name)
    Y = (np.random.RandomState(5).standard_normal((g["N"], 2)) * sigma).astype(np.float32)
    _check_gradient(g, Y, "%s sigma %g" % (name, sigma))


def test_gradient_with_coincident_points():
    """y_i = y_j for i != j is legal: q = 1 and no force between the two."""
    g = _graph("odd")
    Y = np.random.RandomState(6).standard_normal((g["N"], 2)).astype(np.float32)
    Y[[3, 40, 41, 130, 200, 254, 255, 256]] = Y[3]
    _check_gradient(g, Y, "coincident")


def test_z_counts_no_self_term():
    g = _graph("smallest")
    for n_split in (0, 1, 3):
        grad, z, kl = _gradient(g, np.zeros((17, 2), np.float32), 12.0, n_split)
        assert float(z[0]) == 17 * 16 and (grad == 0).all() and np.isfinite(kl).all()


def test_unsupported_arguments_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    g = _graph("odd")
    Y = torch.zeros(g["N"], 2, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.tsne_gradient(Y, *g["dev"], n_split=33)
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.tsne_affinities(torch.zeros(10, 128, device="cuda"), 5)
    with pytest.raises(L.HipExtensionError):
        H.tsne_gradient(Y.cpu(), *g["dev"])
    with pytest.raises(L.HipExtensionError, match="workspace too small"):
        H.tsne_gradient(Y, *g["dev"], ws=torch.empty(256, dtype=torch.uint8, device="cuda"))


# update -----------------------------------------------------------------------------------------------------------------------
def test_update_is_sklearns_step():
    """|grad|, |velocity| >= 1e-3: no sign test on a tie.  Gains start on both sides of the floor 0.01 / 0.8."""
    from cet_pick_amd import hipops as H
    rs = np.random.RandomState(8)
    n = 1031
    sign = lambda: rs.choice([-1.0, 1.0], size=(n, 2))                        # noqa: E731
    y = rs.standard_normal((n, 2)).astype(np.float32)
    grad = (sign() * rs.uniform(1e-3, 2.0, (n, 2))).astype(np.float32)
    vel = (sign() * rs.uniform(1e-3, 2.0, (n, 2))).astype(np.float32)
    gains = np.exp(rs.uniform(np.log(0.01), np.log(3.0), (n, 2))).astype(np.float32)
    for momentum, lr in ((0.5, 50.0), (0.8, 212.5)):
        y2, v2, g2 = T.update32(y, grad, vel, gains, momentum, lr)
        assert (g2 == np.float32(0.01)).sum() > 10 and (g2 > gains).sum() > 100
        ty, tv, tg = _dev(y), _dev(vel), _dev(gains)
        H.tsne_update(ty, _dev(grad), tv, tg, momentum, lr)
        assert np.array_equal(tg.cpu().numpy(), g2)
        for got, want, what in ((tv.cpu().numpy(), v2, "velocity"), (ty.cpu().numpy(), y2, "y")):
            ulp = (np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))).max()
            print("momentum %g lr %g: %s within %.2f ulp" % (momentum, lr, what, ulp))
            assert ulp <= 4


# end to end -------------------------------------------------------------------------------------------------------------------
def test_fit_transform_on_the_fixture(golden):
    """kl_divergence_ is the device's divergence of ITS affinities (its own neighbour search and fp32 table), so it is held
    against the arbiter's float64 divergence of those affinities; the comparison with sklearn's recorded runs takes the
    arbiter's affinities, as the recorded values do."""
    from cet_pick_amd import hipops as H
    from cet_pick_amd.utils.tsne import TSNE
    z = golden("tsne_small.npz")
    x, label = z["x"], z["label"].astype(np.int64)
    ts = TSNE(perplexity=5, seed=42)
    Y = ts.fit_transform(x)
    assert Y.shape == (600, 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and ts.n_iter_ <= 1000
    ts2 = TSNE(perplexity=5, seed=42)
    assert ts2.fit_transform(x).tobytes() == Y.tobytes() and ts2.kl_divergence_ == ts.kl_divergence_
    index, dist = ts.graph(_dev(x))
    P_dev = T.joint_P(index.cpu().numpy(), H.tsne_affinities(dist, 5)[0].cpu().numpy())
    _, _, kl_dev, _, klscale = T.grad_kl64(Y, P_dev)
    P = T.joint_P(z["index"].astype(np.int64), T.affinities64(z["dist"], 5)[0])
    kl, agree = T.kl64(Y, P), T.neighbour_agreement(Y, label)
    cap = z["sk_kl"].max() * (1 + float(z["kl_margin"]))
    print("n_iter_ %d, kl_divergence_ %.6f, KL64 of its affinities %.6f (%.4f band), KL64 %.6f (sklearn's five %s, margin %.4f, cap "
          "%.6f), agreement %.4f (sklearn's worst %.4f)" % (ts.n_iter_, ts.kl_divergence_, kl_dev,
                                                           abs(ts.kl_divergence_ - kl_dev) / (T.band(600) * klscale), kl,
                                                           np.round(z["sk_kl"], 6).tolist(), float(z["kl_margin"]), cap, agree,
                                                           z["sk_agree"].min()))
    assert abs(ts.kl_divergence_ - kl_dev) <= T.band(600) * klscale
    assert kl <= cap
    assert agree >= z["sk_agree"].min()


def test_plot_2d_writes_the_map(tmp_path):
    N, d = 300, 16
    x = T.make_blobs(N, d, 4, seed=9)[0]
    rs = np.random.RandomState(11)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=np.array(["tomo_a", "tomo_b"])[rs.randint(2, size=N)],
             coords=rs.randint(20, 400, size=(N, 3)).astype(np.int64))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for tag, extra in (("map", ["--mode", "tsne", "--num_neighbor", "5"]), ("plain", ["--num_neighbor", "5"])):
        out = tmp_path / tag
        r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path",
                            str(out), "--n_cluster", "0", "--k", "8", "--niter", "5"] + extra, cwd=REPO, env=env, timeout=300,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = (out, r.stdout)
    assert not (outs["plain"][0] / "embeddings_2d.npz").exists() and "embeddings_2d" not in outs["plain"][1]
    e = np.load(outs["map"][0] / "embeddings_2d.npz")
    assert e["y"].shape == (N, 2) and e["y"].dtype == np.float32 and np.isfinite(e["y"]).all()
    assert np.array_equal(e["y01"].min(0), [0, 0]) and np.array_equal(e["y01"].max(0), [1, 1])
    assert (int(e["perplexity"]), int(e["seed"])) == (5, 42) and int(e["n_iter"]) <= 1000 and np.isfinite(e["kl"])
    assert "t-SNE map of 300 picks, perplexity 5" in outs["map"][1]
    g = np.load(outs["map"][0] / "knn_graph.npz")
    knn_ref.check_knn(x, x, 5, "l2", g["index"], g["dist"], True, what="plot_2d --mode tsne")
    p = np.load(outs["plain"][0] / "knn_graph.npz")                              # the first 5 of 16 are the search for 5
    assert g["index"].tobytes() == p["index"].tobytes() and g["dist"].tobytes() == p["dist"].tobytes()
