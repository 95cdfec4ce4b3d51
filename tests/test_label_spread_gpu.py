"""csrc/label_spread.hip through hipops, utils/label_spread.py and propagate_labels against the float64 restatement and the bounds
of tests/label_spread_ref.py.  Every bound comes from the inputs and the number formats (the docstrings derive
them); the tests print the largest share of its bound the device used."""
import argparse
import os

import numpy as np
import pytest

import label_spread_ref as R

pytestmark = pytest.mark.gpu

_cache = {}


def arbiter(name):
    """the variant with the restatement's weights and CSR, computed once and never changed"""
    if name not in _cache:
        v = R.make(name)
        v["w"], v["s"], v["t"] = R.weights(v["index"], v["dist"], 1)
        v["csr"] = R.sym_csr(v["index"], v["w"])
        _cache[name] = v
    return _cache[name]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def share(err, bound):
    """largest err / bound; an entry with bound 0 must have err 0"""
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def device_graph(name, edge_weight="gauss"):
    from cet_pick_amd.utils import label_spread as LS
    v = arbiter(name)
    key = (name, edge_weight, "device")
    if key not in _cache:
        _cache[key] = LS.spread_graph(dev(v["index"]), dev(v["dist"]), edge_weight)
    return v, _cache[key]


def host_csr(g):
    return g.row_ptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy(), g.deg.cpu().numpy()


@pytest.mark.parametrize("name", R.VARIANTS)
def test_weights_within_the_fp32_bound(name):
    """mode 1 against the float64 restatement within R.weights_bound (derived there from the two fp32 square roots, the product,
    the quotient and fp32 exp); the scales and mode 0 exactly."""
    from cet_pick_amd import hipops as H
    v = arbiter(name)
    w, scale = H.spread_weights(dev(v["index"]), dev(v["dist"]), 1)
    got = w.cpu().numpy().astype(np.float64)
    assert w.dtype.is_floating_point and w.element_size() == 4 and got.shape == v["index"].shape
    assert np.array_equal(scale.cpu().numpy().astype(np.float64), v["s"])
    sh = share(np.abs(got - v["w"]), R.weights_bound(v["w"], v["t"]) * (v["w"] > 0))
    print("%s: weights: share of the bound used %.4f; largest exponent %.2f; %d of %d edges at weight 0"
          % (name, sh, v["t"].max(), (v["w"] == 0).sum(), v["w"].size))
    assert sh <= 1.0
    w0, none = H.spread_weights(dev(v["index"]), None, 0)
    assert none is None and np.array_equal(w0.cpu().numpy(), R.weights(v["index"], None, 0)[0].astype(np.float32))
    if name == "dup":                                      # d2 = 0 between copies with s = 0: weight 1; towards such a row: 0
        assert (got[:120] == 1).all() and (v["s"][:120] == 0).all() and (got[120:] == 0).any()
    if name == "hub":
        assert (got[0, 0] == 0) and (got[1:, 0] > 0).all()  # row 0 lists itself: passed over


@pytest.mark.parametrize("name", R.VARIANTS)
def test_csr_structure_values_symmetry_and_bytes(name):
    """row_ptr and col are the restatement's; given the device's own w, deg is a sum of m non-negative float64 terms in another
    order than numpy's, so the two differ by at most 2 (m - 1) 2^-53 relative, taken as 2 m; dis = 1 / sqrt(deg) carries half of
    that plus two roundings on either side, val = w_sym (dis_i dis_j) two more products on either side:
    (m_i + m_j + 12) 2^-53 relative.  The matrix is symmetric to the bit and a second build gives the same bytes."""
    from cet_pick_amd.utils import label_spread as LS
    v, g = device_graph(name)
    row_ptr, col, val, deg = host_csr(g)
    assert np.array_equal(row_ptr, v["csr"][0]) and np.array_equal(col, v["csr"][1])
    assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float64 and deg.dtype == np.float64
    own = R.sym_csr(v["index"], g.w.cpu().numpy().astype(np.float64))
    m = np.diff(row_ptr).astype(np.float64)
    rows = np.repeat(np.arange(len(deg)), np.diff(row_ptr))
    sh_deg = share(np.abs(deg - own[3]), 2 * m * R.U * own[3])
    sh_val = share(np.abs(val - own[4]), (m[rows] + m[col] + 12) * R.U * own[4])
    print("%s: CSR: nnz %d, longest row %d, %d rows of degree 0; share of the bound used: deg %.4f, val %.4f"
          % (name, len(col), m.max(), (deg == 0).sum(), sh_deg, sh_val))
    assert sh_deg <= 1.0 and sh_val <= 1.0
    S = R.dense(row_ptr, col, val)
    assert np.array_equal(S, S.T) and (val >= 0).all()
    again = host_csr(LS.spread_graph(dev(v["index"]), dev(v["dist"]), "gauss"))
    for a, b in zip((row_ptr, col, val, deg), again):
        assert a.tobytes() == b.tobytes()
    if name == "hub":
        assert m[0] >= len(deg) - 2                        # vertex 0's lone-reverse range
    if name == "k70":
        assert v["index"].shape[1] > 64


@pytest.mark.parametrize("name", R.VARIANTS)
def test_sweeps_within_the_rounding_bound_and_exact_residual(name):
    """t = 5 sweeps on the device's own CSR against 5 float64 numpy sweeps.  Every term is non-negative, so errors are relative:
    a row's sum of m products by fused multiply-adds rounds m times, alpha times it once, (1 - alpha) Y once ((1 - alpha) is the
    same double on both sides), the final sum once: (m + 3) 2^-53 <= (m + 4) 2^-53 per sweep, m the longest row; the relative
    error of F_in passes through a non-negative sum unchanged, so t sweeps stay within t (m + 4) 2^-53.  The residual word is
    max |F_out - F_in| of the device's own arrays, exactly, and a sweep without the word writes the same bytes."""
    import torch
    from cet_pick_amd import hipops as H
    v, g = device_graph(name)
    row_ptr, col, val, _ = host_csr(g)
    S, m, t, alpha = R.dense(row_ptr, col, val), R.longest_row(row_ptr), 5, 0.9
    Y = R.one_hot(len(S), v["seed_index"], v["seed_class"], v["C"])
    y = dev(Y)
    f, ref = y.clone(), Y.copy()
    word = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    worst = 0.0
    for it in range(1, t + 1):
        out = H.spread_step(g.row_ptr, g.col, g.val, alpha, f, y, torch.empty_like(f), word)
        plain = H.spread_step(g.row_ptr, g.col, g.val, alpha, f, y, torch.full_like(f, -7.0))
        assert out.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
        assert float(word.view(torch.float64).cpu()[0]) == np.abs(out.cpu().numpy() - f.cpu().numpy()).max()
        f, ref = out, R.sweep(S, ref, Y, alpha)
        worst = max(worst, share(np.abs(f.cpu().numpy() - ref), it * (m + 4) * R.U * ref))
    print("%s: N=%d C=%d longest row %d: %d sweeps, share of t (m + 4) 2^-53 used %.4f" % (name, len(S), v["C"], m, t, worst))
    assert worst <= 1.0


def test_class_counts_outside_2_to_64_are_unsupported():
    import torch
    from cet_pick_amd import _lib as L
    v, g = device_graph("k1")
    n = g.n
    for c in (1, 65):
        f = torch.zeros((n, c), dtype=torch.float64, device="cuda")
        out = torch.full_like(f, 3.0)
        assert L.call("mi_spread_step", g.row_ptr, g.col, g.val, n, c, 0.9, f, f.clone(), out, None, may_decline=True) is False
        lab = torch.full((n,), 9, dtype=torch.int32, device="cuda")
        assert L.call("mi_spread_decide", f, n, c, 0.5, lab, f.clone(), f.clone(), may_decline=True) is False
        assert (out == 3.0).all() and (lab == 9).all()     # nothing was enqueued
    f = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(L.HipExtensionError, match="bad argument"):
        L.call("mi_spread_step", g.row_ptr, g.col, g.val, n, 2, 0.9, f, f.clone(), f, None)


@pytest.mark.parametrize("name", R.VARIANTS)
def test_spread_converges_to_the_closed_form(name):
    """spread() to tol = 1e-10 against F* = (1 - alpha) (I - alpha S)^-1 Y of the device's own S, within
    R.closed_form_bound: alpha / (1 - alpha) sqrt(N C) residual plus the rounding terms derived there."""
    from cet_pick_amd.utils import label_spread as LS
    v, g = device_graph(name)
    row_ptr, col, val, _ = host_csr(g)
    S, alpha = R.dense(row_ptr, col, val), 0.9
    star = R.closed_form(S, R.one_hot(len(S), v["seed_index"], v["seed_class"], v["C"]), alpha)
    F, n_iter, residual = LS.spread(g, v["seed_index"], v["seed_class"], v["C"], alpha=alpha, tol=1e-10, max_iter=1000, check_every=10)
    assert residual <= 1e-10 and n_iter % 10 == 0 and n_iter < 1000
    bound = R.closed_form_bound(len(S), v["C"], R.longest_row(row_ptr), alpha, residual, len(v["seed_index"]))
    err = np.abs(F.cpu().numpy() - star).max()
    print("%s: %d sweeps, residual %.3g, |F - F*| %.3g, share of the bound used %.4f" % (name, n_iter, residual, err, err / bound))
    assert err <= bound
    if name == "split":                                    # no seed in blob 1: mass 0 and label -1 there, to the bit
        label, conf, mass = (a.cpu().numpy() for a in LS.decide(F, 0.0))
        assert (mass[v["blob"] == 1] == 0).all() and (label[v["blob"] == 1] == -1).all() and (conf[v["blob"] == 1] == 0).all()
        assert (label[v["blob"] == 0] >= 0).all()


@pytest.mark.parametrize("name", R.VARIANTS)
def test_decision_is_the_restated_formula(name):
    from cet_pick_amd.utils import label_spread as LS
    v, g = device_graph(name)
    F = LS.spread(g, v["seed_index"], v["seed_class"], v["C"], max_iter=30, tol=0.0, check_every=30)[0]
    for min_conf in (0.0, 0.5, 0.9):
        label, conf, mass = (a.cpu().numpy() for a in LS.decide(F, min_conf))
        want = R.decide(F.cpu().numpy(), min_conf)
        assert np.array_equal(label, want[0]) and label.dtype == np.int32
        assert np.array_equal(conf, want[1]) and np.array_equal(mass, want[2])


@pytest.mark.parametrize("name", R.DECISION_VARIANTS)
def test_labels_agree_with_the_closed_form_where_decided(name):
    """Against the restatement's own closed form (its float64 weights): a pick is decided where its top-two margin exceeds twice
    R.closed_form_bound with delta = the fp32 weights' largest relative bound; at most 1 % are not, asserted before the device
    runs."""
    from cet_pick_amd.utils import label_spread as LS
    v = arbiter(name)
    row_ptr, col, _, _, val = v["csr"]
    S, alpha, tol = R.dense(row_ptr, col, val), 0.9, 1e-10
    star = R.closed_form(S, R.one_hot(len(S), v["seed_index"], v["seed_class"], v["C"]), alpha)
    bound = R.closed_form_bound(len(S), v["C"], R.longest_row(row_ptr), alpha, tol, len(v["seed_index"]), R.weight_delta(v["t"]))
    top = np.sort(star, 1)
    decided = top[:, -1] - top[:, -2] > 2 * bound
    assert (~decided).mean() <= 0.01
    g = device_graph(name)[1]
    F, n_iter, residual = LS.spread(g, v["seed_index"], v["seed_class"], v["C"], alpha=alpha, tol=tol)
    assert residual <= tol
    label = LS.decide(F, 0.0)[0].cpu().numpy()
    differ = label != R.decide(star, 0.0)[0]
    print("%s: bound %.3g, undecided %.3f %%, labels differ on %d picks, %d of them decided"
          % (name, bound, 100 * (~decided).mean(), differ.sum(), (differ & decided).sum()))
    assert not (differ & decided).any()


def _write_input(tmp_path, x, names, coords):
    inp = os.path.join(str(tmp_path), "all_output_info.npz")
    np.savez(inp, pred=x.astype(np.float32), name=names, coords=coords)
    return inp


def _run(tmp_path, **kw):
    from cet_pick_amd import propagate_labels as P
    argv = ["--path", os.path.join(str(tmp_path), "out")]
    for k, val in kw.items():
        argv += ["--" + k] + ([] if val is True else [str(val)])
    return P.main(P.add_arguments(argparse.ArgumentParser()).parse_args(argv))


def test_planted_blobs_are_recovered(tmp_path):
    x, blob, index, dist, seed_index, seed_class = R.planted()
    assert (blob[index] == blob[:, None]).all()            # on the CPU graph: no edge crosses blobs
    n = len(x)
    inp = _write_input(tmp_path, x, np.array(["t0"] * n), np.arange(3 * n).reshape(n, 3).astype(np.float32))
    graph, seeds = os.path.join(str(tmp_path), "knn_graph.npz"), os.path.join(str(tmp_path), "seeds.npz")
    np.savez(graph, index=index, dist=dist)
    np.savez(seeds, **{"index": seed_index, "class": seed_class})
    out = _run(tmp_path, input=inp, graph=graph, seed_index=seeds, min_conf=0.5)
    assert np.array_equal(out["label"], blob) and int(out["seed_flipped"]) == 0
    assert (out["conf"] == 1).all() and (out["mass"] > 0).all()
    assert float(out["residual"]) <= 1e-6 and str(out["edge_weight"]) == "gauss"


def test_seed_nearest_matches_the_restatement():
    from cet_pick_amd.utils import label_spread as LS
    rng = np.random.default_rng(3)
    n = 1000
    picks = rng.uniform(0, 100, (n, 3)).round(1)
    tomo = rng.integers(0, 3, n).astype(np.int32)
    picks[3] = picks[3 + 256] = picks[700] = (50.0, 50.0, 50.0)        # a tie across threads: the lowest pick
    tomo[[3, 3 + 256, 700]] = 1
    picks[10], picks[20] = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0)           # a tie at distance 1
    tomo[[10, 20]] = 2
    seeds = np.concatenate([[(50.0, 50.0, 50.5), (1.0, 0.0, 0.0), (500.0, 500.0, 500.0), (40.0, 40.0, 40.0), (1.0, 0.0, 0.0)],
                            rng.uniform(0, 100, (20, 3))])
    seed_tomo = np.concatenate([[1, 2, 0, 7, -1], rng.integers(0, 3, 20)]).astype(np.int32)
    radius = 6.0
    want_pick, want_dist = R.seed_nearest(picks, tomo, seeds, seed_tomo, radius)
    assert want_pick[0] == 3 and want_pick[1] == 10 and want_pick[2] == -1 and np.isfinite(want_dist[2])
    assert want_pick[3] == -1 and np.isinf(want_dist[3]) and want_pick[4] == -1 and (want_pick[5:] >= 0).any() and (want_pick[5:] < 0).any()
    pick, dist = LS.match_seeds(picks, tomo, seeds, seed_tomo, radius, device="cuda")
    assert np.array_equal(pick, want_pick) and pick.dtype == np.int32
    assert np.array_equal(np.isinf(dist), np.isinf(want_dist))
    fin = np.isfinite(want_dist)
    assert (np.abs(dist[fin] - want_dist[fin]) <= 2.0 ** -52 * want_dist[fin]).all()       # one float64 square root


def test_end_to_end_to_training_coordinates(tmp_path):
    from cet_pick_amd import interactive_to_training_coords as T
    x, blob = R.blobs(240, 3, spread=0.3, sep=6.0, seed=9)
    n = len(x)
    rng = np.random.default_rng(1)
    names = np.array(["tomoA" if i % 2 else "tomoB" for i in range(n)])
    coords = np.stack([rng.permutation(n) * 20 + 3, rng.permutation(n) * 20 + 5, rng.permutation(n) * 2 + 40], 1).astype(np.float32)
    inp = _write_input(tmp_path, x, names, coords)
    chosen = np.concatenate([np.flatnonzero(blob == b)[:3] for b in range(3)])
    lines = ["image_name\tx_coord\ty_coord\tz_coord\tclass"]
    for i in chosen:                                       # a little off the pick, z in full-tomogram units
        lines.append("%s\t%g\t%g\t%g\t%d" % (names[i], coords[i, 0] + 1.5, coords[i, 1] - 2, 2 * (coords[i, 2] + 0.5), blob[i]))
    lines.append("tomoA\t-500\t-500\t-500\t1")             # no pick within the radius
    lines.append("tomoZ\t3\t5\t40\t2")                     # no such tomogram
    table = os.path.join(str(tmp_path), "seeds.txt")
    with open(table, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = _run(tmp_path, input=inp, seeds=table, num_neighbor=8, if_double=True, seed_radius=8, min_conf=0.5)
    assert out["seed_pick"].tolist() == chosen.tolist() + [-1, -1] and out["seed_class"].tolist() == blob[chosen].tolist() + [1, 2]
    assert np.isinf(out["seed_dist"][-1]) and out["seed_dist"][-2] > 8 and (out["seed_dist"][:-2] < 3).all()
    path = os.path.join(str(tmp_path), "out", "propagated_labels.npz")
    saved = np.load(path)
    for key in ("name", "coords", "label", "conf", "mass", "score", "seed_pick", "seed_class", "seed_dist", "n_iter", "residual",
                "alpha", "edge_weight", "seed_flipped"):
        assert key in saved.files, key
    assert saved["score"].shape == (n, 3) and saved["score"].dtype == np.float32 and saved["label"].dtype == np.int32
    assert (saved["label"][saved["label"] >= 0] == blob[saved["label"] >= 0]).mean() > 0.95
    txt = os.path.join(str(tmp_path), "training_coordinates.txt")
    n_out = T.main(T.add_arguments(argparse.ArgumentParser()).parse_args(["--input", path, "--output", txt, "--labels", "0"]))
    want = ["\t".join([str(names[i])] + [str(j) for j in coords[i]]) for i in np.flatnonzero(saved["label"] == 0)]
    assert n_out == len(want) > 0
    assert open(txt).read().splitlines() == ["\t".join(T.HEADER)] + want
