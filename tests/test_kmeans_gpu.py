"""k-means on the MI355X (csrc/kmeans.hip, utils/kmeans.py, plot_2d, interactive_to_training_coords) against the float64
arbiter of tests/kmeans_ref.py.  Parity statement: labels bit-exact outside a (d + 8) 2^-24 tie band that holds
<= 0.2 % of the test points, means f64-arbitrated at the standard factor 2."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kmeans_ref as R
from conftest import REPO, f32_equivalent

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _gpu_assign(x, c):
    from cet_pick_amd import hipops as H
    xd, cd = _dev(x), _dev(np.asarray(c, np.float32))
    labels, dist = H.kmeans_assign(xd, H.kmeans_xnorm(xd), H.kmeans_prep(cd), cd.shape[0])
    return labels.cpu().numpy(), dist.cpu().numpy()


def _gpu_update(x, labels, prev, with_split_counter=False):
    import torch
    from cet_pick_amd import hipops as H
    xd, cd = _dev(x), _dev(np.asarray(prev, np.float32)).clone()
    ns = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = H.kmeans_update(xd, _dev(labels, torch.int32), cd, nsplit=ns)
    return cd, counts, int(ns.cpu()[0])


@functools.lru_cache(maxsize=None)
def _case(name):
    N, d, k, spread = R.CASES[name]
    x = R.make(N, d, seed=7, spread=spread)
    c0 = x[R.init_rows(N, k)].copy()
    c5, _ = R.lloyd(x, c0, 5)
    return x, c0, c5.astype(np.float32)


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
@pytest.mark.parametrize("where", ["initial", "after5"])
def test_assign_matches_float64_outside_the_tie_band(name, where):
    x, c0, c5 = _case(name)
    c = c0 if where == "initial" else c5
    labels, dist = _gpu_assign(x, c)
    R.check_assign(x, c, labels, dist, what="case %s %s" % (name, where))


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_ties_and_duplicates_go_to_the_lowest_index():
    rs = np.random.RandomState(3)
    d, k, n = 24, 40, 3000
    c = rs.randint(-8, 9, size=(k, d)).astype(np.float32)
    c[17] = c[5]                                     # duplicates: 5 must win over 17 and 33
    c[33] = c[5]
    c[21] = c[20]
    c[21, 0] = c[20, 0] + 4                          # c20 and c21 differ in one coordinate by 4: the midplane is integer
    x = np.empty((n, d), np.float32)
    x[:1000] = c[5] + rs.randint(-1, 2, size=(1000, d))
    x[1000:2000] = c[20] + rs.randint(-1, 2, size=(1000, d))
    x[1000:2000, 0] = c[20, 0] + 2                   # exactly equidistant from c20 and c21
    x[2000:] = rs.randint(-8, 9, size=(n - 2000, d))
    want, _, _, gap, _ = R.assign64(x, c)            # integers: float64 is exact, np.argmin takes the first minimum
    assert (gap[:2000] == 0).sum() >= 1000           # the ties are real
    for run in range(3):
        labels, dist = _gpu_assign(x, c)
        assert np.array_equal(labels, want), "run %d: %d labels differ" % (run, int((labels != want).sum()))
    assert not np.isin(labels, [17, 33, 21]).any() or (want == labels).all()
    assert (labels[:1000] != 17).all() and (labels[:1000] != 33).all() and (labels[1000:2000] != 21).all()


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_update_counts_exact_means_f32_equivalent_and_deterministic(name):
    import torch
    x, c0, _ = _case(name)
    k = c0.shape[0]
    labels = R.assign64(x, c0)[0]                    # the float64 labels: assign cannot leak in
    ref, counts = R.means64(x, labels, k, c0)
    assert (counts > 0).all()
    cpu32 = np.stack([x[labels == j].sum(0, dtype=np.float32) / np.float32(counts[j]) for j in range(k)])
    got, gc, ns = _gpu_update(x, labels, c0)
    assert np.array_equal(gc.cpu().numpy(), counts) and ns == 0
    e = f32_equivalent(got.cpu().numpy(), cpu32, ref, what="means case " + name)
    print("case %s means: GPU %.3e, CPU fp32 %.3e from float64" % ((name,) + e))
    got2, gc2, _ = _gpu_update(x, labels, c0)
    assert torch.equal(got, got2) and torch.equal(gc, gc2)


def test_two_fits_give_the_same_bytes():
    from cet_pick_amd.utils.kmeans import Kmeans
    x, c0, _ = _case("C")
    out = []
    for _ in range(2):
        km = Kmeans(x.shape[1], c0.shape[0], niter=12)
        km.train(x)
        D, I = km.assign(x)
        out.append((km.centroids, km.obj, D, I))
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert out[0][1].shape == (12,)


# 4 ------------------------------------------------------------------------------------------------------------------------
def _empty_init():
    x, c0, _ = _case("C")
    init = c0.copy()
    init[[7, 11, 19, 30, 41]] = init[[0, 1, 2, 3, 4]]           # 5 duplicated rows: the later copy never wins a point
    init[[9, 25, 44]] = 50.0 + np.arange(3, dtype=np.float32)[:, None]      # 3 rows far from every point
    return x, init


def test_empty_clusters_follow_the_restated_rule():
    from cet_pick_amd.utils.kmeans import Kmeans
    x, init = _empty_init()
    k = init.shape[0]
    want_c, want_n, _, _, served = R.lloyd_step(x, init)
    assert len(served) == 8
    km = Kmeans(x.shape[1], k, niter=1)
    km.train(x, init=init)
    assert km.n_split == len(served)
    assert np.array_equal(km.counts.cpu().numpy(), want_n)
    got = km.centroids
    # donors exactly: a wrong donor or a wrong sign moves a row by eps = 2^-10 of its size or more.  The bound on the distance
    # from the restated float64 values is the worst case of what fp32 may add: the first-level sums of the mean have at most
    # 64 terms (64 x 2^-24), then one rounding of the mean and one of the (1 +- eps) product
    bound = (64 + 2) * 2.0 ** -24
    err = np.abs(got - want_c).max(axis=1) / np.abs(want_c).max(axis=1)
    print("empty clusters: served", served, "max rel err %.3e (bound %.3e, eps %.3e)" % (float(err.max()), bound, R.EPS))
    assert float(err.max()) <= bound, float(err.max())
    for e, dn in served[-3:]:                        # the (1 + eps) / (1 - eps) ratio between a served row and its last donor
        if sum(1 for s in served if dn in s) == 1:
            ratio = got[e].astype(np.float64) / got[dn].astype(np.float64)
            sign = np.where(np.arange(got.shape[1]) % 2 == 0, 1.0, -1.0)
            assert np.allclose(ratio, (1 + R.EPS * sign) / (1 - R.EPS * sign), rtol=4 * 2.0 ** -24, atol=0)
    km5 = Kmeans(x.shape[1], k, niter=5)
    km5.train(x, init=init)
    assert (km5.counts.cpu().numpy() > 0).all()
    _, I = km5.assign(x)
    assert len(np.unique(I)) == k


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_fit_per_iteration_against_the_arbiter_restarted_from_the_device_state():
    from cet_pick_amd.utils.kmeans import Kmeans
    x, c0, _ = _case("A")
    k, d = c0.shape
    cur = c0
    for it in range(8):                              # niter = 1 fits chained through init=
        km = Kmeans(d, k, niter=1)
        km.train(x, init=cur)
        nxt = km.centroids
        labels64, dist64 = R.check_assign(x, cur, *_gpu_assign(x, cur), what="fit iteration %d" % it)
        # the device's own labels of this iteration (they may differ from float64 inside the band): its means are checked
        # for THOSE labels
        gl = _gpu_assign(x, cur)[0].astype(np.int64)
        ref, counts = R.means64(x, gl, k, cur)
        assert np.array_equal(km.counts.cpu().numpy(), counts) and km.n_split == 0
        cpu32 = np.stack([x[gl == j].sum(0, dtype=np.float32) / np.float32(max(counts[j], 1)) for j in range(k)])
        f32_equivalent(nxt, cpu32, ref, what="means iteration %d" % it)
        assert abs(float(km.obj[0]) - dist64.sum()) <= 1e-4 * dist64.sum()
        cur = nxt


def test_free_running_objective_is_monotone_and_self_consistent():
    from cet_pick_amd.utils.kmeans import Kmeans
    x, c0, _ = _case("A")
    k, d = c0.shape
    seen = []
    km = Kmeans(d, k, niter=25)
    km.iteration_hook = lambda it, self_, cent, counts: seen.append(cent.clone()) if it == 23 else None
    km.train(x, init=c0)
    obj = km.obj.astype(np.float64)
    print("objective:", obj[0], "->", obj[-1], "largest rise", float(np.max(np.diff(obj))))
    assert np.all(np.diff(obj) <= 1e-6 * obj[0])
    # obj[-1] is the objective of iteration 25's assign: against the centroids after 24 iterations
    before = seen[0].cpu().numpy()
    gl = _gpu_assign(x, before)[0].astype(np.int64)
    own = ((x.astype(np.float64) - before.astype(np.float64)[gl]) ** 2).sum()
    assert abs(obj[-1] - own) <= 1e-4 * own, (obj[-1], own)


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_recovers_the_generating_classes():
    from cet_pick_amd.utils.kmeans import Kmeans
    x, cls, _ = R.make(20000, 128, seed=7, spread=0.05, return_classes=True)
    init = np.stack([x[np.flatnonzero(cls == j)[0]] for j in range(48)])
    assert np.array_equal(R.lloyd_step(x, init)[2], cls)             # the float64 restatement does after the first
    km = Kmeans(128, 48, niter=10)
    km.train(x, init=init)
    _, I = km.assign(x)
    assert np.array_equal(I[:, 0], cls)


# 7 ------------------------------------------------------------------------------------------------------------------------
SHAPES = [           # (d, k, N, spread): every d, every k and every N of the issue's lists at least once
    (1, 2, 4099, 0.15),
    (17, 48, 70001, 0.15),
    (32, 256, 4099, 0.15),
    (128, 1000, 70001, 0.15),
    (130, 48, 4099, 0.15),
    (512, 256, 256, 0.15),
    (512, 1000, 4099, 0.15),
    (130, 2, 70001, 0.15),
    (17, 1000, 1000, 0.15),
]


@pytest.mark.parametrize("d,k,N,spread", SHAPES)
def test_shapes(d, k, N, spread):
    x = R.make(N, d, seed=7, spread=spread)
    c = x[R.init_rows(N, k)].copy()
    labels, dist = _gpu_assign(x, c)
    R.check_assign(x, c, labels, dist, what="shape d=%d k=%d N=%d" % (d, k, N))
    # and the update on the float64 labels: counts exact, means f32-equivalent
    l64 = R.assign64(x, c)[0]
    ref, counts = R.means64(x, l64, k, c)
    got, gc, _ = _gpu_update(x, l64, c)
    nz = counts > 0
    assert np.array_equal(gc.cpu().numpy()[nz], counts[nz])
    if nz.all():
        cpu32 = np.stack([x[l64 == j].sum(0, dtype=np.float32) / np.float32(counts[j]) for j in range(k)])
        f32_equivalent(got.cpu().numpy(), cpu32, ref, what="means d=%d k=%d N=%d" % (d, k, N))


def test_rows_past_two_gib_are_addressed():
    """N x d x 4 bytes > 2 GiB: the rows behind the 2 GiB offset get the labels float64 gives them."""
    import torch
    from cet_pick_amd import hipops as H
    d, k, n = 512, 16, (1 << 20) + 4099
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(n, d, device="cuda", generator=g)
    assert x.numel() * 4 > (1 << 31)
    rows = torch.arange(k, device="cuda") * (n // k) + 7
    c = x[rows].clone()
    labels, dist = H.kmeans_assign(x, H.kmeans_xnorm(x), H.kmeans_prep(c), k)
    tail = slice(n - 6000, n)
    R.check_assign(x[tail].cpu().numpy(), c.cpu().numpy(), labels[tail].cpu().numpy(), dist[tail].cpu().numpy(), what="past 2 GiB")
    assert torch.equal(labels[rows].long(), torch.arange(k, device="cuda"))
    counts = H.kmeans_update(x, labels, c)
    assert int(counts.sum()) == n and torch.equal(counts.long(), torch.bincount(labels.long(), minlength=k))
    j = int(labels[n - 1])
    ref = x[labels == j].double().mean(0)
    assert float((c[j].double() - ref).abs().max()) <= 1e-5


def test_unsupported_sizes_are_refused():
    import torch
    from cet_pick_amd import _lib as L, hipops as H
    x = torch.zeros(600, 513, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.kmeans_prep(x[:4].contiguous())                            # d = 513
    x = torch.zeros(600, 16, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.kmeans_prep(x[:1].contiguous())                            # k = 1
    img = H.kmeans_prep(x[:64].contiguous())
    with pytest.raises(L.HipExtensionError, match="unsupported"):    # k > N
        H.kmeans_assign(x[:32].contiguous(), H.kmeans_xnorm(x[:32].contiguous()), img, 64)
    with pytest.raises(L.HipExtensionError):
        H.kmeans_xnorm(torch.zeros(8, 16))                           # a host tensor


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_from_embeddings_to_training_coordinates(tmp_path):
    from cet_pick_amd.datasets.semi_files import read_coord_list
    N, d = 4099, 32
    x = R.make(N, d, seed=7, spread=0.15)
    rs = np.random.RandomState(11)
    tomo = np.array(["tomo_a", "tomo_b", "tomo_c"])
    names = tomo[rs.randint(3, size=N)]
    coords = rs.randint(20, 400, size=(N, 3)).astype(np.int64)
    np.savez(tmp_path / "all_output_info.npz", pred=x, name=names, coords=coords, subvol=np.zeros((N, 1, 2, 2), np.float32))
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cet_pick_amd.plot_2d", "--input", str(tmp_path / "all_output_info.npz"), "--path",
                        str(out), "--n_cluster", "0", "--k", "48", "--niter", "20"], cwd=REPO, env=env, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out / "kmeans_labels.npz")
    assert z["centroids"].shape == (48, d) and z["centroids"].dtype == np.float32 and z["obj"].shape == (20,)
    assert z["assign"].dtype == np.int32 and z["label"].dtype == np.int32 and np.array_equal(z["label"], z["assign"])
    R.check_assign(x, z["centroids"], z["assign"], z["dist"], what="plot_2d")
    a, b = (int(v) for v in np.argsort(-np.bincount(z["label"], minlength=48))[:2])
    txt = tmp_path / "training_coordinates.txt"
    r = subprocess.run([sys.executable, "-m", "cet_pick_amd.interactive_to_training_coords", "--input",
                        str(out / "kmeans_labels.npz"), "--output", str(txt), "--labels", "%d,%d" % (a, b)], cwd=REPO, env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    keep = np.isin(z["label"], [a, b])
    lines = open(txt).read().split("\n")
    assert lines[0] == "image_name\tx_coord\ty_coord\tz_coord" and lines[-1] == ""
    want = ["\t".join([str(n)] + [str(v) for v in c]) for n, c in zip(names[keep], coords[keep])]
    assert lines[1:-1] == want
    got = read_coord_list(str(txt), list(tomo))
    for t in tomo:
        assert np.array_equal(got[t], coords[keep & (names == t)].astype(np.int32))


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_no_host_round_trip_inside_the_iteration_loop():
    import torch
    from cet_pick_amd.utils import kmeans as K
    x, c0, _ = _case("C")
    niter = 50
    prev = torch.cuda.get_sync_debug_mode()

    def hook(it, self_, cent, counts):
        if it == 0:
            torch.cuda.set_sync_debug_mode("error")               # from the end of the first iteration ...
        elif it == niter - 1:
            torch.cuda.set_sync_debug_mode(prev)                  # ... to the end of the last

    km = K.Kmeans(x.shape[1], c0.shape[0], niter=niter)
    km.iteration_hook = hook
    try:
        km.train(x, init=c0)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert km.obj.shape == (niter,) and np.isfinite(km.obj).all()
    src = open(K.__file__).read()
    m = re.search(r"\n( +)for it in range\(self\.niter\):\n((?:\1 +.*\n|\s*\n)+)", src)
    assert m, "the iteration loop of Kmeans.train was not found"
    body = m.group(2)
    assert "kmeans_assign" in body and "kmeans_update" in body
    for word in ("hipDeviceSynchronize", "synchronize", ".item()", ".cpu()", ".numpy()", ".tolist()"):
        assert word not in body, word
