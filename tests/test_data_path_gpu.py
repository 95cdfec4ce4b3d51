"""csrc/preproc.hip (MRC reorder, per-slice statistics, z-score, 8-bit quantise + min-max) and csrc/crop_norm.hip (raw,
sum-z / min-max, z-normalised and chain crops, the table form, the 8-bit round trip), each against the plain float64
restatement in tests/data_path_ref.py (proven on the CPU by tests/test_data_path_ref_cpu.py), through the C entries, so that
extents, slice counts and windows the Python wrappers never produce are reached.

Copies (reorder, raw crops), minima, maxima and quantiser levels are compared bit for bit; mean, std, z-score and the 8-bit
round trip by a relative or ulp bound with the measured worst case beside it; everything else through
conftest.f32_equivalent with its defaults.

Measured on the MI355X (the module prints every figure again when run with -s); norm-relative errors from float64, the
largest over a group's cases, beside the CPU float32 arbiter's on the same case:
  mi_vol_stats, N(100, 7)            mean 0 (equal to numpy's), std 1.384e-16 relative
  mi_vol_stats, voxel 0 = 32767      mean 1.303e-14, std 6.509e-12 relative
  mi_zscore                          0 ulp from float32((x - mean) / std) on every case
  mi_zscore_quantize_minmax          every voxel on its level; no voxel of the inputs is tie-adjacent
  z-norm crop, fast kernel           7.597e-06 at (1, 2, 1), arbiter 7.595e-06; 1.335e-06 at (8, 64, 64), arbiter 1.445e-05
  z-norm crop, generic kernel        with the float32 sums it had: 2.006e-02 at (8, 64, 64), 1.739e-02 at (9, 57, 64),
                                     9.670e-03 at 32^3, 1.345e-04 at (3, 8, 80), arbiter 1e-06 .. 1.4e-05 - it failed 20 of
                                     the 20 cases that reach it.  With double sums (as the fast kernel's): the fast kernel's
                                     figures, 1.559e-06 at (9, 57, 64), 6.957e-07 at (3, 8, 80)
  table form, z-norm                 8.625e-07, arbiter 2.639e-06
  sum-z / min-max                    4.973e-07, float32 evaluation in the kernel's order 4.940e-07
  chain                              1.140e-07, arbiter 1.789e-07
  mi_u8_roundtrip_normalize          levels equal, 0 ulp"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_path_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu

MI_E_ARG, MI_E_WORKSPACE, MI_E_UNSUPPORTED = -1, -2, -3
GUARD, SENTINEL = 64, -7.25
ERRORS = {}                       # group -> largest figure seen

# relative error of mi_vol_stats' mean and std against float64 numpy: 8 x the largest value measured on the cases below
# (mean 0, std 1.384e-16; the factor leaves room for another summation order)
STATS_REL_BOUND = 8 * 1.384e-16
# the same where voxel 0, the shift K of the variance's shifted sums, is a hot pixel: sum d^2 / n - mean(d)^2 then cancels
# nine digits (measured: mean 1.303e-14, std 6.509e-12 - four orders below float32's 6e-8)
HOT_STATS_REL_BOUND = 8 * 6.509e-12


def _lib():
    from cet_pick_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    return getattr(L.lib(), name)(*args, L.stream())


def _ok(name, *args):
    rc = _call(name, *args)
    assert rc == 0, "%s returned %d" % (name, rc)


def _p(t):
    return _lib().ptr(t)


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _note(group, value):
    ERRORS[group] = max(ERRORS.get(group, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, v in sorted(ERRORS.items()):
        print("\nlargest, %-34s %.3e" % (group, v))


def _bits(a):
    """the float32 bit patterns (-0.0 is not +0.0), every NaN as one pattern"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _ulps(a, b):
    """distance in float32 steps; two NaNs are 0 apart, a NaN and a number 2^40"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


def _out(n):
    """n floats to write and a guard behind them"""
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def _take(buf, shape, what):
    n = int(np.prod(shape))
    host = buf.cpu().numpy()
    assert np.all(host[n:] == SENTINEL), what + ": wrote behind its %d floats" % n
    return host[:n].reshape(shape)


def _rel(got, ref):
    """|got - ref| / |ref| (ref == 0: |got|); a NaN on one side only is inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.abs(got))
    r = np.where(np.isnan(got) & np.isnan(ref), 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def _eq(group, got, cpu32, ref64, what):
    from conftest import f32_equivalent
    e_g, e_c = f32_equivalent(got, cpu32, ref64, what=what)
    print("%-16s %-64s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    _note(group + " GPU", e_g)
    _note(group + " CPU fp32", e_c)


# ------------------------------------------------------------------------------------------------
# mi_rec_reorder
# ------------------------------------------------------------------------------------------------
REORDER_SHAPES = [(1, 1, 1), (2, 1, 64), (5, 33, 31), (3, 70, 65), (33, 2, 97)]


def _rec(shape, mode):
    dtype = R.MRC_DTYPES[mode]
    rng = np.random.default_rng(mode + sum(shape))
    n = int(np.prod(shape))
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        flat = rng.integers(info.min, info.max + 1, n).astype(dtype)
        flat[rng.integers(0, n, 4)] = info.min
        flat[rng.integers(0, n, 4)] = info.max
        flat[0] = info.max if n == 1 else info.min
    else:
        flat = rng.standard_normal(n).astype(np.float32)
        flat[rng.integers(0, n, 4)] = -0.0
        # (which zero the maximum of -0.0 and +0.0 is, is nobody's contract: no +0.0 in the data)
        assert np.isfinite(flat).all() and not np.any(_bits(flat) == 0) and np.any(_bits(flat) == 0x80000000)
    return flat.reshape(shape)


def g_reorder(rec, mode, order, compress, n_out):
    src = _dev(rec.view(np.uint8).reshape(-1))
    dst = _out(n_out)
    d0, d1, d2 = rec.shape
    rc = _call("mi_rec_reorder", _p(src), mode, d0, d1, d2, R.ORDERS.index(order), int(compress), _p(dst))
    return rc, dst


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("mode", [0, 1, 2, 6])
def test_reorder(mode, order, compress):
    for shape in REORDER_SHAPES:
        rec = _rec(shape, mode)
        what = "reorder mode %d %s compress %d %s" % (mode, order, compress, shape)
        if order == "zxy" and compress and shape[0] % 2:
            rc, dst = g_reorder(rec, mode, order, compress, rec.size)
            assert rc == MI_E_ARG, what
            assert torch.all(dst == SENTINEL), what + ": a refused call wrote"
            continue
        ref = R.reorder(rec, order, compress)
        rc, dst = g_reorder(rec, mode, order, compress, ref.size)
        assert rc == 0, what
        got = _take(dst, ref.shape, what)
        assert np.array_equal(_bits(got), _bits(ref)), what


def test_reorder_refusals():
    rec = _rec((2, 3, 4), 2)
    src, dst = _dev(rec.view(np.uint8).reshape(-1)), _out(24)
    assert _call("mi_rec_reorder", _p(src), 3, 2, 3, 4, 0, 0, _p(dst)) == MI_E_UNSUPPORTED          # complex int16
    assert _call("mi_rec_reorder", _p(src), 4, 2, 3, 4, 0, 0, _p(dst)) == MI_E_UNSUPPORTED
    assert _call("mi_rec_reorder", _p(src), 2, 2, 3, 4, 4, 0, _p(dst)) == MI_E_ARG                  # no such order
    assert _call("mi_rec_reorder", _p(src), 2, 0, 3, 4, 0, 0, _p(dst)) == MI_E_ARG
    # the transpose kernel's grid.z is the A extent: 65,536 is refused, nothing is launched
    big = torch.zeros(65536, dtype=torch.int8, device="cuda")
    out = _out(65536)
    assert _call("mi_rec_reorder", _p(big), 0, 65536, 1, 1, 0, 0, _p(out)) == MI_E_UNSUPPORTED
    assert _call("mi_rec_reorder", _p(big), 0, 65535, 1, 1, 0, 0, _p(out)) == 0
    torch.cuda.synchronize()
    assert torch.all(out[:65535] == 0) and torch.all(out[65535:] == SENTINEL)


# ------------------------------------------------------------------------------------------------
# mi_vol_stats
# ------------------------------------------------------------------------------------------------
def g_stats(xd, n, e):
    lib = _lib().lib()
    nb = lib.mi_vol_stats_workspace_bytes(n, e)
    assert nb == 32 * n * ((e + 65535) // 65536)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.full((n * 4 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    _ok("mi_vol_stats", _p(xd), n, e, _p(st), _p(ws), nb)
    assert torch.all(st[n * 4:] == SENTINEL)
    return st[:n * 4].reshape(n, 4)


def _check_stats(x, what, group, bound):
    n, e = x.shape
    ref = R.slice_stats(x)
    got = g_stats(_dev(x), n, e).cpu().numpy()
    assert np.array_equal(got[:, 2:], ref[:, 2:]), what + ": min / max"
    e_mean, e_std = float(_rel(got[:, 0], ref[:, 0]).max()), float(_rel(got[:, 1], ref[:, 1]).max())
    print("%-60s mean %.3e  std %.3e" % (what, e_mean, e_std))
    _note(group + " mean rel", e_mean)
    _note(group + " std rel", e_std)
    assert e_mean <= bound, "%s: mean %.3e from float64" % (what, e_mean)
    assert e_std <= bound, "%s: std %.3e from float64" % (what, e_std)


@pytest.mark.parametrize("n,e", R.STAT_SHAPES)
def test_stats(n, e):
    _check_stats(R.slices(n, e), "stats (%d, %d)" % (n, e), "stats", STATS_REL_BOUND)


@pytest.mark.parametrize("name", sorted(R.hot_pixel_cases()))
def test_stats_hot_first_voxel(name):
    _check_stats(R.hot_pixel_cases()[name], "stats " + name, "stats hot voxel 0", HOT_STATS_REL_BOUND)


def test_stats_nan():
    """a NaN anywhere in a slice makes its four statistics NaN, also where the thread that met it goes on to other voxels
    (index 3: the thread visits 259 and 515 after it)"""
    x = R.slices(3, 600)
    x[0, 3] = np.nan
    x[1, 599] = np.nan
    got = g_stats(_dev(x), 3, 600).cpu().numpy()
    ref = R.slice_stats(x)
    print("stats of the NaN slices:", got[:2].tolist())
    assert np.isnan(ref[:2]).all() and np.isnan(got[1]).all()
    assert np.isnan(got[0, :2]).all(), "mean / std of slice 0"
    assert np.isnan(got[0, 2:]).all(), "min / max of slice 0 lost the NaN: %s" % got[0, 2:]
    assert np.array_equal(got[2, 2:], ref[2, 2:])
    assert _rel(got[2, 0], ref[2, 0]) <= STATS_REL_BOUND and _rel(got[2, 1], ref[2, 1]) <= STATS_REL_BOUND


def test_stats_refusals():
    lib = _lib().lib()
    assert lib.mi_vol_stats_workspace_bytes(0, 5) == 0 and lib.mi_vol_stats_workspace_bytes(5, 0) == 0
    n, e = 2, 65537
    x = _dev(R.slices(n, e))
    nb = lib.mi_vol_stats_workspace_bytes(n, e)
    assert nb == 32 * 2 * 2
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    assert _call("mi_vol_stats", _p(x), n, e, _p(st), _p(ws), nb - 1) == MI_E_WORKSPACE
    assert _call("mi_vol_stats", _p(x), n, e, _p(st), _p(None), nb) == MI_E_WORKSPACE
    assert _call("mi_vol_stats", _p(x), 65536, 1, _p(st), _p(ws), nb) == MI_E_ARG          # grid.y
    assert _call("mi_zscore", _p(x), _p(x), 65536, 1, _p(st)) == MI_E_ARG
    assert _call("mi_zscore_quantize_minmax", _p(x), _p(x), 65536, 1, _p(st), -2.5, 2.0, 0) == MI_E_ARG
    assert torch.all(st == SENTINEL)


# ------------------------------------------------------------------------------------------------
# mi_zscore, mi_zscore_quantize_minmax
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,e", R.STAT_SHAPES)
def test_zscore(n, e):
    """float32((x - mean) / std) of float64 within 1 ulp (measured: 0 ulp on every case): the kernel multiplies by 1 / std in double,
    the reference divides"""
    x = R.slices(n, e)
    xd = _dev(x)
    y = _out(n * e)
    _ok("mi_zscore", _p(xd), _p(y), n, e, _p(g_stats(xd, n, e)))
    what = "z-score (%d, %d)" % (n, e)
    got = _take(y, (n, e), what)
    worst = int(_ulps(got, R.zscore(x).astype(np.float32)).max())
    print("%-40s %d ulp" % (what, worst))
    _note("z-score ulp", worst)
    assert worst <= 1, what


@pytest.mark.parametrize("flat_zero", [0, 1])
@pytest.mark.parametrize("n,e", R.STAT_SHAPES)
def test_preprocess(n, e, flat_zero):
    """every voxel lands on the float64 reference's 8-bit level and the output is float32((q - qmin) / (qmax - qmin)) bit for
    bit; only a voxel whose pre-rounding value is within 1e-9 of a half-integer may sit one level off (the CPU module
    proves that at most 1e-4 of these inputs are such voxels, and that no slice's minimum or maximum is one)"""
    x = R.quantiser_slices(n, e)
    what = "preprocess (%d, %d) flat_zero %d" % (n, e, flat_zero)
    xd = _dev(x)
    st = g_stats(xd, n, e)
    ref_st = R.slice_stats(x)
    assert float(_rel(st.cpu().numpy()[:, :2], ref_st[:, :2]).max()) <= 1e-12, what + ": mean / std"
    y = _out(n * e)
    _ok("mi_zscore_quantize_minmax", _p(xd), _p(y), n, e, _p(st), -2.5, 2.0, flat_zero)
    got = _take(y, (n, e), what)
    q, t = R.quantize_levels(x)
    ties = R.tie_adjacent(t, 1e-9)
    assert ties.mean() <= 1e-4, what
    want = R.preprocess(x, flat_zero=bool(flat_zero)).astype(np.float32)
    flat = ~(ref_st[:, 1] > 0)
    if flat.any():
        assert np.all(got[flat] == 0) if flat_zero else np.isnan(got[flat]).all(), what + ": the constant slice"
        assert np.array_equal(_bits(got[flat]), _bits(want[flat]))
    assert np.array_equal(_bits(got)[~ties], _bits(want)[~ties]), \
        "%s: %d voxels off their level" % (what, int((_bits(got) != _bits(want))[~ties].sum()))
    if ties.any():
        with np.errstate(invalid="ignore"):
            lo, hi = q.min(1, keepdims=True), q.max(1, keepdims=True)
            level = np.round(got.astype(np.float64) * (hi - lo) + lo)
        assert np.all(np.abs(level - q)[ties] <= 1), what + ": a voxel next to a tie is more than one level off"
    _note("tie-adjacent share", ties.mean())


def test_preprocess_refusals():
    x = _dev(R.slices(1, 255))
    st = g_stats(x, 1, 255)
    y = _out(255)
    for mi, ma in ((2.0, 2.0), (2.0, -2.5), (float("nan"), 2.0)):
        assert _call("mi_zscore_quantize_minmax", _p(x), _p(y), 1, 255, _p(st), mi, ma, 0) == MI_E_ARG
    assert torch.all(y == SENTINEL)


# ------------------------------------------------------------------------------------------------
# mi_crop_normalize
# ------------------------------------------------------------------------------------------------
VOL_SHAPE, VOL2_SHAPE = (24, 40, 44), (9, 17, 21)
CROP_SHAPES = [(1, 2, 1), (5, 7, 19), (3, 8, 33), (2, 4, 64), (3, 8, 80), (8, 64, 64), (9, 57, 64)]


def _vol():
    return R.volume(VOL_SHAPE, 5)


def _takes_fast(size):
    """(only to label the figures) the shapes crop_fast_kernel takes: rows of <= 64 floats, <= 32 values per thread"""
    cz, cy, cx = size
    if cx > 64:
        return False
    cxp = 1
    while cxp < cx:
        cxp *= 2
    step = 16 * (64 // cxp)                    # rows the 16 waves take per iteration
    return -(-(cz * cy) // step) <= 32


def g_crop(vol_d, shape, centres, size, mode, flip):
    D, H, W = shape
    cz, cy, cx = size
    n = len(centres)
    oshape = (n, cy, cx) if mode == R.SUMZ_MINMAX else (n, cz, cy, cx)
    out = _out(int(np.prod(oshape)))
    cen_d = _dev(np.asarray(centres, np.int32))
    rc = _call("mi_crop_normalize", _p(vol_d), D, H, W, _p(cen_d), n, cz, cy, cx, mode, int(flip), _p(out))
    torch.cuda.synchronize()
    return rc, out, oshape


def _crop_ok(vol_d, shape, centres, size, mode, flip, what):
    rc, out, oshape = g_crop(vol_d, shape, centres, size, mode, flip)
    assert rc == 0, "%s returned %d" % (what, rc)
    return _take(out, oshape, what)


def _c32_znorm(raw):
    t = torch.from_numpy(np.ascontiguousarray(raw, np.float32))
    return torch.stack([(c - c.mean()) / c.std() for c in t]).numpy()


def _c32_chain(raw):
    out = []
    for c in torch.from_numpy(np.ascontiguousarray(raw, np.float32)):
        c = (c - c.mean()) / c.std()
        c = (c - c.min()) / (c.max() - c.min()) * 6.0 - 3.0
        out.append((c - c.mean()) / c.std())
    return torch.stack(out).numpy()


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", CROP_SHAPES)
def test_crop_raw(size, flip, generic, monkeypatch):
    if generic:
        monkeypatch.setenv("MI_CROP_GENERIC", "1")
    vol = _vol()
    cen = R.centres16(VOL_SHAPE, size, sum(size))
    what = "raw %s flip %d generic %d" % (size, flip, generic)
    got = _crop_ok(_dev(vol), VOL_SHAPE, cen, size, R.RAW, flip, what)
    assert np.array_equal(_bits(got), _bits(R.crops(vol, cen, size, R.RAW, flip))), what


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", CROP_SHAPES + [(32, 32, 32)])
def test_crop_znorm(size, flip, generic, monkeypatch):
    """(x - mean) / unbiased std on a volume of mean 100, sigma 7: the arbiter is torch's two-pass float32 evaluation"""
    if generic:
        monkeypatch.setenv("MI_CROP_GENERIC", "1")
    vol = _vol()
    cen = R.centres16(VOL_SHAPE, size, sum(size), keep_y=True)
    what = "z-norm %s flip %d generic %d" % (size, flip, generic)
    got = _crop_ok(_dev(vol), VOL_SHAPE, cen, size, R.ZNORM, flip, what)
    raw = R.crops(vol, cen, size, R.RAW, flip)
    assert all(np.ptp(c) > 0 for c in raw)
    _eq("z-norm " + ("fast" if _takes_fast(size) and not generic else "generic"), got, _c32_znorm(raw),
        R.crops(vol, cen, size, R.ZNORM, flip), what)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", [(3, 36, 36), (5, 8, 12), (3, 128, 126)])
def test_crop_sumz_minmax(size, flip):
    """against the float32 evaluation that adds the slices in ascending z, as the kernel does"""
    vol = _vol()
    cen = R.centres16(VOL_SHAPE, size, sum(size), keep_y=True)
    what = "sum-z %s flip %d" % (size, flip)
    got = _crop_ok(_dev(vol), VOL_SHAPE, cen, size, R.SUMZ_MINMAX, flip, what)
    ref32 = np.stack([R.sumz_minmax_f32(vol, c, size, flip) for c in cen])
    _eq("sum-z", got, ref32, R.crops(vol, cen, size, R.SUMZ_MINMAX, flip), what)
    assert got.min() == 0.0 and np.all(got.reshape(16, -1).min(1) == 0) and got.max() <= 1.0 + 1e-6


def test_crop_sumz_constant_window_and_lds_limit():
    vol = _vol()
    vd = _dev(vol)
    size = (3, 8, 12)
    cen = np.array([[44 + 12, 40 + 8, 24 + 3], [20, 20, 12]], np.int32)          # outside on all three axes; inside
    got = _crop_ok(vd, VOL_SHAPE, cen, size, R.SUMZ_MINMAX, False, "sum-z constant window")
    ref = R.crops(vol, cen, size, R.SUMZ_MINMAX)
    assert not np.isfinite(ref[0]).any() and not np.isfinite(got[0]).any()
    assert np.isfinite(got[1]).all()
    # (3, 128, 128): 64 KiB of dynamic LDS beside the kernel's static array - refused, nothing launched
    rc, out, _ = g_crop(vd, VOL_SHAPE, cen, (3, 128, 128), R.SUMZ_MINMAX, False)
    assert rc == MI_E_UNSUPPORTED
    assert torch.all(out == SENTINEL)
    desc, cen_d = _desc([vd]), _dev(cen)
    out = _out(2 * 128 * 128)
    assert _call("mi_crop_normalize_table", _p(desc), _p(None), _p(cen_d), _p(None), _p(None), 0, 2, 3, 128, 128,
                 R.SUMZ_MINMAX, 0, _p(out)) == MI_E_UNSUPPORTED
    assert torch.all(out == SENTINEL)
    out = _out(2 * 128 * 126)
    _ok("mi_crop_normalize_table", _p(desc), _p(None), _p(cen_d), _p(None), _p(None), 0, 2, 3, 128, 126, R.SUMZ_MINMAX,
        0, _p(out))
    got = _take(out, (2, 128, 126), "table sum-z (3, 128, 126)")
    _eq("sum-z", got[1], R.sumz_minmax_f32(vol, cen[1], (3, 128, 126)), R.crop(vol, cen[1], (3, 128, 126), R.SUMZ_MINMAX),
        "table sum-z (3, 128, 126)")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", [(6, 48, 48), (32, 32, 32)])
def test_crop_chain(size, flip):
    """ZNormalization -> RescaleIntensity(-3, 3) -> ZNormalization; 32^3 is exactly the 128 KiB of LDS the entry accepts"""
    vol = _vol()
    cen = R.centres16(VOL_SHAPE, size, sum(size), keep_y=True)
    what = "chain %s flip %d" % (size, flip)
    got = _crop_ok(_dev(vol), VOL_SHAPE, cen, size, R.CHAIN, flip, what)
    _eq("chain", got, _c32_chain(R.crops(vol, cen, size, R.RAW, flip)), R.crops(vol, cen, size, R.CHAIN, flip), what)


def test_crop_refusals():
    vd = _dev(_vol())
    cen = np.array([[20, 20, 12]], np.int32)
    for size, mode in (((32, 32, 33), R.CHAIN), ((0, 4, 4), R.RAW), ((4, 4, 4), 4), ((4, 4, 4), -1)):
        rc, out, _ = g_crop(vd, VOL_SHAPE, cen, size, mode, False)
        assert rc == (MI_E_UNSUPPORTED if mode == R.CHAIN else MI_E_ARG), (size, mode)
        assert torch.all(out == SENTINEL)


# ------------------------------------------------------------------------------------------------
# mi_crop_normalize_table
# ------------------------------------------------------------------------------------------------
def _desc(vols_d):
    """struct mi_vol_desc {const float* vol; int32 D, H, W, reserved}"""
    d = np.zeros((len(vols_d), 3), np.int64)
    for i, v in enumerate(vols_d):
        D, H, W = (int(a) for a in v.shape)
        d[i] = (v.data_ptr(), D | (H << 32), W)
    return _dev(d)


def _table(size, with_y_shift):
    """16 samples over two volumes of different extents: every sample's centre is one of its own volume's 16"""
    shapes = (VOL_SHAPE, VOL2_SHAPE)
    rng = np.random.default_rng(sum(size))
    owner = (np.arange(16) % 2).astype(np.int32)
    rng.shuffle(owner)
    per_vol = [R.centres16(s, size, 9, keep_y=True) for s in shapes]
    centres = np.stack([per_vol[o][i] for i, o in enumerate(owner)]).astype(np.int32)
    shift = rng.integers(-5, 6, (16, 3)).astype(np.int32)
    if not with_y_shift:
        shift[:, 1] = 0
    return owner, centres, shift, rng.permutation(16).astype(np.int64)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("mode", [R.RAW, R.ZNORM])
@pytest.mark.parametrize("size", [(5, 7, 19), (3, 8, 80)])
def test_crop_table(size, mode, flip, generic, monkeypatch):
    """owner, shift, order and first = 3, then each of owner / shift / order null in turn, against gather-then-crop"""
    if generic:
        monkeypatch.setenv("MI_CROP_GENERIC", "1")
    vols = [_vol(), R.volume(VOL2_SHAPE, 6)]
    vols_d = [_dev(v) for v in vols]
    desc = _desc(vols_d)
    owner, centres, shift, order = _table(size, with_y_shift=(mode == R.RAW))
    cz, cy, cx = size
    first, n = 3, 13
    # (every table stays referenced until its call has returned and the result is read: the pointer of a tensor that is
    # dropped right after _p() is handed out again by the allocator, to the next table of the same call)
    owner_d, centres_d, shift_d, order_d = _dev(owner), _dev(centres), _dev(shift), _dev(order)
    assert len({t.data_ptr() for t in (owner_d, centres_d, shift_d, order_d)}) == 4
    for drop in (None, "owner", "shift", "order"):
        o, s, p = (None if drop == "owner" else owner), (None if drop == "shift" else shift), (None if drop == "order" else order)
        what = "table %s mode %d flip %d generic %d without %s" % (size, mode, flip, generic, drop)
        out = _out(n * cz * cy * cx)
        _ok("mi_crop_normalize_table", _p(desc), _p(None if o is None else owner_d), _p(centres_d),
            _p(None if s is None else shift_d), _p(None if p is None else order_d), first, n, cz, cy, cx, mode, int(flip), _p(out))
        got = _take(out, (n, cz, cy, cx), what)
        raw = R.table_crops(vols, o, centres, s, p, first, n, size, R.RAW, flip)
        if mode == R.RAW:
            assert np.array_equal(_bits(got), _bits(raw)), what
        else:
            assert all(np.ptp(c) > 0 for c in raw)
            _eq("table z-norm", got, _c32_znorm(raw), R.table_crops(vols, o, centres, s, p, first, n, size, R.ZNORM, flip), what)
    out = _out(n * cz * cy * cx)
    assert _call("mi_crop_normalize_table", _p(desc), _p(owner_d), _p(centres_d), _p(shift_d), _p(order_d), first, n, cz, cy, cx,
                 R.CHAIN, int(flip), _p(out)) == MI_E_ARG
    assert torch.all(out == SENTINEL)


# ------------------------------------------------------------------------------------------------
# mi_u8_roundtrip_normalize
# ------------------------------------------------------------------------------------------------
def test_u8_round_trip():
    """x = float32(k / 255) and the float32 on either side of it: the levels are torch's float32 mul(255).byte() exactly, the
    normalised value within 1 ulp (measured: 0 ulp)"""
    k = (np.arange(256) / 255.0).astype(np.float32)
    x = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                        np.array([-0.1, 1.1, 0.0, 1.0], np.float32)])
    mean, std = 0.4, 0.2
    xt = torch.from_numpy(x)
    levels = xt.mul(255).clamp(0, 255).byte()
    want = ((levels.float() / 255.0 - mean) / std).numpy()
    assert levels[:256].tolist() == list(range(256)) and levels[513:768].tolist() == list(range(255))
    y = _out(x.size)
    xd = _dev(x)
    _ok("mi_u8_roundtrip_normalize", _p(xd), _p(y), x.size, mean, std)
    got = _take(y, x.shape, "u8 round trip")
    decoded = np.round((got.astype(np.float64) * np.float32(std) + np.float32(mean)) * 255.0)
    assert np.array_equal(decoded, levels.numpy().astype(np.float64)), \
        "levels differ at x = %s" % x[decoded != levels.numpy()][:8]
    worst = int(_ulps(got, want).max())
    print("u8 round trip: %d ulp" % worst)
    _note("u8 round trip ulp", worst)
    assert worst <= 1
    assert _call("mi_u8_roundtrip_normalize", _p(xd), _p(y), x.size, mean, 0.0) == MI_E_ARG
    assert _call("mi_u8_roundtrip_normalize", _p(xd), _p(y), x.size, mean, -1.0) == MI_E_ARG
