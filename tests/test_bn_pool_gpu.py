"""The first third of csrc/train_ops.hip - the column reduction, every BatchNorm forward and backward kernel, the fused
BatchNorm + ReLU + max-pool, MaxPool3d, the global average pool and the bias column sum - each against the plain float64
restatement in tests/bn_pool_ref.py (proven against torch by tests/test_bn_pool_ref_cpu.py), through the C entries, so that
both BatchNorm paths run at row counts the Python wrappers would never give them.

Numeric results go through conftest.f32_equivalent with its defaults (the GPU may lie as far from float64 as twice torch's CPU
float32 evaluation of the same inputs does, plus the default floor); copies, argmax bytes, pooled maxima and
num_batches_tracked are compared bit for bit.  The float64 reference of a backward takes its ReLU mask from the GPU forward's
own y > 0 (so does the fp32 arbiter: no element is left out of a comparison); that this mask differs from float64's only on
the edge is asserted on its own."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_pool_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS32 = float(np.finfo(np.float32).eps)
MI_E_ARG, MI_E_WORKSPACE = -1, -2
ERRORS = {}                                # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64]
POOLS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2), (6, 2, 3), (2, 1, 0)]


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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(t):
    return None if t is None else t.cuda().contiguous()


def _eq(group, got, cpu32, ref64, what, more=()):
    from conftest import f32_equivalent
    e_g, e_c = f32_equivalent(_np(got), _np(cpu32), _np(ref64), what=what, more_cpu32=[_np(m) for m in more])
    print("%-14s %-60s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    rec = ERRORS.setdefault(group, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e_g), max(rec[1], e_c)
    return e_g, e_c


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, (e_g, e_c) in sorted(ERRORS.items()):
        print("\nlargest error, %-14s GPU %.3e  CPU fp32 %.3e" % (group, e_g, e_c))


def _cr_ok(C):
    return C >= 4 and C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0


# ------------------------------------------------------------------------------------------------
# the C entries, one thin wrapper each (device tensors in, device tensors out)
# ------------------------------------------------------------------------------------------------
def _ws(M, C):
    n = _lib().lib().mi_colreduce_workspace_bytes(M, C)
    return torch.empty(max(n, 16), dtype=torch.uint8, device="cuda"), n


def _sums(C):
    return torch.full((2 * C,), float("nan"), dtype=torch.float64, device="cuda")


def g_stats(x, M, C):
    s, (ws, n) = _sums(C), _ws(M, C)
    _ok("mi_bn_stats", _p(x), M, C, _p(s), _p(ws), n)
    return s


def g_apply(x, M, C, sums, count, gamma, beta, rm, rv, nbt, res, relu):
    y, save = torch.empty_like(x), torch.empty(2 * C, device="cuda")
    _ok("mi_bn_apply_fwd", _p(x), _p(y), M, C, _p(sums), float(count), _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), _p(nbt),
        _p(save), _p(res), int(relu))
    return y, save


def g_eval(x, M, C, rm, rv, gamma, beta, res, relu):
    y, save = torch.empty_like(x), torch.empty(2 * C, device="cuda")
    _ok("mi_bn_eval_fwd", _p(x), _p(y), M, C, _p(rm), _p(rv), _p(gamma), _p(beta), EPS, _p(save), _p(res), int(relu))
    return y, save


def g_bwd_reduce(dy, x, y, M, C, save, relu):
    s, (ws, n) = _sums(C), _ws(M, C)
    _ok("mi_bn_bwd_reduce", _p(dy), _p(x), _p(y), M, C, _p(save), int(relu), _p(s), _p(ws), n)
    return s


def g_bwd_apply(dy, x, y, M, C, save, gamma, sums, count, relu):
    dx, dg, db = torch.empty_like(x), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_bwd_apply", _p(dy), _p(x), _p(y), _p(dx), M, C, _p(save), _p(gamma), _p(sums), float(count), int(relu), _p(dg),
        _p(db))
    return dx, dg, db


def g_bwd_apply_res(dy, x, y, M, C, save, gamma, sums, count):
    dx, dres = torch.empty_like(x), torch.empty_like(x)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_bwd_apply_res", _p(dy), _p(x), _p(y), _p(dx), _p(dres), M, C, _p(save), _p(gamma), _p(sums), float(count),
        _p(dg), _p(db))
    return dx, dres, dg, db


def g_reduce_x(dy, x, M, C, save, gamma, beta):
    s, (ws, n) = _sums(C), _ws(M, C)
    _ok("mi_bn_relu_bwd_reduce_x", _p(dy), _p(x), M, C, _p(save), _p(gamma), _p(beta), _p(s), _p(ws), n)
    return s


def g_apply_x(dy, x, M, C, save, gamma, beta, sums, count):
    dx, dg, db = torch.empty_like(x), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_relu_bwd_apply_x", _p(dy), _p(x), _p(dx), M, C, _p(save), _p(gamma), _p(beta), _p(sums), float(count), _p(dg),
        _p(db))
    return dx, dg, db


def g_colsum(dy, M, C, guard=64):
    out = torch.full((C + guard,), -7.25, device="cuda")
    s, (ws, n) = _sums(max(C, 1)), _ws(M, C)
    _ok("mi_colsum", _p(dy), M, C, _p(out), _p(s), _p(ws), n)
    assert torch.equal(out[C:].cpu(), torch.full((guard,), -7.25)), "mi_colsum wrote behind its %d floats" % C
    return out[:C]


def g_small_fwd(x, M, C, gamma, beta, rm, rv, nbt, res, relu):
    y, save = torch.empty_like(x), torch.empty(2 * C, device="cuda")
    _ok("mi_bn_small_fwd", _p(x), _p(y), M, C, _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), _p(nbt), _p(save), _p(res),
        int(relu))
    return y, save


def g_small_bwd(dy, x, y, M, C, save, gamma, relu):
    dx, dg, db = torch.empty_like(x), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_small_bwd", _p(dy), _p(x), _p(y), _p(dx), M, C, _p(save), _p(gamma), int(relu), _p(dg), _p(db))
    return dx, dg, db


def g_small_pool_fwd(x, M, C, V, gamma, beta, rm, rv, nbt):
    y, pooled, save = torch.empty_like(x), torch.empty(M // V, C, device="cuda"), torch.empty(2 * C, device="cuda")
    _ok("mi_bn_small_pool_fwd", _p(x), _p(y), _p(pooled), M, C, V, _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), _p(nbt),
        _p(save))
    return y, pooled, save


def g_small_pool_bwd(dp, x, y, M, C, V, save, gamma):
    dx, dg, db = torch.empty_like(x), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_small_pool_bwd", _p(dp), _p(x), _p(y), _p(dx), M, C, V, _p(save), _p(gamma), _p(dg), _p(db))
    return dx, dg, db


def _pooled_shape(shape, k, s, p):
    N, D, H, W, C = shape
    return (N, R.pool_out(D, k, s, p), R.pool_out(H, k, s, p), R.pool_out(W, k, s, p), C)


def g_maxpool_fwd(x, k, s, p, want_arg=True):
    N, D, H, W, C = x.shape
    y = torch.empty(_pooled_shape(x.shape, k, s, p), device="cuda")
    arg = torch.full(y.shape, 255, dtype=torch.uint8, device="cuda") if want_arg else None
    _ok("mi_maxpool3d_fwd", _p(x), _p(y), _p(arg), N, D, H, W, C, k, s, p)
    return y, arg


def g_maxpool_bwd(dy, arg, shape, k, s, p):
    N, D, H, W, C = shape
    dx = torch.full(shape, float("nan"), device="cuda")
    _ok("mi_maxpool3d_bwd", _p(dy), _p(arg), _p(dx), N, D, H, W, C, k, s, p)
    return dx


def g_fused(x, k, s, p, sums, count, gamma, beta, rm, rv, nbt, want_arg=True):
    N, D, H, W, C = x.shape
    y = torch.empty(_pooled_shape(x.shape, k, s, p), device="cuda")
    arg = torch.full(y.shape, 255, dtype=torch.uint8, device="cuda") if want_arg else None
    save = torch.empty(2 * C, device="cuda")
    _ok("mi_bn_relu_maxpool3d_fwd", _p(x), _p(y), _p(arg), N, D, H, W, C, k, s, p, _p(sums), float(count), _p(gamma), _p(beta),
        EPS, MOM, _p(rm), _p(rv), _p(nbt), _p(save))
    return y, arg, save


# ------------------------------------------------------------------------------------------------
# torch CPU float32: the arbiter
# ------------------------------------------------------------------------------------------------
def c32_bn_fwd(x, gamma, beta, rm, rv, res, relu, dup=1):
    """(y, save, running_mean, running_var) of torch's CPU fp32 BatchNorm over the batch held `dup` times"""
    M = x.shape[0]
    xx = torch.cat([x] * dup) if dup > 1 else x
    rm2, rv2 = (rm.clone(), rv.clone()) if rm is not None else (None, None)
    if M * dup > 1:
        y, mean, inv = torch.native_batch_norm(xx, gamma, beta, rm2, rv2, True, MOM, EPS)
        y = y[:M]
    else:           # one row: torch's unbiased variance would divide by zero; the forward itself is y = beta
        mean, inv = x[0].clone(), torch.full_like(x[0], 1.0) / torch.sqrt(torch.tensor(EPS))
        y = (x - mean) * inv * (gamma if gamma is not None else 1.0) + (beta if beta is not None else 0.0)
        if rm is not None:
            rm2, rv2 = (1 - MOM) * rm + MOM * mean, (1 - MOM) * rv
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return y, torch.cat([mean, inv]), rm2, rv2


def c32_bn_bwd(dy, x, gamma, mask, dup=1):
    """(dx, dgamma, dbeta) by torch's CPU fp32 backward with its own fp32 statistics; the ReLU mask is given"""
    M = x.shape[0]
    d = dy * mask if mask is not None else dy
    dd, xx = (torch.cat([d] * dup), torch.cat([x] * dup)) if dup > 1 else (d, x)
    if M * dup == 1:
        return torch.zeros_like(x), torch.zeros_like(x[0]), d[0].clone()
    _, mean, inv = torch.native_batch_norm(xx, gamma, None, None, None, True, MOM, EPS)
    dx, dg, db = torch.ops.aten.native_batch_norm_backward(dd, xx, gamma, None, None, mean, inv, True, EPS,
                                                           [True, True, True])
    return dx[:M], dg, db


def c32_bwd_sums(dy, x, mean, inv, mask):
    d = dy * mask if mask is not None else dy
    return torch.cat([d.sum(0), (d * ((x - mean) * inv)).sum(0)])


def _ulp(x, up):
    return torch.nextafter(x, torch.full_like(x, float("inf") if up else float("-inf")))


def _edge(mask_gpu, fw, x, gamma, beta, res, what, mask_c32=None):
    """the GPU's ReLU decisions differ from float64's only where |pre64| is within fp32 rounding of zero: the subtraction,
    the product, the fma and the residual add round once each and mean and invstd are fp32 roundings themselves - less than
    8 eps of the magnitudes that make up pre.  At most 1e-4 of the tensor, for the CPU fp32 evaluation as well."""
    pre = fw["pre"]
    g = np.ones(pre.shape[1]) if gamma is None else _np(gamma).astype(np.float64)
    b = np.zeros(pre.shape[1]) if beta is None else _np(beta).astype(np.float64)
    x64 = _np(x).astype(np.float64)
    mag = (np.abs(x64) + np.abs(fw["mean"])) * fw["invstd"] * np.abs(g) + np.abs(b)
    if res is not None:
        mag = mag + np.abs(_np(res).astype(np.float64))
    flips = _np(mask_gpu) != (pre > 0)
    n = int(flips.sum())
    assert n <= 1e-4 * flips.size, "%s: %d of %d ReLU decisions differ from float64's" % (what, n, flips.size)
    assert np.all(np.abs(pre[flips]) <= 8 * EPS32 * mag[flips]), "%s: a decision off the edge differs from float64's" % what
    if mask_c32 is not None:
        n32 = int((_np(mask_c32) != (pre > 0)).sum())
        assert n32 <= 1e-4 * flips.size, "%s: %d of %d CPU fp32 ReLU decisions differ from float64's" % (what, n32, flips.size)
    return n


def _fma_mask(x, mean, inv, gamma, beta):
    """fmaf((x - mean) * inv, gamma, beta) > 0 as fp32 arithmetic takes it: the difference and the product round to fp32, the
    fma's sign is the sign of the exact xh * gamma + beta, which float64 holds (24 x 24 bits) up to one rounding of the sum"""
    xh = ((x - mean) * inv).double()
    return (xh * gamma.double() + beta.double()) > 0


# ------------------------------------------------------------------------------------------------
# a. column reduction
# ------------------------------------------------------------------------------------------------
CR_C = [4, 16, 64, 256, 1024]


def _cr_rows(C):
    rs8 = 256 // (C // 4) * 8                              # rows of one workgroup's sweep
    rows = [1, rs8, rs8 + 1, 32 * rs8 + 1, 258 * rs8 + 1]        # 1, 1, 2, 33 and 259 partials
    return rows + ([512 * rs8 + 3] if C >= 256 else [])    # past the 512-workgroup cap


@functools.lru_cache(maxsize=6)
def _cr_case(C, M):
    g = _gen(31 * C + M)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    dy = torch.randn(M, C, generator=g)
    y = torch.randn(M, C, generator=g)
    mean, inv = torch.randn(C, generator=g) * 0.3 + 0.5, torch.rand(C, generator=g) + 0.25
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    gamma[1], gamma[2] = 0.0, -abs(float(gamma[2])) - 0.1
    mask_y = y > 0
    mask_x, mask_x0 = _fma_mask(x, mean, inv, gamma, beta), _fma_mask(x, mean, inv, torch.ones(C), torch.zeros(C))
    inp = dict(x=x, dy=dy, y=y, save=torch.cat([mean, inv]), gamma=gamma, beta=beta)
    xn, dn, mn, iv = x.numpy(), dy.numpy(), mean.numpy(), inv.numpy()
    ref = dict(stats=(R.bn_sums(xn), torch.cat([x.sum(0), (x * x).sum(0)])),
               colsum=(R.column_sums(dn), dy.sum(0)))
    for key, mask in (("bwd0", None), ("bwd1", mask_y), ("bwdx", mask_x), ("bwdx0", mask_x0)):
        ref[key] = (R.bn_bwd_sums(dn, xn, mn, iv, None if mask is None else mask.numpy()), c32_bwd_sums(dy, x, mean, inv, mask))
    return inp, ref


@pytest.mark.parametrize("C,cap", [(C, cap) for C in CR_C for cap in (None, 1, 2, 3)])
def test_colreduce(C, cap, monkeypatch):
    if cap is not None:
        monkeypatch.setenv("MI_COLREDUCE_BLOCKS", str(cap))
    for M in _cr_rows(C):
        inp, ref = _cr_case(C, M)
        d = {k: _dev(v) for k, v in inp.items()}
        got = dict(stats=g_stats(d["x"], M, C), colsum=g_colsum(d["dy"], M, C),
                   bwd0=g_bwd_reduce(d["dy"], d["x"], None, M, C, d["save"], 0),
                   bwd1=g_bwd_reduce(d["dy"], d["x"], d["y"], M, C, d["save"], 1),
                   bwdx=g_reduce_x(d["dy"], d["x"], M, C, d["save"], d["gamma"], d["beta"]),
                   bwdx0=g_reduce_x(d["dy"], d["x"], M, C, d["save"], None, None))
        for key, val in got.items():
            _eq("colreduce", val, ref[key][1], ref[key][0], "%s C %d M %d cap %s" % (key, C, M, cap))


def test_colreduce_workspace():
    lib = _lib().lib()
    for C in (12, 48, 2048):
        assert lib.mi_colreduce_workspace_bytes(1000, C) == 0
    assert lib.mi_colreduce_workspace_bytes(1, 64) == 8 * 2 * 64
    M, C = 1000, 64                     # 8 workgroups
    n = lib.mi_colreduce_workspace_bytes(M, C)
    assert n == 8 * 2 * C * 8
    x, s, ws = torch.randn(M, C, device="cuda"), _sums(C), torch.empty(n, dtype=torch.uint8, device="cuda")
    assert _call("mi_bn_stats", _p(x), M, C, _p(s), _p(ws), n - 1) == MI_E_WORKSPACE
    assert _call("mi_bn_stats", _p(x), M, C, _p(s), _p(None), n) == MI_E_WORKSPACE
    assert _call("mi_bn_stats", _p(x), M, 12, _p(s), _p(ws), n) == MI_E_ARG
    assert _call("mi_bn_stats", _p(x), M, C, _p(s), _p(ws), n) == 0


@pytest.mark.parametrize("C", [1, 3, 5, 48])
def test_colsum_any_channel_count(C):
    for M in (1, 63, 64, 65, 1000):
        dy = torch.randn(M, C, generator=_gen(C * 1000 + M)) + 0.25
        _eq("colsum_any", g_colsum(_dev(dy), M, C), dy.sum(0), R.column_sums(dy.numpy()), "colsum C %d M %d" % (C, M))


# ------------------------------------------------------------------------------------------------
# b + d. two-launch BatchNorm, forward and backward
# ------------------------------------------------------------------------------------------------
BN_SHAPES = [(1, 4), (1, 1024), (2048, 4), (2049, 4), (8, 1024), (9, 1024), (1000, 64), (777, 256), (2051, 1024)]
BN_VARIANTS = {      # affine, running statistics, residual, relu, count / M
    "full": (True, True, True, True, 1), "plain": (False, False, False, False, 1), "relu": (True, True, False, True, 1),
    "sync2": (True, True, True, True, 2), "sync2-relu": (True, True, False, True, 2)}


def _bn_inputs(M, C, seed, affine=True, running=True, use_res=True):
    g = _gen(seed)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    gamma = torch.randn(C, generator=g)
    gamma[1], gamma[2] = 0.0, -abs(float(gamma[2])) - 0.1          # zero and negative slopes beside the positive ones
    gamma[0] = abs(float(gamma[0])) + 0.1
    beta = torch.randn(C, generator=g) * 0.5
    res, dy = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    return (x, gamma if affine else None, beta if affine else None, res if use_res else None, dy,
            rm if running else None, rv if running else None)


def _check_fwd(group, what, got_y, got_save, got_rm, got_rv, fw, c32, nbt, calls):
    _eq(group, got_y, c32[0], fw["y"], what + " y")
    _eq(group, got_save, c32[1], fw["save"], what + " save")
    if got_rm is not None:
        _eq(group, got_rm, c32[2], fw["running_mean"], what + " running_mean x%d" % calls)
        _eq(group, got_rv, c32[3], fw["running_var"], what + " running_var x%d" % calls)
    assert int(nbt) == 5 + calls, what + ": num_batches_tracked"


@pytest.mark.parametrize("variant", sorted(BN_VARIANTS))
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_two_launch(M, C, variant):
    affine, running, use_res, relu, dup = BN_VARIANTS[variant]
    x, gamma, beta, res, dy, rm, rv = _bn_inputs(M, C, 7 * M + C, affine, running, use_res)
    what = "bn2 (%d, %d) %s" % (M, C, variant)
    count = dup * M
    xd, gd, bd, rd, dyd = _dev(x), _dev(gamma), _dev(beta), _dev(res), _dev(dy)
    rmd, rvd = _dev(rm), _dev(rv)
    nbt = torch.tensor(5, dtype=torch.int64, device="cuda")
    sums = g_stats(xd, M, C) * dup
    # forward, once and twice
    y, save = g_apply(xd, M, C, sums, count, gd, bd, rmd, rvd, nbt, rd, relu)
    fw = R.bn_train_fwd(x.numpy(), _np(gamma) if affine else None, _np(beta) if affine else None, EPS, MOM,
                        _np(rm) if running else None, _np(rv) if running else None, _np(res) if use_res else None, relu, count)
    c32 = c32_bn_fwd(x, gamma, beta, rm, rv, res, relu, dup)
    _check_fwd("bn_two_launch", what, y, save, rmd.clone() if running else None, rvd, fw, c32, nbt, 1)
    y2, save2 = g_apply(xd, M, C, sums, count, gd, bd, rmd, rvd, nbt, rd, relu)
    assert torch.equal(y, y2) and torch.equal(save, save2), what + ": the second call computes something else"
    if running:
        fw2 = R.bn_train_fwd(x.numpy(), None, None, EPS, MOM, fw["running_mean"], fw["running_var"], count=count)
        c32b = c32_bn_fwd(x, None, None, c32[2], c32[3], None, False, dup)
        _eq("bn_two_launch", rmd, c32b[2], fw2["running_mean"], what + " running_mean x2")
        _eq("bn_two_launch", rvd, c32b[3], fw2["running_var"], what + " running_var x2")
    assert int(nbt) == 7, what + ": num_batches_tracked after two calls"
    # eval forward on the running statistics the two calls left (or fresh ones)
    erm, erv = (rmd, rvd) if running else (_dev(torch.randn(C, generator=_gen(1))), _dev(torch.rand(C, generator=_gen(2)) + 0.5))
    ye, se = g_eval(xd, M, C, erm, erv, gd, bd, rd, relu)
    y64, s64 = R.bn_eval_fwd(x.numpy(), _np(erm), _np(erv), _np(gamma) if affine else None, _np(beta) if affine else None, EPS,
                             _np(res) if use_res else None, relu)
    ye32 = F.batch_norm(x, erm.cpu(), erv.cpu(), gamma, beta, False, MOM, EPS)
    ye32 = ye32 + res if use_res else ye32
    _eq("bn_eval", ye, F.relu(ye32) if relu else ye32, y64, what + " eval y")
    _eq("bn_eval", se, torch.cat([erm.cpu(), 1.0 / torch.sqrt(erv.cpu() + EPS)]), s64, what + " eval save")
    # backward, stored-y form: the mask is the GPU forward's
    mask = (y > 0).cpu() if relu else None
    if relu:
        _edge(mask, fw, x, gamma, beta, res, what, c32[0] > 0)
    mean64, inv64 = fw["mean"], fw["invstd"]
    mask_n = None if mask is None else mask.numpy()
    bsum64 = R.bn_bwd_sums(dy.numpy(), x.numpy(), mean64, inv64, mask_n)
    bw = R.bn_bwd(dy.numpy(), x.numpy(), mean64, inv64, _np(gamma) if affine else None, mask_n, sums=dup * bsum64, count=count)
    b32 = c32_bn_bwd(dy, x, gamma, mask, dup)
    bsums = g_bwd_reduce(dyd, xd, y if relu else None, M, C, save, relu)
    _eq("bn_bwd", bsums, c32_bwd_sums(dy, x, c32[1][:C], c32[1][C:], mask), bsum64, what + " backward sums")
    bsums = bsums * dup
    dx, dg, db = g_bwd_apply(dyd, xd, y if relu else None, M, C, save, gd, bsums, count, relu)
    _eq("bn_bwd", dx, b32[0], bw["dx"], what + " dx")
    _eq("bn_bwd", dg, b32[1], bw["dgamma"], what + " dgamma")
    _eq("bn_bwd", db, b32[2], bw["dbeta"], what + " dbeta")
    pg, pb = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _ok("mi_bn_param_grads", _p(bsums), C, _p(pg), _p(pb))
    assert torch.equal(pb, bsums[:C].float()) and torch.equal(pg, bsums[C:].float()), what + ": mi_bn_param_grads"
    assert torch.equal(pb, db) and torch.equal(pg, dg), what + ": the apply's parameter gradients are not the sums"
    if relu:
        dx2, dres, dg2, db2 = g_bwd_apply_res(dyd, xd, y, M, C, save, gd, bsums, count)
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db), what + ": apply_res differs from apply"
        assert torch.equal(dres.cpu(), dy * mask), what + ": dres is not dy * (y > 0)"
    # recomputed-mask form (y = relu(bn(x)) never stored: no residual)
    if relu and not use_res:
        xs = g_reduce_x(dyd, xd, M, C, save, gd, bd)
        assert torch.equal(xs, bsums / dup), what + ": the sums with the recomputed mask differ from the stored-y sums"
        dx3, dg3, db3 = g_apply_x(dyd, xd, M, C, save, gd, bd, bsums, count)
        assert torch.equal(dx3, dx) and torch.equal(dg3, dg) and torch.equal(db3, db), what + ": apply_x differs from apply"
        # dy of ones and zero sums: dx / (gamma * invstd) IS the mask the backward took
        ones, zeros = torch.ones_like(xd), torch.zeros(2 * C, dtype=torch.float64, device="cuda")
        dxm, _, _ = g_apply_x(ones, xd, M, C, save, gd, bd, zeros, count)
        live = (gamma != 0).numpy()
        assert np.array_equal(_np(dxm != 0)[:, live], mask.numpy()[:, live]), what + ": apply_x took other ReLU decisions"
        assert np.array_equal(_np(dxm)[:, live], (mask.float() * (gd * save[C:]).cpu()).numpy()[:, live])
        cnt = g_reduce_x(ones, xd, M, C, save, gd, bd)
        assert np.array_equal(_np(cnt[:C]), mask.double().sum(0).numpy()), what + ": reduce_x took other ReLU decisions"


# ------------------------------------------------------------------------------------------------
# c. one-launch BatchNorm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 12, 48, 256])
@pytest.mark.parametrize("M", [1, 2, 255, 256, 257, 630, 4096])
def test_bn_small(M, C):
    for affine, running, use_res, relu in ((True, True, True, True), (False, False, False, False)):
        x, gamma, beta, res, dy, rm, rv = _bn_inputs(M, C, 11 * M + C, affine, running, use_res)
        what = "bn_small (%d, %d)%s" % (M, C, "" if affine else " plain")
        xd, gd, bd, rd, dyd, rmd, rvd = _dev(x), _dev(gamma), _dev(beta), _dev(res), _dev(dy), _dev(rm), _dev(rv)
        nbt = torch.tensor(5, dtype=torch.int64, device="cuda")
        y, save = g_small_fwd(xd, M, C, gd, bd, rmd, rvd, nbt, rd, relu)
        fw = R.bn_train_fwd(x.numpy(), _np(gamma) if affine else None, _np(beta) if affine else None, EPS, MOM,
                            _np(rm) if running else None, _np(rv) if running else None, _np(res) if use_res else None, relu)
        c32 = c32_bn_fwd(x, gamma, beta, rm, rv, res, relu)
        _check_fwd("bn_small", what, y, save, rmd, rvd, fw, c32, nbt, 1)
        mask = (y > 0).cpu() if relu else None
        if relu:
            _edge(mask, fw, x, gamma, beta, res, what, c32[0] > 0)
        mask_n = None if mask is None else mask.numpy()
        bw = R.bn_bwd(dy.numpy(), x.numpy(), fw["mean"], fw["invstd"], _np(gamma) if affine else None, mask_n)
        b32 = c32_bn_bwd(dy, x, gamma, mask)
        dx, dg, db = g_small_bwd(dyd, xd, y if relu else None, M, C, save, gd, relu)
        _eq("bn_small", dx, b32[0], bw["dx"], what + " dx")
        _eq("bn_small", dg, b32[1], bw["dgamma"], what + " dgamma")
        _eq("bn_small", db, b32[2], bw["dbeta"], what + " dbeta")
        if _cr_ok(C):        # the two-launch path on the same inputs meets float64 on its own
            rm2, rv2 = _dev(rm), _dev(rv)
            nbt2 = torch.tensor(5, dtype=torch.int64, device="cuda")
            y2, save2 = g_apply(xd, M, C, g_stats(xd, M, C), M, gd, bd, rm2, rv2, nbt2, rd, relu)
            _check_fwd("bn_two_launch", what + " two-launch", y2, save2, rm2, rv2, fw, c32, nbt2, 1)


@pytest.mark.parametrize("V", [1, 2, 8, 64])
def test_bn_small_pool(V):
    for C in (4, 12):
        for M in (V, 3 * V, {1: 321, 2: 322, 8: 328, 64: 448}[V]):
            x, gamma, beta, _, _, rm, rv = _bn_inputs(M, C, 13 * M + C + V)
            dp = torch.randn(M // V, C, generator=_gen(M + V))
            what = "bn_small_pool (%d, %d) V %d" % (M, C, V)
            xd, gd, bd, rmd, rvd = _dev(x), _dev(gamma), _dev(beta), _dev(rm), _dev(rv)
            nbt = torch.tensor(5, dtype=torch.int64, device="cuda")
            y, pooled, save = g_small_pool_fwd(xd, M, C, V, gd, bd, rmd, rvd, nbt)
            fw = R.bn_train_fwd(x.numpy(), gamma.numpy(), beta.numpy(), EPS, MOM, rm.numpy(), rv.numpy(), None, True)
            c32 = c32_bn_fwd(x, gamma, beta, rm, rv, None, True)
            _check_fwd("bn_small_pool", what, y, save, rmd, rvd, fw, c32, nbt, 1)
            _eq("bn_small_pool", pooled, c32[0].reshape(M // V, V, C).mean(1), R.avgpool_fwd(fw["y"].reshape(M // V, V, C)),
                what + " pooled")
            # the pooled output is the plain pool of the y it wrote, rows added in order
            y3 = y.reshape(M // V, V, C)
            acc = y3[:, 0].clone()
            for k in range(1, V):
                acc += y3[:, k]
            assert torch.equal(pooled, acc / float(V)), what + ": pooled is not the row-ordered mean of y"
            mask = (y > 0).cpu()
            _edge(mask, fw, x, gamma, beta, None, what, c32[0] > 0)
            d64 = R.avgpool_bwd(dp.numpy(), V).reshape(M, C)
            d32 = (dp[:, None, :] / V).expand(M // V, V, C).reshape(M, C)
            bw = R.bn_bwd(d64, x.numpy(), fw["mean"], fw["invstd"], gamma.numpy(), mask.numpy())
            b32 = c32_bn_bwd(d32, x, gamma, mask)
            dx, dg, db = g_small_pool_bwd(_dev(dp), xd, y, M, C, V, save, gd)
            _eq("bn_small_pool", dx, b32[0], bw["dx"], what + " dx")
            _eq("bn_small_pool", dg, b32[1], bw["dgamma"], what + " dgamma")
            _eq("bn_small_pool", db, b32[2], bw["dbeta"], what + " dbeta")


def test_bn_small_refuses_4097_rows():
    M, C = 4097, 4
    x = torch.zeros(M, C, device="cuda")
    y, save, g = torch.zeros_like(x), torch.zeros(2 * C, device="cuda"), torch.ones(C, device="cuda")
    pooled = torch.zeros(M, C, device="cuda")
    assert _call("mi_bn_small_fwd", _p(x), _p(y), M, C, _p(g), _p(g), EPS, MOM, None, None, None, _p(save), None, 0) == MI_E_ARG
    assert _call("mi_bn_small_bwd", _p(x), _p(x), _p(y), _p(y), M, C, _p(save), _p(g), 0, None, None) == MI_E_ARG
    assert _call("mi_bn_small_pool_fwd", _p(x), _p(y), _p(pooled), M, C, 1, _p(g), _p(g), EPS, MOM, None, None, None,
                 _p(save)) == MI_E_ARG
    assert _call("mi_bn_small_pool_bwd", _p(pooled), _p(x), _p(y), _p(y), M, C, 1, _p(save), _p(g), None, None) == MI_E_ARG
    # V must be a power of two <= 64 that divides M
    for M2, V in ((12, 3), (128, 128), (6, 4)):
        assert _call("mi_bn_small_pool_fwd", _p(x), _p(y), _p(pooled), M2, C, V, _p(g), _p(g), EPS, MOM, None, None, None,
                     _p(save)) == MI_E_ARG


# ------------------------------------------------------------------------------------------------
# e. conditioning: columns whose mean is large against their spread
# ------------------------------------------------------------------------------------------------
RATIOS = [0, 1, 4, 16, 64, "const"]


def _cond_inputs(M, C):
    g = _gen(M + C)
    x = torch.randn(M, C, generator=g)
    for c in range(C):
        r = RATIOS[c % 6]
        x[:, c] = 3.7 if r == "const" else x[:, c] + float(r)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    dy = torch.randn(M, C, generator=g)
    rm, rv = torch.zeros(C), torch.ones(C)
    return x, gamma, beta, dy, rm, rv


@pytest.mark.parametrize("path,M,C,cap", [("small", 4096, 24, None), ("two", 4096, 64, None), ("two", 65536, 64, None),
                                          ("two", 65536, 64, 8)])
def test_bn_conditioning(path, M, C, cap, monkeypatch):
    if cap is not None:
        monkeypatch.setenv("MI_COLREDUCE_BLOCKS", str(cap))
    x, gamma, beta, dy, rm, rv = _cond_inputs(M, C)
    xd, gd, bd, dyd, rmd, rvd = _dev(x), _dev(gamma), _dev(beta), _dev(dy), _dev(rm), _dev(rv)
    nbt = torch.tensor(0, dtype=torch.int64, device="cuda")
    if path == "small":
        y, save = g_small_fwd(xd, M, C, gd, bd, rmd, rvd, nbt, None, 0)
        dx, _, _ = g_small_bwd(dyd, xd, None, M, C, save, gd, 0)
    else:
        y, save = g_apply(xd, M, C, g_stats(xd, M, C), M, gd, bd, rmd, rvd, nbt, None, 0)
        dx, _, _ = g_bwd_apply(dyd, xd, None, M, C, save, gd, g_bwd_reduce(dyd, xd, None, M, C, save, 0), M, 0)
    fw = R.bn_train_fwd(x.numpy(), gamma.numpy(), beta.numpy(), EPS, MOM, rm.numpy(), rv.numpy())
    bw = R.bn_bwd(dy.numpy(), x.numpy(), fw["mean"], fw["invstd"], gamma.numpy())
    evals = []                   # three fp32 evaluations: the inputs as they are, one ulp up, one ulp down
    for xe in (x, _ulp(x, True), _ulp(x, False)):
        evals.append(c32_bn_fwd(xe, gamma, beta, rm, rv, None, False) + (c32_bn_bwd(dy, xe, gamma, None)[0],))
    group = "cond_" + path
    for gi, r in enumerate(RATIOS):
        cols = np.arange(gi, C, 6)
        scols = np.concatenate([cols, C + cols])
        what = "%s M %d cap %s ratio %s" % (path, M, cap, r)
        _eq(group, _np(y)[:, cols], _np(evals[0][0])[:, cols], fw["y"][:, cols], what + " y",
            more=[_np(e[0])[:, cols] for e in evals[1:]])
        _eq(group, _np(save)[scols], _np(evals[0][1])[scols], fw["save"][scols], what + " save",
            more=[_np(e[1])[scols] for e in evals[1:]])
        _eq(group, _np(rvd)[cols], _np(evals[0][3])[cols], fw["running_var"][cols], what + " running_var",
            more=[_np(e[3])[cols] for e in evals[1:]])
        _eq(group, _np(dx)[:, cols], _np(evals[0][4])[:, cols], bw["dx"][:, cols], what + " dx",
            more=[_np(e[4])[:, cols] for e in evals[1:]])


# ------------------------------------------------------------------------------------------------
# f. pooling
# ------------------------------------------------------------------------------------------------
def _pool_input(kind, shape, seed):
    x = torch.randn(*shape, generator=_gen(seed))
    if kind == "relu":
        x = F.relu(x)                              # many exact-zero ties
    elif kind == "negative":
        x = -x.abs() - 0.5                          # padding must never win
    elif kind == "constant":
        x = torch.full(shape, 1.25)                 # every window ties
    elif kind == "nan":
        x[0, shape[1] // 2, shape[2] // 2, shape[3] // 2, 1] = float("nan")
    return x


def _pool_check(x, k, s, p, what, check_null_arg=True):
    shape = tuple(x.shape)
    y64, arg64 = R.maxpool3d_fwd(x.numpy(), k, s, p)
    xd = _dev(x)
    y, arg = g_maxpool_fwd(xd, k, s, p)
    assert np.array_equal(_np(y), y64.astype(np.float32), equal_nan=True), what + ": maxima"
    assert np.array_equal(_np(arg), arg64), what + ": argmax taps"
    if check_null_arg:
        y0, _ = g_maxpool_fwd(xd, k, s, p, want_arg=False)
        assert np.array_equal(_np(y0), _np(y), equal_nan=True), what + ": maxima without argmax"
    dy = torch.randint(-4, 5, y.shape, generator=_gen(5)).float()
    dx64 = R.maxpool3d_bwd(dy.numpy(), arg64, shape[1:4], k, s, p)
    xt = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    F.max_pool3d(xt, k, s, p).backward(dy.permute(0, 4, 1, 2, 3).contiguous())
    dx32 = xt.grad.permute(0, 2, 3, 4, 1)
    dyd = _dev(dy)
    dx = g_maxpool_bwd(dyd, arg, shape, k, s, p)
    _eq("maxpool_bwd", dx, dx32, dx64, what + " dx")
    return dyd, arg, dx, dx32, dx64


@pytest.mark.parametrize("k,s,p", POOLS)
def test_maxpool3d(k, s, p):
    for vol in ((2, 5, 7, 6), (1, 4, 4, 4)):
        for C in (4, 12, 16, 64):
            for kind in ("random", "relu", "negative", "constant", "nan"):
                _pool_check(_pool_input(kind, vol + (C,), k + s + p + C), k, s, p,
                            "maxpool k%d s%d p%d %s C %d %s" % (k, s, p, vol, C, kind), check_null_arg=kind == "random")


@pytest.mark.parametrize("Wi,C", [(16, 64), (64, 16)])
def test_maxpool3d_bwd_k3s2_bands(Wi, C, monkeypatch):
    """the stem's plane kernel (Wi * C / 4 == 256) at odd Hi and Di, with its default band, bands of 2 and 6 rows, one band
    taller than the plane, and the generic kernel: all against float64, and bit-identical among themselves"""
    x = _pool_input("relu", (2, 5, 7, Wi, C), Wi + C)
    outs = []
    for env in ({}, {"MI_MAXPOOL_BWD_BAND": "2"}, {"MI_MAXPOOL_BWD_BAND": "6"}, {"MI_MAXPOOL_BWD_BAND": "8"},
                {"MI_MAXPOOL_BWD_GENERIC": "1"}):
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            outs.append(_pool_check(x, 3, 2, 1, "k3s2 Wi %d C %d %s" % (Wi, C, env), check_null_arg=False)[2])
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize("k,s,p", POOLS)
def test_bn_relu_maxpool_fused(k, s, p):
    for vol in ((2, 5, 7, 6), (1, 4, 4, 4)):
        for C in (4, 16, 64):
            shape = vol + (C,)
            M = int(np.prod(vol))
            x, gamma, beta, _, _, rm, rv = _bn_inputs(M, C, k + s + p + C)
            x5 = x.reshape(shape)
            what = "fused k%d s%d p%d %s C %d" % (k, s, p, vol, C)
            xd, gd, bd = _dev(x5), _dev(gamma), _dev(beta)
            sums = g_stats(xd, M, C)
            for train in (True, False):
                w = what + (" train" if train else " eval")
                rm1, rv1, rm2, rv2 = _dev(rm), _dev(rv), _dev(rm), _dev(rv)
                nbt1, nbt2 = (torch.tensor(5, dtype=torch.int64, device="cuda") for _ in range(2))
                y, arg, save = g_fused(xd, k, s, p, sums if train else None, M, gd, bd, rm1, rv1, nbt1 if train else None)
                # the composition: two-launch BatchNorm + ReLU, then the plain pool - the same arithmetic, bit for bit
                if train:
                    act, save2 = g_apply(xd.reshape(M, C), M, C, sums, M, gd, bd, rm2, rv2, nbt2, None, 1)
                    assert torch.equal(save, save2) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2), w + ": statistics"
                    assert int(nbt1) == 6 and int(nbt2) == 6, w + ": num_batches_tracked"
                else:
                    act, _ = g_eval(xd.reshape(M, C), M, C, rm2, rv2, gd, bd, None, 1)
                    assert torch.equal(rm1, _dev(rm)) and torch.equal(rv1, _dev(rv)), w + ": eval mode wrote the statistics"
                yc, argc = g_maxpool_fwd(act.reshape(shape), k, s, p)
                assert torch.equal(y, yc), w + ": pooled values differ from the composition"
                assert torch.equal(arg, argc), w + ": argmax taps differ from the composition"
                y0, _, _ = g_fused(xd, k, s, p, sums if train else None, M, gd, bd, _dev(rm), _dev(rv), None, want_arg=False)
                assert torch.equal(y0, y), w + ": pooled values without argmax"
                # float64
                y64, arg64, bn = R.bn_relu_maxpool_fwd(x5.numpy(), k, s, p, gamma.numpy(), beta.numpy(), EPS, MOM, rm.numpy(),
                                                       rv.numpy(), train)
                xt = x5.permute(0, 4, 1, 2, 3).contiguous()
                a32 = F.relu(F.batch_norm(xt, rm.clone(), rv.clone(), gamma, beta, train, MOM, EPS))
                _eq("fused_pool", y, F.max_pool3d(a32, k, s, p).permute(0, 2, 3, 4, 1), y64, w + " pooled")
                # gamma == 0 in channel 1: relu(beta) everywhere, every window ties and the first tap inside the volume wins
                assert np.array_equal(_np(arg)[..., 1], arg64[..., 1]), w + ": ties"
                if train:
                    c32 = c32_bn_fwd(x, gamma, beta, rm, rv, None, True)
                    _check_fwd("fused_pool", w, act, save, rm1, rv1, bn, c32, nbt1, 1)


def test_bn_relu_maxpool_fused_nan():
    """eval mode (a NaN in training mode is in the statistics and so in every voxel of its channel): the NaN comes out of
    every window that holds it, as float64's maximum does"""
    shape, C = (2, 5, 7, 6, 4), 4
    M = int(np.prod(shape[:4]))
    x, gamma, beta, _, _, rm, rv = _bn_inputs(M, C, 3)
    x5 = x.reshape(shape).clone()
    x5[1, 2, 3, 3, 0] = float("nan")
    for k, s, p in ((3, 2, 1), (2, 2, 0), (5, 2, 2)):
        y, arg, _ = g_fused(_dev(x5), k, s, p, None, M, _dev(gamma), _dev(beta), _dev(rm), _dev(rv), None)
        y64, arg64, _ = R.bn_relu_maxpool_fwd(x5.numpy(), k, s, p, gamma.numpy(), beta.numpy(), EPS, MOM, rm.numpy(), rv.numpy(),
                                              False)
        assert np.array_equal(np.isnan(_np(y)), np.isnan(y64)) and np.isnan(y64).sum() >= 1
        assert np.array_equal(_np(arg)[np.isnan(y64)], arg64[np.isnan(y64)])


def test_pool_refusals():
    C = 4
    x = torch.zeros(1, 4, 4, 4, 8, device="cuda")
    y, arg = torch.zeros_like(x), torch.zeros(x.shape, dtype=torch.uint8, device="cuda")
    rm, rv, save = torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"), torch.zeros(16, device="cuda")
    for (D, Cc, k, s, p), why in (((4, C, 7, 2, 3), "k = 7"), ((4, C, 3, 2, -1), "pad < 0"), ((4, 6, 3, 2, 1), "C = 6"),
                                  ((2, C, 3, 2, 0), "no output voxel")):
        assert _call("mi_maxpool3d_fwd", _p(x), _p(y), _p(arg), 1, D, D, D, Cc, k, s, p) == MI_E_ARG, why
        assert _call("mi_maxpool3d_bwd", _p(y), _p(arg), _p(x), 1, D, D, D, Cc, k, s, p) == MI_E_ARG, why
        assert _call("mi_bn_relu_maxpool3d_fwd", _p(x), _p(y), _p(arg), 1, D, D, D, Cc, k, s, p, None, 1.0, None, None, EPS, MOM,
                     _p(rm), _p(rv), None, _p(save)) == MI_E_ARG, why


@pytest.mark.parametrize("B,S,C", [(1, 1, 1), (3, 8, 5), (5, 63, 12), (2, 512, 64), (300, 7, 3)])
def test_avgpool(B, S, C):
    x = torch.randn(B, S, C, generator=_gen(B + S + C)) + 0.5
    dy = torch.randn(B, C, generator=_gen(B * S))
    y, dx = torch.empty(B, C, device="cuda"), torch.empty(B, S, C, device="cuda")
    _ok("mi_avgpool_fwd", _p(_dev(x)), _p(y), B, S, C)
    _ok("mi_avgpool_bwd", _p(_dev(dy)), _p(dx), B, S, C)
    xt = x.permute(0, 2, 1).reshape(B, C, S, 1, 1).contiguous().requires_grad_(True)
    y32 = F.adaptive_avg_pool3d(xt, 1).flatten(1)
    y32.backward(dy)
    what = "avgpool (%d, %d, %d)" % (B, S, C)
    _eq("avgpool", y, y32.detach(), R.avgpool_fwd(x.numpy()), what + " y")
    _eq("avgpool", dx, xt.grad.reshape(B, C, S).permute(0, 2, 1), R.avgpool_bwd(dy.numpy(), S), what + " dx")
