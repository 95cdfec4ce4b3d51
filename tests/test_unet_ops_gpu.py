"""csrc/unet_ops.hip - the detector network's glue: the ceil-mode 2-D max pool, the 2x2 transposed convolution's shuffle and
un-shuffle, the fused up-convolution tail, concat / split / copy-into-slice, the (3,1,1) head with its two backward kernels and
the 7x7 one-channel first layer - each against the plain float64 restatement in tests/unet_ops_ref.py (proven against torch by
tests/test_unet_ops_ref_cpu.py), through the C entries, at small ragged shapes, at every size where an entry takes another
kernel, and at the smallest sizes that send a grid-stride loop on its second trip.

Numeric results (the head's forward and both gradients, the tail's first Co channels, the first layer) go through
conftest.f32_equivalent with its defaults: the GPU may lie as far from float64 as twice torch's CPU float32 evaluation of the
same inputs does, plus the default floor.  Pooled maxima, argmax bytes, the pool's backward, shuffle, un-shuffle, concat, split,
copy-into-slice and the tail's encoder half are moves: compared bit for bit.  Shuffle with a bias is one fp32 add per element:
compared bit for bit with numpy's fp32 add.

Not tested: the lane-group head kernel's own grid cap of 2^20 blocks (zhead_rows_kernel: 2^20 * 256 / (C / 4) voxels of C floats,
4 GB of input at C = 16 and more above) - its stride loop makes one trip in every case here."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ops_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu

MI_E_ARG, MI_E_WORKSPACE, MI_E_UNSUPPORTED = -1, -2, -3
EW_CAP = 4096 * 256                        # ew_blocks: at most 4096 workgroups of 256 threads, one float4 item each per trip
ZW_CAP = 1024                              # zhead_w_blocks: at most 1024 workgroups
ERRORS = {}                                # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64]
SENTINEL = -7.25
HW = [(6, 5), (1, 1), (1, 9)]


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
    if t is None:
        return None
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def _wide(g, *shape):
    """a wide dynamic range, as tests/test_train_gpu.py draws it"""
    return torch.randn(*shape, generator=g) * torch.exp(2 * torch.randn(*shape, generator=g))


def _eq(group, got, cpu32, ref64, what):
    from conftest import f32_equivalent
    e_g, e_c = f32_equivalent(_np(got), _np(cpu32), _np(ref64), what=what)
    print("%-12s %-64s GPU %.3e  CPU fp32 %.3e" % (group, what, e_g, e_c))
    rec = ERRORS.setdefault(group, [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], e_g), max(rec[1], e_c)
    return e_g, e_c


def _same(got, want, what):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), what + ": not bit for bit"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, (e_g, e_c) in sorted(ERRORS.items()):
        print("\nlargest error, %-12s GPU %.3e  CPU fp32 %.3e" % (group, e_g, e_c))


# ------------------------------------------------------------------------------------------------
# the C entries, one thin wrapper each (device tensors in, device tensors out; outputs pre-filled so that an element the
# kernel leaves out shows)
# ------------------------------------------------------------------------------------------------
def g_pool_fwd(x, k, want_arg=True):
    N, Hi, Wi, C = x.shape
    y = torch.full((N, R.ceil_div(Hi, k), R.ceil_div(Wi, k), C), SENTINEL, device="cuda")
    arg = torch.full(y.shape, 255, dtype=torch.uint8, device="cuda") if want_arg else None
    _ok("mi_maxpool2d_ceil_fwd", _p(x), _p(y), _p(arg), N, Hi, Wi, C, k)
    return y, arg


def g_pool_bwd(dy, arg, shape, k):
    N, Hi, Wi, C = shape
    dx = torch.full(shape, float("nan"), device="cuda")
    _ok("mi_maxpool2d_ceil_bwd", _p(dy), _p(arg), _p(dx), N, Hi, Wi, C, k)
    return dx


def g_shuffle(t, bias, Ho, Wo):
    N, H, W, C4 = t.shape
    y = torch.full((N, Ho, Wo, C4 // 4), float("nan"), device="cuda")
    _ok("mi_shuffle2x2_fwd", _p(t), _p(bias), _p(y), N, H, W, C4 // 4, Ho, Wo)
    return y


def g_unshuffle(dy, H, W):
    N, Ho, Wo, Co = dy.shape
    dt = torch.full((N, H, W, 4 * Co), float("nan"), device="cuda")
    _ok("mi_shuffle2x2_bwd", _p(dy), _p(dt), N, H, W, Co, Ho, Wo)
    return dt


def g_tail(t, scale, shift, enc, Ho, Wo):
    N, H, W, C4 = t.shape
    Co, Ce = C4 // 4, enc.shape[-1]
    out = torch.full((N, Ho, Wo, Co + Ce), float("nan"), device="cuda")
    _ok("mi_upconv_tail_fwd", _p(t), _p(scale), _p(shift), _p(enc), _p(out), N, H, W, Co, Ce, Ho, Wo)
    return out


def g_concat(a, b):
    out = torch.full((a.shape[0], a.shape[1] + b.shape[1]), float("nan"), device="cuda")
    _ok("mi_concat_channels", _p(a), a.shape[1], _p(b), b.shape[1], _p(out), a.shape[0])
    return out


def g_split(dout, Ca, Cb):
    M = dout.shape[0]
    da, db = torch.full((M, Ca), float("nan"), device="cuda"), torch.full((M, Cb), float("nan"), device="cuda")
    _ok("mi_split_channels", _p(dout), _p(da), Ca, _p(db), Cb, M)
    return da, db


def g_copy_into(src, dst, c0):
    _ok("mi_copy_channels_into", _p(src), src.shape[1], _p(dst), dst.shape[1], c0, src.shape[0])
    return dst


def g_zhead(x, w):
    N, D, P, C = x.shape
    K = w.shape[2]
    y = torch.full((N, D, P, K), float("nan"), device="cuda")
    _ok("mi_zhead_fwd", _p(x), _p(w), _p(y), N, D, P, C, K)
    return y


def zhead_ws_bytes(N, D, P, C, K):
    return _lib().lib().mi_zhead_bwd_workspace_bytes(N, D, P, C, K)


def g_zhead_bwd(x, w, dy, want_dx=True, want_dw=True, dw=None):
    """the workspace holds NaN bytes before the call: a partial sum that is read without having been written shows"""
    N, D, P, C = x.shape
    K = w.shape[2]
    n = zhead_ws_bytes(N, D, P, C, K)
    assert n > 0
    ws = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    dx = torch.full(x.shape, float("nan"), device="cuda") if want_dx else None
    if want_dw and dw is None:
        dw = torch.full((3, C, K), float("nan"), device="cuda")
    _ok("mi_zhead_bwd", _p(x), _p(w), _p(dy), _p(dx), _p(dw if want_dw else None), N, D, P, C, K, _p(ws), n)
    return dx, (dw if want_dw else None)


def g_stem(x, w, bias, relu):
    N, H, W = x.shape
    y = torch.full((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16), float("nan"), device="cuda")
    _ok("mi_stem2d_fwd_bias_f32", _p(x), _p(w), _p(bias), _p(y), int(relu), N, H, W)
    return y


def test_every_entry_of_the_file_is_called_here():
    """the extern "C" names of csrc/unet_ops.hip, as _lib.SIGNATURES lists them, against the names this file's wrappers call"""
    L = _lib()
    src = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc", "unet_ops.hip")
    with open(src) as f:
        exported = set(re.findall(r'extern "C" \w+ (mi_\w+)\(', f.read()))
    entries = sorted(n for n in L.SIGNATURES if n in exported)
    assert set(entries) == exported and len(entries) == 12, (entries, sorted(exported))
    with open(os.path.abspath(__file__)) as f:
        mine = f.read()
    called = set(re.findall(r'_(?:ok|call)\("(mi_\w+)"', mine)) | set(re.findall(r"lib\(\)\.(mi_\w+)\(", mine))
    assert not [n for n in entries if n not in called], [n for n in entries if n not in called]


# ------------------------------------------------------------------------------------------------
# max pool
# ------------------------------------------------------------------------------------------------
def _pool_case(x, k, what, null_arg=False):
    """x: fp32 numpy (N, Hi, Wi, C).  Maxima, argmax bytes and the backward are moves: bit for bit."""
    y_ref, arg_ref = R.maxpool2d_ceil(x, k)
    xd = _dev(x)
    y, arg = g_pool_fwd(xd, k)
    _same(y, y_ref, what + " maxima")
    _same(arg, arg_ref, what + " argmax taps")
    if null_arg:
        y0, _ = g_pool_fwd(xd, k, want_arg=False)
        _same(y0, y_ref, what + " maxima with argmax = NULL")
    dy = _wide(_gen(5), *y_ref.shape).numpy()
    dx = g_pool_bwd(_dev(dy), arg, x.shape, k)
    _same(dx, R.maxpool2d_ceil_bwd(dy, arg_ref, x.shape, k), what + " dx")


def _pool_images(k):
    return [(16, 16), (13, 9), (1, 7)] + ([(2, 2)] if k == 3 else []) + ([(31, 46)] if k == 15 else [])


@pytest.mark.parametrize("k", [1, 2, 3, 5, 15])
def test_maxpool2d_ceil(k):
    for Hi, Wi in _pool_images(k):
        for C in (4, 8, 20, 64):
            for kind in R.POOL_KINDS:
                for N in (1, 3) if kind in ("random", "negative") else (3,):
                    x = R.pool_input(kind, (N, Hi, Wi, C), k, 100 * k + Hi + C, np.float32)
                    _pool_case(x, k, "k %d (%d, %d, %d, %d) %s" % (k, N, Hi, Wi, C, kind), null_arg=kind == "random")
    if k == 15:                                  # the largest tap there is: 14 * 15 + 14
        x = R.pool_input("random", (1, 31, 46, 4), 15, 1, np.float32)
        x[0, 14, 14, :] = 100.0
        assert int(g_pool_fwd(_dev(x), 15)[1][0, 0, 0, 0]) == 224


def test_maxpool2d_ceil_second_trip():
    N, Hi, Wi, C, k = 2, 257, 259, 128, 2
    fwd_items = N * R.ceil_div(Hi, k) * R.ceil_div(Wi, k) * (C // 4)
    bwd_items = N * Hi * Wi * (C // 4)
    assert fwd_items == 1073280 and EW_CAP < fwd_items < 2 * EW_CAP and bwd_items > 4 * EW_CAP
    x = torch.randn(N, Hi, Wi, C, generator=_gen(1)).numpy()
    _pool_case(x, k, "second trip")


def test_maxpool2d_ceil_refusals():
    """every one returns from the argument check: nothing is launched and the outputs keep their sentinel"""
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    y = torch.full((1, 4, 4, 8), SENTINEL, device="cuda")
    arg = torch.full((1, 4, 4, 8), 255, dtype=torch.uint8, device="cuda")
    for (N, C, k), why in (((1, 8, 0), "k = 0"), ((1, 8, 16), "k = 16"), ((1, 6, 2), "C = 6"), ((0, 8, 2), "N = 0")):
        assert _call("mi_maxpool2d_ceil_fwd", _p(x), _p(y), _p(arg), N, 4, 4, C, k) == MI_E_ARG, why
        assert _call("mi_maxpool2d_ceil_bwd", _p(x), _p(arg), _p(y), N, 4, 4, C, k) == MI_E_ARG, why
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((arg == 255).all())


# ------------------------------------------------------------------------------------------------
# the shuffle pair
# ------------------------------------------------------------------------------------------------
def _one_hot(Co):
    """conv_transpose2d weights (4 * Co, Co, 2, 2) that route column (a * 2 + b) * Co + co of the 1x1 product to tap (a, b) of
    channel co: the transposed convolution as a function of its 1x1 product"""
    eye = torch.zeros(4 * Co, Co, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for co in range(Co):
                eye[(a * 2 + b) * Co + co, co, a, b] = 1.0
    return eye


def _crops(H, W):
    return [(Ho, Wo) for Ho in (2 * H, 2 * H - 1) for Wo in (2 * W, 2 * W - 1)]


@pytest.mark.parametrize("Co", [4, 16, 36])
@pytest.mark.parametrize("H,W", HW)
def test_shuffle2x2_pair(H, W, Co):
    N = 2
    eye = _one_hot(Co)
    for Ho, Wo in _crops(H, W):
        what = "shuffle (%d, %d) -> (%d, %d) Co %d" % (H, W, Ho, Wo, Co)
        g = _gen(H + 10 * W + 100 * Co + Ho + Wo)
        t, bias, dy = _wide(g, N, H, W, 4 * Co), _wide(g, Co), _wide(g, N, Ho, Wo, Co)
        td = _dev(t)
        moved = R.shuffle2x2(t.numpy(), None, Ho, Wo)
        _same(g_shuffle(td, None, Ho, Wo), moved, what + " bias NULL")
        _same(g_shuffle(td, _dev(bias), Ho, Wo), moved + bias.numpy(), what + " + bias (one fp32 add)")
        # backward: the float64 autograd gradient of F.conv_transpose2d with respect to its 1x1 product
        t64 = t.double().requires_grad_(True)
        y64 = F.conv_transpose2d(t64.permute(0, 3, 1, 2), eye, bias.double(), stride=2)[:, :, :Ho, :Wo]
        (dt64,) = torch.autograd.grad(y64, t64, dy.double().permute(0, 3, 1, 2))
        dt = g_unshuffle(_dev(dy), H, W)                     # into a buffer of NaN
        assert np.array_equal(_np(dt).astype(np.float64), dt64.numpy()), what + ": un-shuffle is not the gradient"
        _same(dt, R.unshuffle2x2(dy.numpy(), H, W), what + " un-shuffle")
        if Ho < 2 * H:
            assert bool((dt[:, H - 1, :, 2 * Co:] == 0).all()), what + ": the cropped row is not zero"
        if Wo < 2 * W:
            assert bool((dt[:, :, W - 1, Co:2 * Co] == 0).all()) and bool((dt[:, :, W - 1, 3 * Co:] == 0).all()), what


def test_shuffle2x2_second_trip():
    N, H, W, Co, Ho, Wo = 1, 129, 130, 64, 257, 259
    fwd_items, bwd_items = N * Ho * Wo * (Co // 4), N * H * W * 4 * (Co // 4)
    assert fwd_items == 1065008 and bwd_items == 1073280 and min(fwd_items, bwd_items) > EW_CAP
    g = _gen(2)
    t, bias, dy = torch.randn(N, H, W, 4 * Co, generator=g), torch.randn(Co, generator=g), torch.randn(N, Ho, Wo, Co, generator=g)
    moved = R.shuffle2x2(t.numpy(), None, Ho, Wo)
    _same(g_shuffle(_dev(t), None, Ho, Wo), moved, "second trip, bias NULL")
    _same(g_shuffle(_dev(t), _dev(bias), Ho, Wo), moved + bias.numpy(), "second trip + bias")
    _same(g_unshuffle(_dev(dy), H, W), R.unshuffle2x2(dy.numpy(), H, W), "second trip un-shuffle")


def test_shuffle2x2_refusals():
    H, W, Co = 3, 3, 8
    t = torch.zeros(1, H, W, 4 * Co, device="cuda")
    y = torch.full((1, 2 * H + 1, 2 * W, Co), SENTINEL, device="cuda")
    dt = torch.full((1, H, W, 4 * Co), SENTINEL, device="cuda")
    for (co, Ho), why in (((Co, 2 * H + 1), "Ho = 2H + 1"), ((6, 2 * H), "Co = 6")):
        assert _call("mi_shuffle2x2_fwd", _p(t), None, _p(y), 1, H, W, co, Ho, 2 * W) == MI_E_ARG, why
        assert _call("mi_shuffle2x2_bwd", _p(y), _p(dt), 1, H, W, co, Ho, 2 * W) == MI_E_ARG, why
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((dt == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# the fused up-convolution tail
# ------------------------------------------------------------------------------------------------
def _tail_case(N, H, W, Ho, Wo, Co, Ce, what, wide=True):
    g = _gen(N + H + 10 * W + Ho + Wo + Co + Ce)
    draw = _wide if wide else (lambda g, *s: torch.randn(*s, generator=g))
    t, enc = draw(g, N, H, W, 4 * Co), draw(g, N, Ho, Wo, Ce)
    scale, shift = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    scale[0], scale[1], shift[1] = -abs(float(scale[0])) - 0.1, 0.0, 0.3         # a negative slope; a dead channel at relu(0.3)
    scale[2], shift[2] = 0.0, -0.3                                                # and one dead at zero
    out = g_tail(_dev(t), _dev(scale), _dev(shift), _dev(enc), Ho, Wo)
    head64, tail = R.upconv_tail(t.numpy(), scale.numpy(), shift.numpy(), enc.numpy(), Ho, Wo)
    head32 = F.relu(torch.from_numpy(R.shuffle2x2(t.numpy(), None, Ho, Wo)) * scale + shift)
    _same(out[..., Co:], tail, what + " encoder half")
    _eq("upconv_tail", out[..., :Co], head32, head64, what)
    assert bool((out[..., 2] == 0).all()) and bool((out[..., 1] == float(shift[1])).all()), what + ": dead channels"
    if out[..., 0].numel() >= 32:
        assert bool((out[..., 0] == 0).any()) and bool((out[..., 0] > 0).any()), what + ": the ReLU does not occur"


@pytest.mark.parametrize("Co,Ce", [(32, 32), (16, 64), (4, 4)])
@pytest.mark.parametrize("H,W", HW)
def test_upconv_tail(H, W, Co, Ce):
    for Ho, Wo in _crops(H, W):
        _tail_case(2, H, W, Ho, Wo, Co, Ce, "tail (%d, %d) -> (%d, %d) Co %d Ce %d" % (H, W, Ho, Wo, Co, Ce))


def test_upconv_tail_second_trip():
    N, H, W, Ho, Wo, Co, Ce = 1, 129, 130, 257, 259, 32, 32
    items = N * Ho * Wo * ((Co + Ce) // 4)
    assert items == 1065008 and items > EW_CAP
    _tail_case(N, H, W, Ho, Wo, Co, Ce, "tail second trip", wide=False)


def test_upconv_tail_refusals():
    H, W, Co, Ce = 3, 3, 8, 8
    t, v = torch.zeros(1, H, W, 4 * Co, device="cuda"), torch.zeros(Co, device="cuda")
    enc = torch.zeros(1, 2 * H, 2 * W, Ce, device="cuda")
    out = torch.full((1, 2 * H, 2 * W, Co + Ce), SENTINEL, device="cuda")
    for (ce, Ho), why in (((Ce, 2 * H - 2), "Ho = 2H - 2"), ((6, 2 * H), "Ce = 6")):
        assert _call("mi_upconv_tail_fwd", _p(t), _p(v), _p(v), _p(enc), _p(out), 1, H, W, Co, ce, Ho, 2 * W) == MI_E_ARG, why
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# concat, split, copy-into-slice
# ------------------------------------------------------------------------------------------------
ROWS = [1, 50, 70001]


@pytest.mark.parametrize("Ca,Cb", [(16, 32), (4, 4), (48, 16)])
@pytest.mark.parametrize("M", ROWS)
def test_concat_split(M, Ca, Cb):
    if M == ROWS[-1] and Ca + Cb == 64:
        items = M * ((Ca + Cb) // 4)
        assert items == 1120016 and items > EW_CAP                # the second trip of both kernels
    g = _gen(M + Ca)
    a, b, dout = _wide(g, M, Ca), _wide(g, M, Cb), _wide(g, M, Ca + Cb)
    what = "M %d (%d, %d)" % (M, Ca, Cb)
    _same(g_concat(_dev(a), _dev(b)), R.concat(a.numpy(), b.numpy()), what + " concat")
    da, db = g_split(_dev(dout), Ca, Cb)
    ra, rb = R.split(dout.numpy(), Ca, Cb)
    _same(da, ra, what + " split, first part")
    _same(db, rb, what + " split, second part")


@pytest.mark.parametrize("Cs", [4, 16, 64])
@pytest.mark.parametrize("M", ROWS)
def test_copy_channels_into(M, Cs):
    if M == ROWS[-1] and Cs == 64:
        items = M * (Cs // 4)
        assert items == 1120016 and items > EW_CAP                # the second trip
    src = _wide(_gen(M + Cs), M, Cs)
    for c0, Ct in ((0, Cs + 8), (4, Cs + 8), (8, Cs + 8), (0, Cs)):      # first, middle and last slice of a wider row; the whole row
        dst = (torch.arange(M * Ct, dtype=torch.float32) % 8191 - 4096.5).reshape(M, Ct)      # a sentinel pattern
        got = g_copy_into(_dev(src), _dev(dst), c0)
        what = "copy M %d Cs %d into [%d, %d) of %d" % (M, Cs, c0, c0 + Cs, Ct)
        _same(got, R.copy_channels_into(src.numpy(), dst.numpy(), c0), what)
        assert torch.equal(got[:, :c0].cpu(), dst[:, :c0]) and torch.equal(got[:, c0 + Cs:].cpu(), dst[:, c0 + Cs:]), what


def test_concat_split_copy_refusals():
    a = torch.zeros(4, 8, device="cuda")
    out = torch.full((4, 16), SENTINEL, device="cuda")
    assert _call("mi_copy_channels_into", _p(a), 8, _p(out), 12, 8, 4) == MI_E_ARG, "c0 + Cs > Ct"
    assert _call("mi_copy_channels_into", _p(a), 8, _p(out), 16, 2, 4) == MI_E_ARG, "c0 = 2"
    assert _call("mi_concat_channels", _p(a), 6, _p(a), 8, _p(out), 4) == MI_E_ARG, "Ca = 6"
    assert _call("mi_split_channels", _p(a), _p(out), 8, _p(out), 6, 4) == MI_E_ARG, "Cb = 6"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# the (3,1,1) head
# ------------------------------------------------------------------------------------------------
def _zhead_inputs(N, D, P, C, K, wide=True):
    g = _gen(N + 10 * D + P + 1000 * C + K)
    draw = _wide if wide else (lambda g, *s: torch.randn(*s, generator=g))
    x, dy = draw(g, N, D, P, C), draw(g, N, D, P, K)
    w = torch.randn(3, C, K, generator=g) * (3 * C) ** -0.5
    return x, w, dy


def _zhead_c32(x, w, dy=None, need_x=True, need_w=True):
    """torch's CPU fp32 Conv3d(C, K, (3,1,1), padding (1,0,0)) and its autograd gradients, channels-last in and out"""
    N, D, P, C = x.shape
    K = w.shape[2]
    xt = x.permute(0, 3, 1, 2).reshape(N, C, D, P, 1).clone().requires_grad_(need_x)
    wt = w.permute(2, 1, 0).reshape(K, C, 3, 1, 1).clone().requires_grad_(need_w)
    y = F.conv3d(xt, wt, padding=(1, 0, 0))
    out = [y.detach()[..., 0].permute(0, 2, 3, 1), None, None]
    if dy is not None:
        y.backward(dy.permute(0, 3, 1, 2).reshape(N, K, D, P, 1))
        out[1] = xt.grad[..., 0].permute(0, 2, 3, 1) if need_x else None
        out[2] = wt.grad[:, :, :, 0, 0].permute(2, 1, 0) if need_w else None
    return out


def _zhead_fwd_case(N, D, P, C, K, what, wide=True):
    x, w, _ = _zhead_inputs(N, D, P, C, K, wide)
    y = g_zhead(_dev(x), _dev(w))
    _eq("zhead_fwd", y, _zhead_c32(x, w)[0], R.zhead(x.numpy(), w.numpy()), what)
    return y


@pytest.mark.parametrize("C", [4, 8, 16, 32, 48, 64, 128])
def test_zhead_fwd(C):
    for K in (1, 2, 3, 4):
        for D in (1, 2, 5):
            for P in (63, 837):
                _zhead_fwd_case(2, D, P, C, K, "zhead C %d K %d (2, %d, %d)" % (C, K, D, P))


@pytest.mark.parametrize("C", [16, 32, 64])
def test_zhead_fwd_both_sides_of_the_lane_group_switch(C, monkeypatch):
    """from 4,096 voxels on C = 16 / 32 / 64 take zhead_rows_kernel (C / 4 lanes per voxel); MI_ZHEAD_GENERIC=1 keeps the
    thread-per-voxel kernel there: both against float64"""
    for K in (1, 2, 3, 4):
        _zhead_fwd_case(1, 3, 1365, C, K, "zhead C %d K %d 4095 voxels" % (C, K))
        _zhead_fwd_case(2, 2, 1024, C, K, "zhead C %d K %d 4096 voxels, lane groups" % (C, K))
        with monkeypatch.context() as mp:
            mp.setenv("MI_ZHEAD_GENERIC", "1")
            _zhead_fwd_case(2, 2, 1024, C, K, "zhead C %d K %d 4096 voxels, generic" % (C, K))


def test_zhead_fwd_second_trip_of_the_generic_kernel():
    N, D, P, C, K = 1, 3, 350003, 8, 1
    assert N * D * P == 1050009 and N * D * P > EW_CAP                     # one voxel per thread
    _zhead_fwd_case(N, D, P, C, K, "zhead second trip", wide=False)


def test_zhead_fwd_refusals():
    x, w = torch.zeros(1, 2, 8, 1028 * 4, device="cuda"), torch.zeros(3 * 1028 * 4, device="cuda")
    y = torch.full((1, 2, 8, 8), SENTINEL, device="cuda")
    for (C, K), why in (((8, 0), "K = 0"), ((8, 5), "K = 5"), ((6, 1), "C = 6")):
        assert _call("mi_zhead_fwd", _p(x), _p(w), _p(y), 1, 2, 8, C, K) == MI_E_ARG, why
    assert _call("mi_zhead_fwd", _p(x), _p(w), _p(y), 1, 2, 8, 1028, 4) == MI_E_UNSUPPORTED, "3 * 1028 * 4 floats of LDS"
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


def _zw_blocks(vox, C):
    return max(1, min(vox // ((256 // C) * 64) + 1, ZW_CAP))


def _zhead_bwd_case(N, D, P, C, K, what, data=True, weight=True, wide=True):
    x, w, dy = _zhead_inputs(N, D, P, C, K, wide)
    xd, wd, dyd = _dev(x), _dev(w), _dev(dy)
    _, dx32, dw32 = _zhead_c32(x, w, dy, data, weight)
    dx, dw = g_zhead_bwd(xd, wd, dyd, data, weight)
    if data:
        _eq("zhead_dx", dx, dx32, R.zhead_bwd_data(dy.numpy(), w.numpy()), what + " dx")
    if weight:
        _eq("zhead_dw", dw, dw32, R.zhead_bwd_weight(x.numpy(), dy.numpy()), what + " dw")
    return xd, wd, dyd, dx, dw


@pytest.mark.parametrize("C", [4, 8, 16, 32, 64, 128])
def test_zhead_bwd_data(C):
    for K in (1, 2, 3, 4):
        for D in (1, 2, 5):
            for P in (63, 837):
                _zhead_bwd_case(2, D, P, C, K, "zhead C %d K %d (2, %d, %d)" % (C, K, D, P), weight=False)


def test_zhead_bwd_data_second_trip():
    N, D, P, C, K = 2, 3, 11667, 64, 2
    items = N * D * P * (C // 4)
    assert items == 1120032 and items > EW_CAP
    _zhead_bwd_case(N, D, P, C, K, "zhead dx second trip", weight=False, wide=False)


@pytest.mark.parametrize("C", [4, 8, 16, 32, 64, 128, 256])
def test_zhead_bwd_weight(C):
    """5 voxels: one workgroup whose row groups beyond the fifth idle (all of them busy at C = 64 and above, where there are four or
    fewer); 5 x 837 voxels: several workgroups, a ragged last sweep"""
    for K in (1, 2, 3, 4):
        assert _zw_blocks(5, C) == 1 and (256 // C > 5) == (C < 64)
        _zhead_bwd_case(1, 5, 1, C, K, "zhead C %d K %d 5 voxels in z" % (C, K), data=False)
        _zhead_bwd_case(1, 1, 5, C, K, "zhead C %d K %d 5 voxels in a plane" % (C, K), data=False)
        assert 2 <= _zw_blocks(5 * 837, C) < ZW_CAP
        _zhead_bwd_case(1, 5, 837, C, K, "zhead C %d K %d (1, 5, 837)" % (C, K), data=False)


@pytest.mark.parametrize("C,K,capped", [(256, 3, True), (64, 4, False), (64, 1, False)])
def test_zhead_bwd_weight_many_workgroups(C, K, capped):
    """70,002 voxels.  C = 256: one voxel per workgroup and sweep, 1,094 workgroups wanted, 1,024 given - the stride loop of
    the first 70,002 - 68 * 1,024 = 370 workgroups runs 69 times, the others' 68.  C = 64: 274 workgroups, uncapped."""
    N, D, P = 2, 3, 11667
    vox = N * D * P
    wanted = vox // ((256 // C) * 64) + 1
    assert vox == 70002 and wanted == (1094 if capped else 274) and (wanted > ZW_CAP) == capped
    assert zhead_ws_bytes(N, D, P, C, K) == 8 * 3 * C * K * min(wanted, ZW_CAP)
    _zhead_bwd_case(N, D, P, C, K, "zhead C %d K %d 70,002 voxels" % (C, K), data=False, wide=False)


@pytest.mark.parametrize("C,K", [(4, 1), (32, 3), (256, 4)])
def test_zhead_bwd_pointer_forms_and_rewrite(C, K):
    """dx = NULL, dw = NULL and both given are the same kernels on the same inputs: the same bits.  dw is written, not
    accumulated: a second call into the same buffer leaves the same values."""
    xd, wd, dyd, dx, dw = _zhead_bwd_case(2, 3, 211, C, K, "zhead C %d K %d both pointers" % (C, K))
    dx1, none = g_zhead_bwd(xd, wd, dyd, True, False)
    assert none is None and torch.equal(dx1, dx)
    none, dw1 = g_zhead_bwd(xd, wd, dyd, False, True)
    assert none is None and torch.equal(dw1, dw)
    _, dw2 = g_zhead_bwd(xd, wd, dyd, False, True, dw=dw1.clone())
    assert torch.equal(dw2, dw), "the weight gradient accumulates into what the buffer held"


def test_zhead_bwd_workspace():
    for N, D, P, C, K in ((1, 1, 1, 4, 1), (1, 5, 837, 32, 3), (2, 3, 11667, 256, 4), (2, 3, 11667, 8, 2), (1, 1, 64 * 8 - 1, 32, 1),
                          (1, 1, 64 * 8, 32, 1)):
        assert zhead_ws_bytes(N, D, P, C, K) == 8 * 3 * C * K * _zw_blocks(N * D * P, C), (N, D, P, C, K)
    for N, D, P, C, K in ((0, 1, 1, 4, 1), (1, 1, 1, 48, 1), (1, 1, 1, 4, 5), (1, 1, 1, 4, 0), (1, 1, 0, 4, 1), (1, 1, 1, 512, 1)):
        assert zhead_ws_bytes(N, D, P, C, K) == 0, (N, D, P, C, K)
    N, D, P, C, K = 1, 5, 837, 32, 3
    x, w, dy = (_dev(t) for t in _zhead_inputs(N, D, P, C, K))
    n = zhead_ws_bytes(N, D, P, C, K)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    dw = torch.full((3, C, K), SENTINEL, device="cuda")
    args = (_p(x), _p(w), _p(dy), None, _p(dw), N, D, P, C, K)
    assert _call("mi_zhead_bwd", *args, _p(ws), n - 1) == MI_E_WORKSPACE, "one byte short"
    assert _call("mi_zhead_bwd", *args, None, n) == MI_E_WORKSPACE, "no workspace"
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all())
    assert _call("mi_zhead_bwd", *args, _p(ws), n) == 0
    assert not bool((dw == SENTINEL).any())


def test_zhead_48_channels_forward_only():
    """the contract between the two entries, written down: the forward takes any C % 4 == 0, the backward only a C that
    divides 256.  hipops.HipZHead says so where the graph is built instead of failing inside backward()."""
    from cet_pick_amd import hipops as H
    N, D, P, C, K = 1, 2, 63, 48, 2
    x, w, dy = (_dev(t) for t in _zhead_inputs(N, D, P, C, K))
    assert g_zhead(x, w).isfinite().all()
    dx = torch.full(x.shape, SENTINEL, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert zhead_ws_bytes(N, D, P, C, K) == 0
    assert _call("mi_zhead_bwd", _p(x), _p(w), _p(dy), _p(dx), None, N, D, P, C, K, _p(ws), ws.numel()) == MI_E_ARG
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all())
    head = H.HipZHead(C, K).cuda()
    x5 = x.view(N, D, 7, 9, C)
    with torch.no_grad():
        head.weight.copy_(w.permute(2, 1, 0).reshape(K, C, 3, 1, 1))
        assert torch.equal(head(x5).view(N, D, P, K), g_zhead(x, w))
    with pytest.raises(H.L.HipExtensionError, match="divides 256"):
        head(x5)
    head.weight.requires_grad_(False)
    assert torch.equal(head(x5).view(N, D, P, K), g_zhead(x, w))           # nothing to differentiate: the forward alone
    with pytest.raises(H.L.HipExtensionError, match="divides 256"):
        head(x5.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------
# the first layer
# ------------------------------------------------------------------------------------------------
STEM_EXTENTS = [1, 31, 33, 64, 65]          # Ho, Wo = 1, 16, 17, 32, 33: one pixel, one tile, a tile and a pixel, two tiles, ...


@pytest.mark.parametrize("H", STEM_EXTENTS)
def test_stem2d(H):
    for W in STEM_EXTENTS + [10]:
        for N in (1, 3):
            g = _gen(H + 100 * W + N)
            x = _wide(g, N, H, W)
            w, bias = torch.randn(7, 7, 16, generator=g) * 0.2, torch.randn(16, generator=g)
            for relu, use_bias in ((True, True), (False, False), (True, False), (False, True)):
                b = bias if use_bias else None
                y = g_stem(_dev(x), _dev(w), _dev(b), relu)
                y32 = F.conv2d(x.unsqueeze(1), w.permute(2, 0, 1).unsqueeze(1), b, stride=2, padding=3)
                y32 = (F.relu(y32) if relu else y32).permute(0, 2, 3, 1)
                _eq("stem2d", y, y32, R.stem2d(x.numpy(), w.numpy(), None if b is None else b.numpy(), relu),
                    "stem2d (%d, %d, %d) relu %d bias %d" % (N, H, W, relu, use_bias))


def test_stem2d_refusals():
    x, w = torch.zeros(1, 8, 8, device="cuda"), torch.zeros(7 * 7 * 16, device="cuda")
    y = torch.full((1, 4, 4, 16), SENTINEL, device="cuda")
    for (N, H, W), why in (((0, 8, 8), "N = 0"), ((1, 0, 8), "H = 0"), ((1, 8, 0), "W = 0")):
        assert _call("mi_stem2d_fwd_bias_f32", _p(x), _p(w), None, _p(y), 1, N, H, W) == MI_E_ARG, why
    assert _call("mi_stem2d_fwd_bias_f32", _p(x), _p(w), None, _p(y), 1, 65536, 8, 8) == MI_E_UNSUPPORTED, "grid z"
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# the autograd wrappers in hipops, against the float64 autograd gradient of the torch operation
# ------------------------------------------------------------------------------------------------
def _cf(t):
    return t.permute(0, t.dim() - 1, *range(1, t.dim() - 1))


def _cl(t):
    return t.permute(0, *range(2, t.dim()), 1)


class _Holder(nn.Module):
    def __init__(self, bias):
        super().__init__()
        self.bias = nn.Parameter(bias.clone())


def _op_pool(k):
    def make(ps):
        from cet_pick_amd import hipops as H
        return (lambda x: H.maxpool2d_ceil(x, k)), []
    x = _wide(_gen(k), 2, 13, 9, 8)
    return [x], [], make, (lambda xs, ps: _cl(F.max_pool2d(_cf(xs[0]), k, ceil_mode=True))), True


def _op_convt(crop):
    ci, co, h, w = 32, 16, 6, 5
    ho, wo = (2 * h - 1, 2 * w - 1) if crop else (2 * h, 2 * w)

    def make(ps):
        from cet_pick_amd import hipops as H
        up = H.HipConvTranspose2x2(ci, co).cuda()
        with torch.no_grad():
            up.weight.copy_(ps[0])
            up.bias.copy_(ps[1])
        return (lambda x: up(x, ho, wo) if crop else up(x)), [up.weight, up.bias]
    g = _gen(40 + crop)
    x = torch.randn(2, h, w, ci, generator=g)
    ps = [torch.randn(ci, co, 2, 2, generator=g) * 0.2, torch.randn(co, generator=g)]
    return [x], ps, make, (lambda xs, ps: _cl(F.conv_transpose2d(_cf(xs[0]), ps[0], ps[1], stride=2)[:, :, :ho, :wo])), False


def _op_concat():
    def make(ps):
        from cet_pick_amd import hipops as H
        return (lambda a, b: H.concat_channels(a, b)), []
    g = _gen(41)
    return ([_wide(g, 2, 5, 7, 16), _wide(g, 2, 5, 7, 32)], [], make, (lambda xs, ps: torch.cat((xs[0], xs[1]), -1)), True)


def _op_bias():
    def make(ps):
        from cet_pick_amd import hipops as H
        holder = _Holder(ps[0]).cuda()
        return (lambda x: H.bias_add(x, holder)), [holder.bias]
    g = _gen(42)
    return [torch.randn(2, 5, 7, 12, generator=g)], [torch.randn(12, generator=g)], make, (lambda xs, ps: xs[0] + ps[0]), False


def _op_zhead(c, k):
    def make(ps):
        from cet_pick_amd import hipops as H
        head = H.HipZHead(c, k).cuda()
        with torch.no_grad():
            head.weight.copy_(ps[0])
        return (lambda x: head(x)), [head.weight]
    g = _gen(43 + c + k)
    x = torch.randn(2, 3, 5, 7, c, generator=g)
    ps = [torch.randn(k, c, 3, 1, 1, generator=g) * 0.2]
    return [x], ps, make, (lambda xs, ps: _cl(F.conv3d(_cf(xs[0]), ps[0], padding=(1, 0, 0)))), False


WRAPPERS = {"maxpool2d_ceil k2": lambda: _op_pool(2), "maxpool2d_ceil k3": lambda: _op_pool(3),
            "HipConvTranspose2x2": lambda: _op_convt(False), "HipConvTranspose2x2 cropped": lambda: _op_convt(True),
            "concat_channels": _op_concat, "bias_add": _op_bias, "HipZHead 32 -> 1": lambda: _op_zhead(32, 1),
            "HipZHead 16 -> 3": lambda: _op_zhead(16, 3)}


def _torch_side(fn, xs, ps, need_x, need_p, dy, twice, dtype):
    xt = [x.to(dtype).clone().requires_grad_(n) for x, n in zip(xs, need_x)]
    pt = [p.to(dtype).clone().requires_grad_(need_p) for p in ps]
    y = fn(xt, pt)
    if dy is not None and y.requires_grad:
        for _ in range(2 if twice else 1):
            y.backward(dy.to(dtype), retain_graph=True)
    return y.detach(), [t.grad for t in xt + pt]


@pytest.mark.parametrize("mode", ["all", "input_without_grad", "parameter_frozen", "backward_twice", "dy_not_contiguous"])
@pytest.mark.parametrize("op", sorted(WRAPPERS))
def test_autograd_wrappers(op, mode):
    """y and every gradient against float64 autograd; a tensor that asks for no gradient gets none; a second backward adds to
    .grad (inputs through autograd's AccumulateGrad, parameters through hipops' own target); a dy that is not contiguous"""
    xs, ps, make, torch_fn, exact = WRAPPERS[op]()
    need_x = [True] * len(xs)
    if mode == "input_without_grad":
        need_x[-1] = False
    need_p = mode != "parameter_frozen"
    twice = mode == "backward_twice"
    y64, _ = _torch_side(torch_fn, xs, ps, need_x, need_p, None, False, torch.float64)
    dy = _wide(_gen(9), *y64.shape)
    y64, g64 = _torch_side(torch_fn, xs, ps, need_x, need_p, dy, twice, torch.float64)
    y32, g32 = _torch_side(torch_fn, xs, ps, need_x, need_p, dy, twice, torch.float32)
    fn, hp = make(ps)
    for p in hp:
        p.requires_grad_(need_p)
    xd = [x.cuda().requires_grad_(n) for x, n in zip(xs, need_x)]
    y = fn(*xd)
    assert y.requires_grad == (any(need_x) or (need_p and bool(hp))), op
    if y.requires_grad:
        dyd = dy.cuda()
        if mode == "dy_not_contiguous":
            dyd = torch.stack((dyd, dyd.flip(0)), -1)[..., 0]
            assert not dyd.is_contiguous()
        for _ in range(2 if twice else 1):
            y.backward(dyd, retain_graph=True)
    what = "%s, %s" % (op, mode)
    results = [("y", y.detach(), y32, y64)] + [("gradient %d" % i, t.grad, a, b) for i, (t, a, b) in enumerate(zip(xd + hp, g32, g64))]
    for name, got, r32, r64 in results:
        assert (got is None) == (r64 is None), "%s %s: %s" % (what, name, "missing" if got is None else "not asked for")
        if got is None:
            continue
        assert got.shape == r64.shape, (what, name)
        if exact:
            assert torch.equal(got.cpu().double(), r64), "%s %s: a move, bit for bit" % (what, name)
        else:
            _eq("wrappers", got, r32, r64, "%s %s" % (what, name))
