"""tests/unet_ops_ref.py is the float64 reference of tests/test_unet_ops_gpu.py; here it is proven against torch in float64 on
the CPU (F.max_pool2d with ceil_mode and its indices, F.conv_transpose2d and its autograd gradient, torch.cat and slicing,
F.conv3d with a (3,1,1) kernel and its gradients, F.conv2d): numeric results to 1e-12 of the largest entry, argmax taps, ties
and every pure move bit for bit, on small random and adversarial inputs (ties, all-negative data under overhanging windows, a
-inf row, one NaN, two NaNs in one window)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ops_ref as R       # noqa: E402


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, want, what):
    """1e-12 of the largest entry"""
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if isinstance(want, torch.Tensor) else want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300)
    assert float(np.abs(got - want).max()) <= 1e-12 * scale, (what, float(np.abs(got - want).max()), scale)


def _cf(a):        # channels-last numpy -> channels-first torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.permute(0, t.dim() - 1, *range(1, t.dim() - 1)).contiguous()


def _cl(t):        # channels-first torch -> channels-last numpy
    return t.detach().permute(0, *range(2, t.dim()), 1).contiguous().numpy()


def _maxpool_scalar(x, k):
    """the pool once more, one scalar at a time, as the kernel's thread walks its window"""
    N, Hi, Wi, C = x.shape
    Ho, Wo = R.ceil_div(Hi, k), R.ceil_div(Wi, k)
    y, arg = np.empty((N, Ho, Wo, C), x.dtype), np.empty((N, Ho, Wo, C), np.uint8)
    for n in range(N):
        for yo in range(Ho):
            for xo in range(Wo):
                for ch in range(C):
                    best, tap, first = 0.0, 0, True
                    for b in range(k):
                        if yo * k + b >= Hi:
                            break
                        for c in range(k):
                            if xo * k + c >= Wi:
                                break
                            v = x[n, yo * k + b, xo * k + c, ch]
                            if first or v > best or v != v:
                                best, tap = v, b * k + c
                            first = False
                    y[n, yo, xo, ch], arg[n, yo, xo, ch] = best, tap
    return y, arg


@pytest.mark.parametrize("kind", R.POOL_KINDS)
@pytest.mark.parametrize("k,hw", [(1, (5, 4)), (2, (16, 16)), (2, (13, 9)), (2, (1, 7)), (3, (13, 9)), (3, (2, 2)), (5, (13, 9)),
                                  (15, (31, 46)), (15, (16, 16))])
def test_maxpool2d_ceil(k, hw, kind):
    shape = (2, hw[0], hw[1], 3)
    x = R.pool_input(kind, shape, k, 7 * k + hw[0])
    xt = _cf(x).requires_grad_(True)
    y, idx = F.max_pool2d(xt, k, ceil_mode=True, return_indices=True)
    got, arg = R.maxpool2d_ceil(x, k)
    assert got.shape == (2, R.ceil_div(hw[0], k), R.ceil_div(hw[1], k), 3) and arg.dtype == np.uint8
    assert np.array_equal(got, _cl(y), equal_nan=True), (kind, shape)                           # maxima bit for bit
    assert np.array_equal(R.maxpool2d_input_index(arg, hw[1], k), _cl(idx)), (kind, shape)     # argmax and ties bit for bit
    y1, a1 = _maxpool_scalar(x, k)
    assert np.array_equal(got, y1, equal_nan=True) and np.array_equal(arg, a1)
    dy = torch.randint(-4, 5, y.shape, generator=_gen(3)).double() + 0.5                         # never zero
    y.backward(dy)
    dx = R.maxpool2d_ceil_bwd(_cl(dy), arg, shape, k)
    assert np.array_equal(dx, _cl(xt.grad)), (kind, shape)
    assert np.count_nonzero(dx) == dy.numel()                                                    # one input per window


def test_maxpool2d_ceil_tap_order_and_nan_rule():
    _, arg = R.maxpool2d_ceil(np.ones((1, 5, 5, 1)), 3)
    assert np.all(arg == 0)                                             # ties: the first tap, in clipped windows as well
    x = np.arange(25.0).reshape(1, 5, 5, 1)
    y, arg = R.maxpool2d_ceil(x, 3)
    assert arg[0, :, :, 0].tolist() == [[8, 7], [5, 4]]                 # the last tap INSIDE the image, numbered b * 3 + c
    assert y[0, :, :, 0].tolist() == [[12.0, 14.0], [22.0, 24.0]]
    x = -np.ones((1, 3, 3, 1))
    assert R.maxpool2d_ceil(x, 2)[0].max() == -1.0                      # the overhang is not a zero
    x = np.zeros((1, 2, 2, 1))
    x[0, 0, 1, 0] = x[0, 1, 0, 0] = np.nan
    x[0, 1, 1, 0] = 9.0
    y, arg = R.maxpool2d_ceil(x, 2)
    assert np.isnan(y[0, 0, 0, 0]) and arg[0, 0, 0, 0] == 2             # the last NaN; 9.0 behind it does not replace it


@pytest.mark.parametrize("H,W", [(6, 5), (1, 1), (1, 9)])
@pytest.mark.parametrize("crop_h,crop_w", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("Co", [1, 4])
def test_shuffle_pair_is_conv_transpose2d(H, W, crop_h, crop_w, Co):
    """conv_transpose2d(x, wt, b, stride=2)[:, :, :Ho, :Wo] = shuffle(x @ wt as [ci][(a*2+b)*Co + co]) + b, and the gradient
    with respect to that 1x1 product is the un-shuffle of dy with a zero rim"""
    N, Ci = 2, 3
    Ho, Wo = 2 * H - crop_h, 2 * W - crop_w
    g = _gen(H * 100 + W * 10 + Co + crop_h)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    wt = torch.randn(Ci, Co, 2, 2, generator=g, dtype=torch.float64)
    bias = torch.randn(Co, generator=g, dtype=torch.float64)
    t = torch.einsum("nihw,icab->nhwabc", x, wt).reshape(N, H, W, 4 * Co).requires_grad_(True)   # the 1x1 product
    # the transposed convolution as a function of t: one-hot "weights" pick the taps (so that autograd reaches t)
    eye = torch.zeros(4 * Co, Co, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for co in range(Co):
                eye[(a * 2 + b) * Co + co, co, a, b] = 1.0
    for bb in (bias, None):
        y = F.conv_transpose2d(t.permute(0, 3, 1, 2), eye, bb, stride=2)[:, :, :Ho, :Wo]
        want = F.conv_transpose2d(x, wt, bb, stride=2)[:, :, :Ho, :Wo]
        _close(_cl(y), _cl(want), "the one-hot form is the transposed convolution")
        got = R.shuffle2x2(t.detach().numpy(), None if bb is None else bb.numpy(), Ho, Wo)
        if bb is None:
            assert got.dtype == np.float64 and np.array_equal(got, _cl(y)), "shuffle is a move"
        else:
            _close(got, _cl(y), "shuffle + bias")
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        (dt,) = torch.autograd.grad(y, t, dy)
        got = R.unshuffle2x2(_cl(dy), H, W)
        assert np.array_equal(got, dt.numpy()), "un-shuffle is a move with a zero rim"
        if crop_h:
            assert np.all(got[:, H - 1, :, 2 * Co:] == 0)
        if crop_w:
            assert np.all(got[:, :, W - 1, Co:2 * Co] == 0) and np.all(got[:, :, W - 1, 3 * Co:] == 0)


def test_moves_keep_dtype_and_bits():
    t = np.arange(2 * 3 * 2 * 8, dtype=np.float32).reshape(2, 3, 2, 8)
    y = R.shuffle2x2(t, None, 5, 4)
    assert y.dtype == np.float32 and y.shape == (2, 5, 4, 2)
    assert y[1, 3, 2, 1] == t[1, 1, 1, (1 * 2 + 0) * 2 + 1]
    assert np.array_equal(R.shuffle2x2(R.unshuffle2x2(y, 3, 2), None, 5, 4), y)


@pytest.mark.parametrize("H,W,Ho,Wo", [(6, 5, 12, 10), (6, 5, 11, 9), (1, 1, 1, 1), (1, 9, 2, 17)])
def test_upconv_tail(H, W, Ho, Wo):
    N, Co, Ce = 2, 4, 3
    g = _gen(Ho + Wo)
    t = torch.randn(N, H, W, 4 * Co, generator=g, dtype=torch.float64)
    enc = torch.randn(N, Ho, Wo, Ce, generator=g, dtype=torch.float64)
    scale = torch.tensor([1.5, -0.7, 0.0, 0.3], dtype=torch.float64)
    shift = torch.tensor([0.1, 0.2, -0.5, -0.4], dtype=torch.float64)
    eye = torch.zeros(4 * Co, Co, 2, 2, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for co in range(Co):
                eye[(a * 2 + b) * Co + co, co, a, b] = 1.0
    up = F.conv_transpose2d(t.permute(0, 3, 1, 2), eye, None, stride=2)[:, :, :Ho, :Wo]
    want = torch.cat((F.relu(up * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)), enc.permute(0, 3, 1, 2)), 1)
    head, tail = R.upconv_tail(t.numpy(), scale.numpy(), shift.numpy(), enc.numpy(), Ho, Wo)
    _close(head, _cl(want)[..., :Co], "relu(scale * shuffle + shift)")
    assert np.array_equal(tail, _cl(want)[..., Co:])
    assert np.all(head[..., 2] == 0) and (head[..., 1] > 0).any() and (head[..., 1] == 0).any()


@pytest.mark.parametrize("M,Ca,Cb", [(1, 4, 4), (50, 16, 32), (7, 3, 5)])
def test_concat_split_copy(M, Ca, Cb):
    g = _gen(M + Ca)
    a, b = torch.randn(M, Ca, generator=g), torch.randn(M, Cb, generator=g)
    out = R.concat(a.numpy(), b.numpy())
    assert out.dtype == np.float32 and np.array_equal(out, torch.cat((a, b), 1).numpy())
    da, db = R.split(out, Ca, Cb)
    assert np.array_equal(da, a.numpy()) and np.array_equal(db, b.numpy())
    dst = torch.randn(M, Ca + Cb + 4, generator=g)
    kept = dst.clone()
    for c0 in (0, 4, Cb + 4):
        want = dst.clone()
        want[:, c0:c0 + Ca] = a
        got = R.copy_channels_into(a.numpy(), dst.numpy(), c0)
        assert np.array_equal(got, want.numpy())
    assert torch.equal(dst, kept), "the destination given is left as it was"


@pytest.mark.parametrize("N,D,P,C,K", [(2, 1, 5, 4, 1), (1, 2, 7, 8, 3), (2, 5, 9, 12, 4), (3, 3, 1, 4, 2)])
def test_zhead(N, D, P, C, K):
    g = _gen(N + D + P + C + K)
    x = torch.randn(N, D, P, C, generator=g, dtype=torch.float64)
    w = torch.randn(3, C, K, generator=g, dtype=torch.float64)
    dy = torch.randn(N, D, P, K, generator=g, dtype=torch.float64)
    xt = x.permute(0, 3, 1, 2).reshape(N, C, D, P, 1).clone().requires_grad_(True)
    wt = w.permute(2, 1, 0).reshape(K, C, 3, 1, 1).clone().requires_grad_(True)
    y = F.conv3d(xt, wt, padding=(1, 0, 0))
    y.backward(dy.permute(0, 3, 1, 2).reshape(N, K, D, P, 1))
    _close(R.zhead(x.numpy(), w.numpy()), y.detach()[..., 0].permute(0, 2, 3, 1), "zhead")
    _close(R.zhead_bwd_data(dy.numpy(), w.numpy()), xt.grad[..., 0].permute(0, 2, 3, 1), "zhead dx")
    _close(R.zhead_bwd_weight(x.numpy(), dy.numpy()), wt.grad[:, :, :, 0, 0].permute(2, 1, 0), "zhead dw")


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 1, 7), (1, 31, 33), (2, 33, 10), (1, 6, 64), (1, 65, 2)])
@pytest.mark.parametrize("relu,use_bias", [(True, True), (False, False)])
def test_stem2d(N, H, W, relu, use_bias):
    g = _gen(N + H + W)
    x = torch.randn(N, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(7, 7, 16, generator=g, dtype=torch.float64) * 0.2
    bias = torch.randn(16, generator=g, dtype=torch.float64) if use_bias else None
    want = F.conv2d(x.unsqueeze(1), w.permute(2, 0, 1).unsqueeze(1), bias, stride=2, padding=3)
    if relu:
        want = F.relu(want)
    got = R.stem2d(x.numpy(), w.numpy(), None if bias is None else bias.numpy(), relu)
    assert got.shape == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 16)
    _close(got, want.permute(0, 2, 3, 1), "stem2d")
