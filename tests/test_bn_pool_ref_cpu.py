"""tests/bn_pool_ref.py is the float64 reference of tests/test_bn_pool_gpu.py; here it is proven against torch in float64 on the
CPU (F.batch_norm, F.max_pool3d, F.adaptive_avg_pool3d, gradients through autograd): numeric results to 1e-12 relative,
argmax taps and ties bit for bit, on small random and adversarial inputs (ties, all-negative, one NaN)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_pool_ref as R       # noqa: E402

POOLS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2), (6, 2, 3), (2, 1, 0)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, want, what, scale=None):
    """1e-12 of the largest entry - or of `scale`, the size of the terms a cancelling result is the difference of"""
    got, want = np.asarray(got, np.float64), np.asarray(want.detach().numpy() if isinstance(want, torch.Tensor) else want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300) if scale is None else scale
    assert float(np.abs(got - want).max()) <= 1e-12 * scale, (what, float(np.abs(got - want).max()), scale)


def _bn_inputs(M, C, seed, ratio=0.5):
    g = _gen(seed)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + ratio
    gamma = torch.randn(C, generator=g, dtype=torch.float64)
    gamma[0] = 0.0
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    res = torch.randn(M, C, generator=g, dtype=torch.float64)
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    rm = torch.randn(C, generator=g, dtype=torch.float64)
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return x, gamma, beta, res, dy, rm, rv


def test_column_sums():
    x = torch.randn(37, 5, generator=_gen(0), dtype=torch.float64)
    _close(R.column_sums(x.numpy()), x.sum(0), "column sums")
    _close(R.bn_sums(x.numpy()), torch.cat([x.sum(0), (x * x).sum(0)]), "bn sums")


@pytest.mark.parametrize("M,C", [(2, 4), (7, 3), (64, 8), (301, 12)])
@pytest.mark.parametrize("affine,use_res,relu", [(True, True, True), (True, False, False), (False, False, True),
                                                 (False, True, False)])
def test_bn_train_fwd_bwd(M, C, affine, use_res, relu):
    x, gamma, beta, res, dy, rm, rv = _bn_inputs(M, C, 100 * M + C)
    xt = x.clone().requires_grad_(True)
    gt, bt = (gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)) if affine else (None, None)
    rt = res.clone().requires_grad_(True) if use_res else None
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(xt, rm_t, rv_t, gt, bt, True, 0.1, 1e-5)
    if use_res:
        y = y + rt
    pre = y
    if relu:
        y = F.relu(y)
    y.backward(dy)
    out = R.bn_train_fwd(x.numpy(), gamma.numpy() if affine else None, beta.numpy() if affine else None, 1e-5, 0.1,
                         rm.numpy(), rv.numpy(), res.numpy() if use_res else None, relu)
    _close(out["y"], y, "y")
    _close(out["pre"], pre, "pre")
    _close(out["running_mean"], rm_t, "running_mean")
    _close(out["running_var"], rv_t, "running_var")
    _close(out["mean"], x.mean(0), "mean")
    _close(out["invstd"], 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5), "invstd")
    _close(out["save"], torch.cat([x.mean(0), 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)]), "save")
    mask = out["y"] > 0 if relu else None
    bw = R.bn_bwd(dy.numpy(), x.numpy(), out["mean"], out["invstd"], gamma.numpy() if affine else None, mask)
    # dx = gamma * invstd * (dy' - mean(dy') - xhat * mean(dy' * xhat)): with two rows it cancels to zero altogether
    g_inv = float(np.abs((gamma.numpy() if affine else 1.0) * out["invstd"]).max())
    _close(bw["dx"], xt.grad, "dx", scale=g_inv * float(dy.abs().max()) if M == 2 else None)
    if affine:
        _close(bw["dgamma"], gt.grad, "dgamma")
        _close(bw["dbeta"], bt.grad, "dbeta")
    if use_res:
        _close(bw["dres"], rt.grad, "dres")
    _close(R.bn_bwd_sums(dy.numpy(), x.numpy(), out["mean"], out["invstd"], mask),
           np.concatenate([bw["dbeta"], bw["dgamma"]]), "backward sums")
    assert R.bn_train_fwd(x.numpy())["running_mean"] is None


def test_bn_count_is_the_replicated_batch():
    """count = 2 M with doubled sums is the BatchNorm of the batch held twice (two SyncBN ranks with the same rows)"""
    M, C = 9, 4
    x, gamma, beta, _, dy, rm, rv = _bn_inputs(M, C, 5)
    x2 = torch.cat([x, x]).requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = F.batch_norm(x2, rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
    y.backward(torch.cat([dy, dy]))
    out = R.bn_train_fwd(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, 0.1, rm.numpy(), rv.numpy(), count=2 * M)
    _close(out["y"], y[:M], "y")
    _close(out["running_mean"], rm_t, "running_mean")
    _close(out["running_var"], rv_t, "running_var")
    sums = 2 * R.bn_bwd_sums(dy.numpy(), x.numpy(), out["mean"], out["invstd"])
    bw = R.bn_bwd(dy.numpy(), x.numpy(), out["mean"], out["invstd"], gamma.numpy(), sums=sums, count=2 * M)
    _close(bw["dx"], x2.grad[:M], "dx")


def test_bn_one_row_and_constant_column():
    x = np.array([[3.0, -2.0, 0.0, 7.5]])
    out = R.bn_train_fwd(x, beta=np.arange(4.0), running_mean=np.zeros(4), running_var=np.ones(4))
    _close(out["invstd"], np.full(4, 1.0 / np.sqrt(1e-5)), "invstd of one row")
    _close(out["y"], np.arange(4.0)[None], "y of one row is beta")
    _close(out["running_var"], np.full(4, 0.9), "one row: the variance stays biased (no division by zero)")
    xc = np.full((17, 4), 2.5)
    _close(R.bn_train_fwd(xc, beta=np.arange(4.0))["y"], np.repeat(np.arange(4.0)[None], 17, 0), "constant column")


def test_bn_eval_fwd():
    x, gamma, beta, res, _, rm, rv = _bn_inputs(33, 8, 9)
    y = F.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5) + res)
    got, save = R.bn_eval_fwd(x.numpy(), rm.numpy(), rv.numpy(), gamma.numpy(), beta.numpy(), 1e-5, res.numpy(), True)
    _close(got, y, "eval y")
    _close(save, torch.cat([rm, 1.0 / torch.sqrt(rv + 1e-5)]), "eval save")
    got, _ = R.bn_eval_fwd(x.numpy(), rm.numpy(), rv.numpy())
    _close(got, F.batch_norm(x, rm, rv, None, None, False, 0.1, 1e-5), "eval y, no affine")


def _pool_input(kind, shape, seed):
    g = _gen(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    if kind == "relu":
        x = F.relu(x)                              # many exact-zero ties
    elif kind == "negative":
        x = -x.abs() - 0.5                          # padding (zero or -inf) must never win
    elif kind == "constant":
        x = torch.full(shape, 1.25, dtype=torch.float64)
    elif kind == "nan":
        x[0, shape[1] // 2, shape[2] // 2, shape[3] // 2, 1] = float("nan")
    elif kind == "quantised":
        x = torch.round(x * 2) / 2                  # ties between non-zero values
    return x


@pytest.mark.parametrize("k,s,p", POOLS)
@pytest.mark.parametrize("kind", ["random", "relu", "negative", "constant", "nan", "quantised"])
def test_maxpool3d(k, s, p, kind):
    for shape in [(2, 5, 7, 6, 3), (1, 4, 4, 4, 2)] if k <= 4 + 2 * p else [(2, 5, 7, 6, 3)]:
        x = _pool_input(kind, shape, 7 * k + s + p)
        xt = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        y, idx = F.max_pool3d(xt, k, s, p, return_indices=True)
        got, arg = R.maxpool3d_fwd(x.numpy(), k, s, p)
        want = y.detach().permute(0, 2, 3, 4, 1).numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want, equal_nan=True), (kind, shape)           # maxima bit for bit
        flat = R.maxpool3d_input_index(arg, shape[1:4], k, s, p)
        assert np.array_equal(flat, idx.permute(0, 2, 3, 4, 1).numpy()), (kind, shape)     # argmax and ties bit for bit
        dy = torch.randint(-4, 5, y.shape, generator=_gen(3)).double()
        y.backward(dy)
        dx = R.maxpool3d_bwd(dy.permute(0, 2, 3, 4, 1).numpy(), arg, shape[1:4], k, s, p)
        assert np.array_equal(dx, xt.grad.permute(0, 2, 3, 4, 1).numpy()), (kind, shape)


def test_maxpool3d_tap_order():
    """a constant volume: every window ties, and the first tap INSIDE the volume wins"""
    _, arg = R.maxpool3d_fwd(np.ones((1, 4, 4, 4, 1)), 3, 2, 1)
    assert arg[0, 0, 0, 0, 0] == (1 * 3 + 1) * 3 + 1 and arg[0, 1, 1, 1, 0] == 0 and arg[0, 1, 0, 1, 0] == 3


def test_avgpool():
    x = torch.randn(3, 4, 2, 5, 6, generator=_gen(1), dtype=torch.float64, requires_grad=True)      # (B, C, D, H, W)
    y = F.adaptive_avg_pool3d(x, 1).flatten(1)
    dy = torch.randn(3, 4, generator=_gen(2), dtype=torch.float64)
    y.backward(dy)
    rows = x.detach().permute(0, 2, 3, 4, 1).reshape(3, 60, 4).numpy()
    _close(R.avgpool_fwd(rows), y, "avgpool")
    _close(R.avgpool_bwd(dy.numpy(), 60), x.grad.permute(0, 2, 3, 4, 1).reshape(3, 60, 4), "avgpool backward")


@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (5, 2, 2)])
@pytest.mark.parametrize("train", [True, False])
def test_bn_relu_maxpool(k, s, p, train):
    g = _gen(11)
    shape = (2, 5, 7, 6, 4)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = torch.tensor([1.5, -0.7, 0.0, 0.3], dtype=torch.float64)
    beta = torch.tensor([0.1, 0.2, 0.5, -0.4], dtype=torch.float64)
    rm, rv = torch.randn(4, generator=g, dtype=torch.float64), torch.rand(4, generator=g, dtype=torch.float64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    xt = x.permute(0, 4, 1, 2, 3).contiguous()
    act = F.relu(F.batch_norm(xt, rm_t, rv_t, gamma, beta, train, 0.1, 1e-5))
    y, idx = F.max_pool3d(act, k, s, p, return_indices=True)
    got, arg, bn = R.bn_relu_maxpool_fwd(x.numpy(), k, s, p, gamma.numpy(), beta.numpy(), 1e-5, 0.1, rm.numpy(), rv.numpy(),
                                         train)
    _close(got, y.permute(0, 2, 3, 4, 1), "pooled")
    # ties between exact zeros are decided alike only where both sides produce the SAME zeros: they do (max(., 0))
    assert np.array_equal(R.maxpool3d_input_index(arg, shape[1:4], k, s, p), idx.permute(0, 2, 3, 4, 1).numpy())
    if train:
        _close(bn["running_var"], rv_t, "running_var")
