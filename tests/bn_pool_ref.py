"""Plain float64 numpy restatements of the operations in the first third of csrc/train_ops.hip: column sums, BatchNorm
(training and eval forward, backward with a given ReLU mask), MaxPool3d with its argmax tap, the global average pool and the
fused BatchNorm + ReLU + max-pool.  No torch, no hipops: tests/test_bn_pool_ref_cpu.py proves every function here against
torch in float64, tests/test_bn_pool_gpu.py measures the kernels against them.

Layout as in the kernels: activations are channels-last, (M, C) rows or (N, D, H, W, C) volumes."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def column_sums(x):
    """(M, C) -> (C,)"""
    return _f64(x).sum(0)


def bn_sums(x):
    """what mi_bn_stats leaves: [sum x (C), sum x^2 (C)]"""
    x = _f64(x)
    return np.concatenate([x.sum(0), (x * x).sum(0)])


def bn_train_fwd(x, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, res=None,
                 relu=False, count=None):
    """Training-mode BatchNorm over the rows of x (M, C): y = relu?((x - mean) * invstd * gamma + beta + res).
    count: the number of rows the statistics stand for when it is not M - SyncBN over `count / M` ranks that all hold these
    rows hands the kernel `count / M` times the sums: mean and biased variance are those of x, only the unbiased factor
    count / (count - 1) of the running variance sees `count`.  (Variance by the two-pass formula: no cancellation.)
    Returns a dict: y, pre (y in front of the ReLU), mean, var (biased), invstd, save = [mean, invstd], running_mean,
    running_var (None where no running statistics were given)."""
    x = _f64(x)
    M, C = x.shape
    count = float(M if count is None else count)
    g = np.ones(C) if gamma is None else _f64(gamma)
    b = np.zeros(C) if beta is None else _f64(beta)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    pre = (x - mean) * invstd * g + b
    if res is not None:
        pre = pre + _f64(res)
    out = dict(y=np.maximum(pre, 0.0) if relu else pre, pre=pre, mean=mean, var=var, invstd=invstd,
               save=np.concatenate([mean, invstd]), running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * _f64(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * _f64(running_var) + momentum * unbiased
    return out


def bn_eval_fwd(x, running_mean, running_var, gamma=None, beta=None, eps=1e-5, res=None, relu=False):
    """Eval-mode BatchNorm: the running statistics normalise.  Returns (y, save = [mean, invstd])."""
    x = _f64(x)
    C = x.shape[1]
    g = np.ones(C) if gamma is None else _f64(gamma)
    b = np.zeros(C) if beta is None else _f64(beta)
    mean, invstd = _f64(running_mean), 1.0 / np.sqrt(_f64(running_var) + eps)
    pre = (x - mean) * invstd * g + b
    if res is not None:
        pre = pre + _f64(res)
    return (np.maximum(pre, 0.0) if relu else pre), np.concatenate([mean, invstd])


def bn_bwd_sums(dy, x, mean, invstd, mask=None):
    """what the backward reduction leaves: [sum dy' (C), sum dy' * xhat (C)], dy' = dy * mask"""
    d = _f64(dy) if mask is None else _f64(dy) * np.asarray(mask, bool)
    xhat = (_f64(x) - _f64(mean)) * _f64(invstd)
    return np.concatenate([d.sum(0), (d * xhat).sum(0)])


def bn_bwd(dy, x, mean, invstd, gamma=None, mask=None, sums=None, count=None):
    """Backward of training-mode BatchNorm (+ ReLU with the given mask = the forward's y > 0):
    dx = gamma * invstd * (dy' - sum_dy / count - xhat * sum_dyxhat / count), dgamma = sum_dyxhat, dbeta = sum_dy, dres = dy'.
    sums / count: as all-reduced over the ranks (default: this tensor's own sums over its M rows)."""
    x = _f64(x)
    M, C = x.shape
    d = _f64(dy) if mask is None else _f64(dy) * np.asarray(mask, bool)
    mean, invstd = _f64(mean), _f64(invstd)
    g = np.ones(C) if gamma is None else _f64(gamma)
    sums = bn_bwd_sums(d, x, mean, invstd) if sums is None else _f64(sums)
    count = float(M if count is None else count)
    xhat = (x - mean) * invstd
    dx = g * invstd * (d - sums[:C] / count - xhat * sums[C:] / count)
    return dict(dx=dx, dgamma=sums[C:].copy(), dbeta=sums[:C].copy(), dres=d)


def pool_out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def maxpool3d_fwd(x, k, s, p):
    """MaxPool3d(k, stride s, padding p) of x (N, D, H, W, C) -> (y, arg): arg (uint8) is the window tap (a * k + b) * k + c of
    the maximum, the FIRST one in (z, y, x) order; padding never takes part; a NaN wins over everything that came before it
    and keeps its place against everything but a later NaN (torch's rule: val > max || isnan(val))."""
    x = _f64(x)
    N, D, H, W, C = x.shape
    Do, Ho, Wo = pool_out(D, k, s, p), pool_out(H, k, s, p), pool_out(W, k, s, p)
    assert min(Do, Ho, Wo) > 0
    xp = np.zeros((N, D + 2 * p, H + 2 * p, W + 2 * p, C))
    vp = np.zeros((1, D + 2 * p, H + 2 * p, W + 2 * p, 1), bool)
    xp[:, p:p + D, p:p + H, p:p + W] = x
    vp[:, p:p + D, p:p + H, p:p + W] = True
    best = np.full((N, Do, Ho, Wo, C), -np.inf)
    arg = np.zeros((N, Do, Ho, Wo, C), np.uint8)
    first = np.ones((1, Do, Ho, Wo, 1), bool)
    for a in range(k):
        for b in range(k):
            for c in range(k):
                sl = (slice(None), slice(a, a + (Do - 1) * s + 1, s), slice(b, b + (Ho - 1) * s + 1, s),
                      slice(c, c + (Wo - 1) * s + 1, s))
                t, ok = xp[sl], vp[sl]
                with np.errstate(invalid="ignore"):
                    take = ok & (first | (t > best) | np.isnan(t))
                best = np.where(take, t, best)
                arg = np.where(take, np.uint8((a * k + b) * k + c), arg)
                first = first & ~ok
    return best, arg


def maxpool3d_input_index(arg, in_shape, k, s, p):
    """the argmax taps as flat indices z * H * W + y * W + x into the input volume (what torch's return_indices gives)"""
    D, H, W = in_shape
    N, Do, Ho, Wo, C = arg.shape
    a = arg.astype(np.int64)
    zo, yo, xo = np.meshgrid(np.arange(Do), np.arange(Ho), np.arange(Wo), indexing="ij")
    zi = zo[None, ..., None] * s - p + a // (k * k)
    yi = yo[None, ..., None] * s - p + (a // k) % k
    xi = xo[None, ..., None] * s - p + a % k
    assert zi.min() >= 0 and zi.max() < D and yi.min() >= 0 and yi.max() < H and xi.min() >= 0 and xi.max() < W
    return (zi * H + yi) * W + xi


def maxpool3d_bwd(dy, arg, in_shape, k, s, p):
    """dx (N, D, H, W, C): every pooled gradient goes to the voxel its argmax tap names"""
    D, H, W = in_shape
    dy = _f64(dy)
    N, Do, Ho, Wo, C = dy.shape
    flat = maxpool3d_input_index(arg, in_shape, k, s, p)
    dx = np.zeros((N, D * H * W, C))
    n = np.arange(N)[:, None, None, None, None] + np.zeros_like(flat)
    c = np.arange(C)[None, None, None, None, :] + np.zeros_like(flat)
    np.add.at(dx, (n.ravel(), flat.ravel(), c.ravel()), dy.ravel())
    return dx.reshape(N, D, H, W, C)


def avgpool_fwd(x):
    """global average pool: x (B, S, C) -> (B, C)"""
    return _f64(x).mean(1)


def avgpool_bwd(dy, S):
    dy = _f64(dy)
    return np.repeat(dy[:, None, :] / S, S, axis=1)


def bn_relu_maxpool_fwd(x, k, s, p, gamma=None, beta=None, eps=1e-5, momentum=0.1, running_mean=None, running_var=None,
                        train=True):
    """MaxPool3d(relu(bn(x))) of x (N, D, H, W, C) as the composition of the functions above.
    Returns (pooled, arg, bn): bn is bn_train_fwd's dict (train) or the (y, save) of bn_eval_fwd."""
    x = _f64(x)
    C = x.shape[-1]
    if train:
        bn = bn_train_fwd(x.reshape(-1, C), gamma, beta, eps, momentum, running_mean, running_var, relu=True)
        act = bn["y"]
    else:
        bn = bn_eval_fwd(x.reshape(-1, C), running_mean, running_var, gamma, beta, eps, relu=True)
        act = bn[0]
    y, arg = maxpool3d_fwd(act.reshape(x.shape), k, s, p)
    return y, arg, bn
