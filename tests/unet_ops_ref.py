"""Plain float64 numpy restatements of the operations in csrc/unet_ops.hip, the detector network's glue: the ceil-mode 2-D
max pool with its argmax tap, the 2x2 transposed convolution's shuffle and un-shuffle, the fused up-convolution tail, concat /
split / copy-into-slice, the (3,1,1) head with both gradients and the 7x7 one-channel first layer.  No torch, no hipops:
tests/test_unet_ops_ref_cpu.py proves every function here against torch in float64, tests/test_unet_ops_gpu.py measures the
kernels against them.

Layout as in the kernels: channels-last, (N, H, W, C) images, (M, C) rows, (N, D, P, C) head volumes with P = H * W.  Every
function takes what the C entry of the same operation takes.  Pure moves keep the dtype they are given (they are compared
bit for bit); arithmetic is float64."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def ceil_div(a, b):
    return (a + b - 1) // b


# ---- nn.MaxPool2d(k, stride=k, ceil_mode=True) ---------------------------------------------------------------------------------
def maxpool2d_ceil(x, k):
    """x (N, Hi, Wi, C) -> y (N, Ho, Wo, C), arg uint8 (N, Ho, Wo, C) with Ho = ceil(Hi / k).  arg is the tap b * k + c of the
    maximum inside its window.  The window is clipped to the image: the overhang does not exist (it is neither 0 nor -inf, it
    is not looked at).  Row-major scan; the first element is taken as it is, a later one replaces the held one when it is
    strictly greater (the first maximum wins a tie) or when it is a NaN (the last NaN of a window wins, and nothing replaces
    a NaN but another NaN)."""
    x = np.asarray(x)
    N, Hi, Wi, C = x.shape
    # tap (0, 0) exists in every window: it is the first element, taken as it is
    y = x[:, 0::k, 0::k, :].copy()
    arg = np.zeros(y.shape, np.uint8)
    assert y.shape[1:3] == (ceil_div(Hi, k), ceil_div(Wi, k))
    for b in range(k):                      # the loop over the window's taps, row-major; all windows at once
        for c in range(k):
            if b == 0 and c == 0:
                continue
            v = x[:, b::k, c::k, :]         # the windows that have this tap inside the image: the others do not see it
            if v.size == 0:
                continue
            held = y[:, :v.shape[1], :v.shape[2], :]
            tap = arg[:, :v.shape[1], :v.shape[2], :]
            with np.errstate(invalid="ignore"):
                take = (v > held) | (v != v)
            held[take] = v[take]
            tap[take] = b * k + c
    return y, arg


POOL_KINDS = ["random", "constant", "quantised", "negative", "neg_inf_row", "all_neg_inf", "nan", "two_nans"]


def pool_input(kind, shape, k, seed, dtype=np.float64):
    """(N, Hi, Wi, C) inputs of the pool, the adversarial ones among them; both test files draw from here"""
    N, Hi, Wi, C = shape
    x = np.random.default_rng(seed).standard_normal(shape).astype(dtype)
    if kind == "constant":
        x[...] = 1.25                                          # every window ties: tap 0 wins
    elif kind == "quantised":
        x = np.round(x * 2) / 2                                 # ties between non-zero values
    elif kind == "negative":
        x = -np.abs(x) - 0.5                                    # an overhang taken as 0 would win every edge window
    elif kind == "neg_inf_row":
        x[:, Hi - 1, :, :] = -np.inf                            # the last row: with Hi % k == 1 whole windows are -inf
        x[:, :, 0, 0] = -np.inf
    elif kind == "all_neg_inf":
        x[...] = -np.inf                                        # the first element is taken although nothing is > -inf
    elif kind == "nan":
        x[0, Hi // 2, Wi // 2, C // 2] = np.nan
    elif kind == "two_nans":                                    # both in the window of (0, 0): the last one wins
        x[0, 0, 0, 0] = np.nan
        x[0, min(k, Hi) - 1, min(k, Wi) - 1, 0] = np.nan
        x[N - 1, Hi - 1, Wi - 1, C - 1] = np.nan                # and one in the far corner's (clipped) window
    return x


def maxpool2d_ceil_bwd(dy, arg, shape, k):
    """dy, arg (N, Ho, Wo, C), shape = (N, Hi, Wi, C) -> dx: the windows are disjoint, each dy goes to its window's tap"""
    dy = np.asarray(dy)
    N, Hi, Wi, C = shape
    dx = np.zeros(shape, dy.dtype)
    for b in range(k):
        for c in range(k):
            into = dx[:, b::k, c::k, :]     # tap (b, c) of every window that has it
            if into.size == 0:
                continue
            hit = arg[:, :into.shape[1], :into.shape[2], :] == b * k + c
            into[hit] = dy[:, :into.shape[1], :into.shape[2], :][hit]
    return dx


def maxpool2d_input_index(arg, Wi, k):
    """the flat index yi * Wi + xi (torch's return_indices) of every argmax tap"""
    N, Ho, Wo, C = arg.shape
    tap = arg.astype(np.int64)
    yo = np.arange(Ho).reshape(1, Ho, 1, 1)
    xo = np.arange(Wo).reshape(1, 1, Wo, 1)
    return (yo * k + tap // k) * Wi + xo * k + tap % k


# ---- nn.ConvTranspose2d(Ci, Co, 2, stride=2) behind its 1x1 product ------------------------------------------------------------
def shuffle2x2(t, bias, Ho, Wo):
    """t (N, H, W, 4 * Co), column (a * 2 + b) * Co + co -> y (N, Ho, Wo, Co) with y[n][2h + a][2w + b][co] = t[...] + bias[co],
    cropped to (Ho, Wo) <= (2H, 2W).  bias None: a pure move in t's dtype.  With a bias: float64."""
    t = np.asarray(t)
    N, H, W, C4 = t.shape
    Co = C4 // 4
    y = np.empty((N, Ho, Wo, Co), t.dtype if bias is None else np.float64)
    assert 0 < Ho <= 2 * H and 0 < Wo <= 2 * W
    for a in range(2):
        for b in range(2):
            into = y[:, a::2, b::2, :]                      # the output pixels (2h + a, 2w + b) that survive the crop
            v = t[:, :into.shape[1], :into.shape[2], (a * 2 + b) * Co:(a * 2 + b + 1) * Co]
            into[...] = v if bias is None else _f64(v) + _f64(bias)
    return y


def unshuffle2x2(dy, H, W):
    """dy (N, Ho, Wo, Co) -> dt (N, H, W, 4 * Co): dt[n][h][w][(a * 2 + b) * Co + co] = dy[n][2h + a][2w + b][co], and zero
    where (2h + a, 2w + b) lies in the rim the forward cropped away"""
    dy = np.asarray(dy)
    N, Ho, Wo, Co = dy.shape
    dt = np.zeros((N, H, W, 4 * Co), dy.dtype)
    assert 0 < Ho <= 2 * H and 0 < Wo <= 2 * W
    for a in range(2):
        for b in range(2):
            v = dy[:, a::2, b::2, :]                        # (2h + a, 2w + b) inside (Ho, Wo); the rest of dt stays zero
            dt[:, :v.shape[1], :v.shape[2], (a * 2 + b) * Co:(a * 2 + b + 1) * Co] = v
    return dt


def upconv_tail(t, scale, shift, enc, Ho, Wo):
    """out (N, Ho, Wo, Co + Ce): [..., :Co] = relu(scale * shuffle(t) + shift) in float64, [..., Co:] = enc (a move: returned
    apart, in enc's dtype).  Returns (head float64 (N, Ho, Wo, Co), enc)."""
    s = _f64(shuffle2x2(t, None, Ho, Wo))
    return np.maximum(s * _f64(scale) + _f64(shift), 0.0), np.asarray(enc)


# ---- torch.cat over the channel axis and its pieces ----------------------------------------------------------------------------
def concat(a, b):
    """a (M, Ca), b (M, Cb) -> (M, Ca + Cb)"""
    a, b = np.asarray(a), np.asarray(b)
    out = np.empty((a.shape[0], a.shape[1] + b.shape[1]), a.dtype)
    for m in range(a.shape[0]):
        out[m, :a.shape[1]] = a[m]
        out[m, a.shape[1]:] = b[m]
    return out


def split(dout, Ca, Cb):
    """dout (M, Ca + Cb) -> da (M, Ca), db (M, Cb)"""
    dout = np.asarray(dout)
    assert dout.shape[1] == Ca + Cb
    return dout[:, :Ca].copy(), dout[:, Ca:].copy()


def copy_channels_into(src, dst, c0):
    """dst (M, Ct) with dst[m][c0 : c0 + Cs] = src[m][:], everything else as it was; returns the new dst"""
    src, out = np.asarray(src), np.array(dst, copy=True)
    out[:, c0:c0 + src.shape[1]] = src
    return out


# ---- nn.Conv3d(C, K, (3,1,1), padding=(1,0,0), bias=False) ---------------------------------------------------------------------
def zhead(x, w):
    """x (N, D, P, C), w [3][C][K] -> y (N, D, P, K): y[n][z][p][k] = sum_{dz, c} x[n][z + dz - 1][p][c] * w[dz][c][k], planes
    outside [0, D) are zero"""
    x, w = _f64(x), _f64(w)
    N, D, P, C = x.shape
    y = np.zeros((N, D, P, w.shape[2]))
    for z in range(D):
        for dz in range(3):
            zz = z + dz - 1
            if 0 <= zz < D:
                y[:, z] += x[:, zz] @ w[dz]
    return y


def zhead_bwd_data(dy, w):
    """dy (N, D, P, K), w [3][C][K] -> dx (N, D, P, C): dx[n][z][p][c] = sum_{dz, k} dy[n][z - dz + 1][p][k] * w[dz][c][k]"""
    dy, w = _f64(dy), _f64(w)
    N, D, P, K = dy.shape
    dx = np.zeros((N, D, P, w.shape[1]))
    for z in range(D):
        for dz in range(3):
            zo = z - dz + 1
            if 0 <= zo < D:
                dx[:, z] += dy[:, zo] @ w[dz].T
    return dx


def zhead_bwd_weight(x, dy):
    """x (N, D, P, C), dy (N, D, P, K) -> dw [3][C][K]: dw[dz][c][k] = sum over voxels of x[n][z + dz - 1][p][c] * dy[n][z][p][k]"""
    x, dy = _f64(x), _f64(dy)
    N, D, P, C = x.shape
    dw = np.zeros((3, C, dy.shape[3]))
    for z in range(D):
        for dz in range(3):
            zz = z + dz - 1
            if 0 <= zz < D:
                dw[dz] += np.einsum("npc,npk->ck", x[:, zz], dy[:, z])
    return dw


# ---- nn.Conv2d(1, 16, 7, stride 2, padding 3) ----------------------------------------------------------------------------------
def stem2d(x, w, bias, relu):
    """x (N, H, W), w [7][7][16], bias [16] or None -> y (N, Ho, Wo, 16) with Ho = (H - 1) // 2 + 1:
    y[n][yo][xo][c] = act(sum_{ky, kx} x[n][2 yo + ky - 3][2 xo + kx - 3] * w[ky][kx][c] + bias[c]), zero outside the image"""
    x, w = _f64(x), _f64(w).reshape(7, 7, 16)
    N, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 5, 2 * Wo + 5))
    xp[:, 3:3 + H, 3:3 + W] = x
    y = np.zeros((N, Ho, Wo, 16))
    for ky in range(7):
        for kx in range(7):
            y += xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, None] * w[ky, kx]
    if bias is not None:
        y = y + _f64(bias)
    return np.maximum(y, 0.0) if relu else y
