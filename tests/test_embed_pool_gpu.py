"""mi_embed_pool (csrc/crop_pose.hip) through hipops.embed_pool, against its float64 restatement: F.normalize of every row,
the mean over the poses, F.normalize again.

Bound: 1e-5 absolute on the unit-norm outputs.  The reductions run over at most dim + P = 136 float32 terms, each with a
relative error of at most 2^-24: about 8e-6 in the worst case.  Measured on the MI355X: 1.9e-08 .. 8.1e-08 over the six cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ATOL = 1e-5
N = 5


def _ref64(x):
    x = np.asarray(x, np.float64)
    u = x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)
    m = u.mean(1)
    return m / np.maximum(np.linalg.norm(m, axis=-1, keepdims=True), 1e-12)


def _case(p, dim):
    """(5, p, dim): row 0 of pick 1 all zero; pick 3's rows cancel to a zero mean (p > 1: v, -v and zero rows - a sum that is
    exactly zero in every order, so that the pick can stay in the permutation check)"""
    rng = np.random.default_rng(100 * p + dim)
    x = (rng.standard_normal((N, p, dim)) * rng.uniform(0.01, 50.0, (N, p, 1))).astype(np.float32)
    x[1, 0] = 0.0
    if p > 1:
        x[3, 1] = -x[3, 0]
        x[3, 2:] = 0.0
    return x


@pytest.mark.parametrize("dim", [128, 7])
@pytest.mark.parametrize("p", [1, 3, 8])
def test_embed_pool_matches_float64(p, dim):
    from cet_pick_amd import hipops as H
    x = _case(p, dim)
    xd = torch.as_tensor(x).cuda()
    got = H.embed_pool(xd)
    assert tuple(got.shape) == (N, dim) and got.dtype == torch.float32
    g = got.cpu().numpy()
    ref = _ref64(x)
    err = float(np.abs(g - ref).max())
    print("P %d dim %d: %.3e from float64" % (p, dim, err))
    assert err <= ATOL
    if p > 1:
        assert np.all(g[3] == 0.0) and np.all(ref[3] == 0.0)                 # the cancelling pick: a zero mean stays a zero row
    else:
        assert np.all(g[1] == 0.0)                                            # the all-zero row
        assert float((got - F.normalize(xd[:, 0], dim=1)).abs().max()) <= ATOL
    norms = np.linalg.norm(g.astype(np.float64), axis=1)
    live = np.linalg.norm(ref, axis=1) > 0
    assert np.all(np.abs(norms[live] - 1.0) <= ATOL)
    # the order of the poses does not matter beyond rounding, and the same input gives the same bytes
    perm = np.random.default_rng(p).permutation(p)
    assert float((H.embed_pool(xd[:, perm].contiguous()) - got).abs().max()) <= ATOL
    assert torch.equal(H.embed_pool(xd), got)


def test_embed_pool_refusals():
    from cet_pick_amd import _lib as L
    from cet_pick_amd import hipops as H
    out = torch.full((4, 8), -7.25, device="cuda")
    with pytest.raises(L.HipExtensionError, match="unsupported"):
        H.embed_pool(torch.zeros(2, 2, 1025, device="cuda"))
    with pytest.raises(L.HipExtensionError, match="bad argument"):
        L.call("mi_embed_pool", torch.zeros(4, 8, device="cuda"), 4, 0, 8, out)
    with pytest.raises(L.HipExtensionError):
        H.embed_pool(torch.zeros(4, 8, device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.all(out == -7.25))
    assert tuple(H.embed_pool(torch.zeros(0, 8, 16, device="cuda")).shape) == (0, 16)
