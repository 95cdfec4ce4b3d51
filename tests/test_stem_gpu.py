"""The 7^3 stride-2 stem (csrc/conv_stem.hip) and its tail (BatchNorm + ReLU + MaxPool3d(3, 2, 1), csrc/train_ops.hip) against
torch on the CPU in float64, arbitrated by the same chain in fp32 on the CPU (conftest.f32_equivalent), at every tiling, switch and
edge of the tile walk.  Every convolution case asserts the kernel family it ran (mi_debug_last_conv_kernel); the variant inside
the family is pinned by the shape and the switch (conv_stem.hip mi_stem7_fwd / mi_stem7_wgrad):

  forward   default          Do % 8 == 0: stem_fwd_bf3_kernel<1, 2>, otherwise <1, 1>
            MI_STEM_FWD_Z4     <1, 1> (the 8 x 4 x 4 tile at every depth)
            MI_STEM_FWD_NBUF2  <2, 1>
            MI_CONV_ARITH=f32  stem_fwd_kernel
            MI_CONV_NO_STEM    the implicit GEMM
  weight    default          stem_wgrad_bf3_kernel<2>
  gradient  MI_STEM_WGRAD_OCC=1  stem_wgrad_bf3_kernel<1>
            MI_STEM_WGRAD_F32    stem_wgrad_kernel
            MI_CONV_NO_STEM      the implicit GEMM

Inputs are randn * exp(2 randn): the three-way bf16 cut has to hold at every exponent."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCHES = ("MI_STEM_FWD_Z4", "MI_STEM_FWD_NBUF2", "MI_CONV_ARITH", "MI_CONV_NO_STEM", "MI_STEM_WGRAD_OCC", "MI_STEM_WGRAD_F32",
            "MI_STEM_NO_STATS", "MI_MAXPOOL_BWD_BAND", "MI_MAXPOOL_BWD_GENERIC", "MI_COLREDUCE_BLOCKS")


def cl(x):  # NCDHW -> channels-last contiguous on the GPU
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def make_w(co, ci, k, g):
    from cet_pick_amd import hipops as H
    p = H.conv_weight_param(co, ci, k)
    w = torch.randn(co, ci, k, k, k, generator=g) * (2.0 / (ci * k ** 3)) ** 0.5
    with torch.no_grad():
        p.copy_(w)
    p.data = p.data.cuda()
    return p, w


def wide(g, *shape):
    return torch.randn(*shape, generator=g) * torch.exp(2 * torch.randn(*shape, generator=g))


def switch(monkeypatch, env):
    """Exactly the switches of `env` (most of them are tested with getenv() != NULL: off means unset)."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def last_kernel():
    from cet_pick_amd import _lib as L
    return L.lib().mi_debug_last_conv_kernel().decode()


def out_extent(v):
    return (v + 6 - 7) // 2 + 1


def cpu_reference():
    """The CPU references are torch's own convolution kernels: oneDNN's fp32 weight gradient of the (3, 7, 7, 15) case is off by a
    factor of 1e20 and more (float64 never goes through oneDNN)."""
    return torch.backends.mkldnn.flags(enabled=False)


def equivalent(got, cpu32, ref64, what):
    """conftest.f32_equivalent with its default factor and floor - and the arbiter must itself be an fp32 evaluation: a CPU result
    that is garbage would allow anything.  1e-4 is the suite's fp32 tolerance, far above 2^-24 sqrt(K) of the longest reduction here
    (K = 140,800 voxels: 2e-5)."""
    from conftest import f32_equivalent
    e = f32_equivalent(got, cpu32, ref64, what=what)
    assert e[1] < 1e-4, "%s: the CPU fp32 arbiter is %.3e from float64" % (what, e[1])
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------
FWD_SHAPES = [(1, 8, 8, 16),       # one tile, every face of the patch is padding; Do = 4: <1, 1>
              (3, 7, 7, 15),       # odd extents (the high-side padding fully used), one tile per sample, <1, 1>
              (2, 24, 8, 32),      # Do = 12: first / interior / last z tile on <1, 1>, two x tiles
              (2, 16, 24, 16),     # non-cubic on <1, 2>: Do = 8, Ho = 12, Wo = 8
              (2, 15, 23, 31),     # odd extents on <1, 2>
              (5, 16, 16, 16)]     # cubic, odd batch
FWD_SETTINGS = [("default", {}), ("z4", {"MI_STEM_FWD_Z4": "1"}), ("nbuf2", {"MI_STEM_FWD_NBUF2": "1"}),
                ("f32", {"MI_CONV_ARITH": "f32"}), ("generic", {"MI_CONV_NO_STEM": "1"})]


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_stem_forward_every_variant_matches_float64(shape, monkeypatch):
    """Plain and with the fused epilogue (residual + ReLU), under the five settings: each result f32-equivalent to float64, each
    pair of variants within 2e-6 of the float64 result's largest magnitude (test_conv_direct3_matches_igemm_and_float64's bound for
    two fp32 summation orders at K = 1728; K = 343 here).
    The three bf16x3 tilings are held to BIT equality instead.  From the code (stem_fwd_bf3_kernel): the accumulator of an output
    voxel and channel receives, for each of the 25 k-steps in the order (slab 0, u 0..3), ..., (slab 5, u 0..3), (slab 6, u 0), the
    six products pr = 0..5 of (PA[pr], PB[pr]) - `mfmas` walks pr outside and the z-planes of the wave inside, so ZPW = 2 only
    interleaves the chains of two different voxels; NBUF only moves where the slab's store and the next k-step's fragment reads sit
    between the MFMAs.  The fragments are the same bytes (one cut of the patch, one weight image), and a voxel keeps its row
    (r & 3) + 8 (r >> 2) + 4 h of the 32 x 32 tile in every tiling."""
    from cet_pick_amd import hipops as H
    n, d, h, w_ = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    x = wide(g, n, 1, d, h, w_)
    param, w = make_w(64, 1, 7, g)
    res = torch.randn(n, 64, out_extent(d), out_extent(h), out_extent(w_), generator=g)

    def chain(dt):
        y = F.conv3d(x.to(dt), w.to(dt), stride=2, padding=3)
        return (y.permute(0, 2, 3, 4, 1), F.relu(y + res.to(dt)).permute(0, 2, 3, 4, 1))
    with cpu_reference():
        ref64, cpu32 = chain(torch.float64), chain(torch.float32)
    xc, rc = cl(x), cl(res)
    out = {}
    for tag, env in FWD_SETTINGS:
        switch(monkeypatch, env)
        y = H.conv_fwd(xc, param, 7, 2, 3)
        names = [last_kernel()]
        y2 = H.conv_fwd(xc, param, 7, 2, 3, rc, True)
        names.append(last_kernel())
        for name in names:
            assert (name.startswith("implicit GEMM") if tag == "generic" else name == "stem_fwd"), (tag, names)
        out[tag] = (y.cpu(), y2.cpu())
        for i, what in enumerate(("plain", "residual + ReLU")):
            e = equivalent(out[tag][i].numpy(), cpu32[i].numpy(), ref64[i].numpy(), what="stem fwd %s %s %s" % (shape, tag, what))
            print("stem fwd %s %-8s %-15s kernel %-14s GPU %.3e  CPU fp32 %.3e" % (shape, tag, what, names[i], e[0], e[1]))
    for i in range(2):
        for tag in ("z4", "nbuf2"):
            assert torch.equal(out["default"][i], out[tag][i]), (tag, i)
        scale = float(ref64[i].abs().max())
        for a, b in itertools.combinations(out, 2):
            assert float((out[a][i] - out[b][i]).abs().max()) / scale < 2e-6, (a, b, i)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. statistics epilogue
# ---------------------------------------------------------------------------------------------------------------------------
def _stats_bound(y):
    """(want, scale) of the 128 sums of y (rows x 64, float64): the existing bound is 2e-6 of the column's absolute sum for the sums
    and of the sum of squares for the squares (fp32 partial sums over a lane's 16 ZPW voxels, doubles from there)."""
    y64 = y.double().reshape(-1, 64)
    want = torch.cat([y64.sum(0), (y64 * y64).sum(0)])
    return want, torch.cat([y64.abs().sum(0), want[64:]])


@pytest.mark.parametrize("shape,z4", [((1, 8, 8, 16), False), ((1, 8, 8, 16), True), ((2, 24, 8, 32), False), ((2, 24, 8, 32), True),
                                      ((2, 15, 23, 31), False), ((2, 15, 23, 31), True), ((2, 16, 24, 16), False)])
def test_stem_statistics_epilogue(shape, z4, monkeypatch):
    """mi_conv3d_stem_stats_f32 on <1, 1> (Do = 4, 12, and Do = 8 under MI_STEM_FWD_Z4) and <1, 2> (Do = 8): y bit-equal to the plain
    forward of the same variant, the 128 sums within 2e-6 of float64 column sums of y.  The entry does not pass through the dispatcher
    that notes the kernel family: its return code (0, not MI_E_UNSUPPORTED) says that the stem kernel ran, and the workspace - partials
    included - starts as NaN."""
    from cet_pick_amd import hipops as H, _lib as L
    lib = L.lib()
    n, d, h, w_ = shape
    g = torch.Generator().manual_seed(2000 + sum(shape))
    x = wide(g, n, d, h, w_, 1).cuda()
    param, _ = make_w(64, 1, 7, g)
    switch(monkeypatch, {"MI_STEM_FWD_Z4": "1"} if z4 else {})
    y_plain = H.conv_fwd(x, param, 7, 2, 3)
    assert last_kernel() == "stem_fwd"
    nbytes = lib.mi_conv3d_stem_stats_workspace_bytes(n, d, h, w_, 64)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    y = torch.full_like(y_plain, float("nan"))
    sums = torch.full((128,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.mi_conv3d_stem_stats_f32(L.ptr(x), L.ptr(param), L.ptr(y), n, d, h, w_, 64, L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
    assert rc == 0
    assert torch.equal(y, y_plain)
    want, scale = _stats_bound(y)
    err = float(((sums - want).abs() / scale).max())
    print("stem stats %s z4=%d: %.3e" % (shape, z4, err))
    assert err < 2e-6


def test_stem_statistics_workspace_declines():
    from cet_pick_amd import _lib as L
    lib = L.lib()
    assert lib.mi_conv3d_stem_stats_workspace_bytes(2, 8, 8, 16, 64) > 0
    assert lib.mi_conv3d_stem_stats_workspace_bytes(2, 8, 8, 24, 64) == 0        # Wo = 12
    assert lib.mi_conv3d_stem_stats_workspace_bytes(2, 8, 8, 16, 32) == 0        # Co = 32


@pytest.mark.parametrize("shape", [(2, 16, 24, 16), (3, 24, 8, 32)])
def test_stem_block_with_and_without_epilogue_statistics(shape, monkeypatch):
    """The encoder trunk's stem block (conv1, then bn1 + ReLU + MaxPool3d as TomoResClassifier3D._trunk runs them) with bn1's sums from
    conv1's epilogue and, under MI_STEM_NO_STATS=1, from the statistics pass: the convolution output is equal bit for bit; the
    epilogue's sums are within the 2e-6 bound of float64 column sums, and so are the pass's.  The running buffers and the pooled
    activations then differ by what that bound lets through, worked out below from the float64 sums - nothing here is taken from the
    two runs' difference.  With dm, dq the bound on sum / m and sum of squares / m:
      running_mean = 0.1 mean:                     2 x 0.1 dm (one bound per run) + an fp32 rounding each
      running_var = 0.9 + 0.1 var m / (m - 1):     var = q - mean^2, dvar = dq + 2 |mean| dm; 2 x 0.1 dvar m / (m - 1) + roundings
      activation = max over a window of relu(gamma (y - mean) inv + beta), 1-Lipschitz in each unit's argument:
                   |gamma| (inv dm + max |y - mean| dinv) per run, dinv = inv^3 dvar / 2, + the fp32 roundings of
                   fmaf((y - mean) * inv, gamma, beta) per run: mean and inv as floats, the difference, the product, the fmaf."""
    from cet_pick_amd import hipops as H
    from cet_pick_amd.models.networks.moco_encoder_3d import TomoResClassifier3D, BasicBlock
    from cet_pick_amd.synthetic import seeded_state_dict
    n, d, h, w_ = shape
    enc = TomoResClassifier3D(BasicBlock, [2, 2, 2, 2], {"proj": 256, "pred": 256}, 0)
    enc.load_state_dict(seeded_state_dict(enc, seed=317))
    enc = enc.cuda().train()
    conv1, bn1 = enc.conv1, enc.bn1
    bn0 = {k: v.clone() for k, v in bn1.state_dict().items()}
    g = torch.Generator().manual_seed(2500 + sum(shape))
    x = wide(g, n, d, h, w_, 1).cuda()

    def stem_block(env):
        switch(monkeypatch, env)
        bn1.load_state_dict(bn0)
        with torch.no_grad():
            conv1.stats_for_bn = True
            y = conv1(x)
            name = last_kernel()
            sums = conv1.bn_sums
            conv1.bn_sums = None
            used = sums if sums is not None else H.bn_local_sums(y)
            a = H.bn_relu_maxpool3d(y, bn1, 3, 2, 1, sums=sums)
        return y, sums, used.clone(), a, bn1.running_mean.clone(), bn1.running_var.clone(), name

    y_e, sums_e, used_e, a_e, rm_e, rv_e, _ = stem_block({})
    y_p, sums_p, used_p, a_p, rm_p, rv_p, name_p = stem_block({"MI_STEM_NO_STATS": "1"})
    assert sums_e is not None and sums_p is None and name_p == "stem_fwd"      # epilogue statistics / plain stem + statistics pass
    assert torch.equal(y_e, y_p)
    want, scale = _stats_bound(y_e)
    for used in (used_e, used_p):
        assert float(((used - want).abs() / scale).max()) < 2e-6
    m = y_e.numel() // 64
    half_ulp = 2.0 ** -24
    mean, q = want[:64] / m, want[64:] / m
    dm, dq = 2e-6 * scale[:64] / m, 2e-6 * scale[64:] / m
    var = (q - mean * mean).clamp_min(0)
    dvar = dq + 2 * mean.abs() * dm
    rm0, rv0 = bn0["running_mean"].double().abs(), bn0["running_var"].double().abs()
    unb = m / (m - 1.0)
    assert bool(((rm_e - rm_p).abs().double() <= 2 * 0.1 * dm + 6 * half_ulp * (0.9 * rm0 + 0.1 * mean.abs())).all())
    assert bool(((rv_e - rv_p).abs().double() <= 2 * 0.1 * dvar * unb + 6 * half_ulp * (0.9 * rv0 + 0.1 * var * unb)).all())
    inv = (var + bn1.eps).rsqrt()
    dinv = 0.5 * inv ** 3 * dvar
    dev = (y_e.double().reshape(-1, 64) - mean).abs().max(0).values
    gam, bet = bn1.weight.detach().double().abs(), bn1.bias.detach().double().abs()
    bound = 2 * gam * (inv * dm + dev * dinv) + 2 * half_ulp * (gam * inv * (mean.abs() + 4 * dev) + 2 * bet)
    diff = (a_e - a_p).abs().double().reshape(-1, 64).max(0).values
    assert bool((diff <= bound).all()), (float((diff / bound).max()))
    assert float(a_e.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
WG_SHAPES = [(1, 8, 8, 16),        # 1 tile
             (3, 7, 7, 15),        # odd extents
             (2, 24, 8, 32),       # 12 tiles, non-cubic
             (33, 8, 8, 16),       # 33 workgroups: level-1 groups of 2, the last holds one slab
             (130, 16, 16, 16),    # 520 tiles, 2 per workgroup, 252 workgroups own none
             (513, 8, 8, 16),      # workgroup 256: one live tile and one past the end
             (1100, 8, 8, 16)]     # 3 tiles per workgroup, the last live workgroup has two
MANY_TILES = WG_SHAPES[4:]
WG_SETTINGS = [("bf3 occ2", {}), ("bf3 occ1", {"MI_STEM_WGRAD_OCC": "1"}), ("f32", {"MI_STEM_WGRAD_F32": "1"}),
               ("generic", {"MI_CONV_NO_STEM": "1"})]


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape):
    """Inputs and the two CPU weight gradients of a shape, computed once (the three many-tile shapes serve two tests)."""
    n, d, h, w_ = shape
    g = torch.Generator().manual_seed(3000 + sum(shape))
    x = wide(g, n, 1, d, h, w_)
    dy = torch.randn(n, 64, out_extent(d), out_extent(h), out_extent(w_), generator=g)

    def wgrad(dt):
        w = torch.zeros(64, 1, 7, 7, 7, dtype=dt, requires_grad=True)
        return torch.autograd.grad(F.conv3d(x.to(dt), w, stride=2, padding=3), w, dy.to(dt))[0]
    with cpu_reference():
        return x, dy, wgrad(torch.float64), wgrad(torch.float32)


@pytest.mark.parametrize("shape", WG_SHAPES)
def test_stem_weight_gradient_every_variant_matches_float64(shape, monkeypatch):
    """tiles = N (Do / 4) (Ho / 4) (Wo / 8) on at most 512 workgroups of ceil(tiles / 512) tiles each.  Every variant f32-equivalent to
    the float64 weight gradient (the arbiter's error grows with the reduction like the kernel's); two calls of a variant bit-equal
    (slab order, no atomics); a second conv_wgrad_into on the same parameter accumulates - twice the gradient, exactly for that
    reason; the two occupancies of the bf16x3 kernel bit-equal (one kernel body)."""
    from cet_pick_amd import hipops as H
    n, d, h, w_ = shape
    x, dy, gw64, gw32 = _wgrad_case(shape)
    param, _ = make_w(64, 1, 7, torch.Generator().manual_seed(1))
    xc, dyc = cl(x), cl(dy)
    got = {}
    for tag, env in WG_SETTINGS:
        switch(monkeypatch, env)
        runs = []
        for _ in range(2):
            param.grad = None
            H.conv_wgrad_into(xc, dyc, param, 7, 2, 3)
            name = last_kernel()
            assert (name.startswith("implicit GEMM") if tag == "generic" else name == "stem_wgrad"), (tag, name)
            runs.append(param.grad.detach().cpu().clone())
        assert torch.equal(runs[0], runs[1]), tag
        H.conv_wgrad_into(xc, dyc, param, 7, 2, 3)            # param.grad holds the second run: this one accumulates
        assert torch.equal(param.grad.detach().cpu(), 2 * runs[0]), tag
        got[tag] = runs[0]
        e = equivalent(got[tag].numpy(), gw32.numpy(), gw64.numpy(), what="stem wgrad %s %s" % (shape, tag))
        print("stem wgrad %s %-9s kernel %-24s GPU %.3e  CPU fp32 %.3e" % (shape, tag, name, e[0], e[1]))
    assert torch.equal(got["bf3 occ2"], got["bf3 occ1"])


@pytest.mark.parametrize("shape", MANY_TILES)
def test_stem_weight_gradient_from_a_dirty_workspace(shape, monkeypatch):
    """mi_conv_wgrad_f32 with a workspace of mi_conv_workspace_bytes that starts as NaN: every slab the reduce reads must have been
    written - by workgroups that own no tile too -, so the gradient is finite, bit-equal to the run on a zeroed workspace, and
    f32-equivalent to float64."""
    from cet_pick_amd import hipops as H, _lib as L
    lib = L.lib()
    n, d, h, w_ = shape
    x, dy, gw64, gw32 = _wgrad_case(shape)
    xc, dyc = cl(x), cl(dy)
    geom = H._Geom((n, d, h, w_, 1), 64, (7, 7, 7), 2, (3, 3, 3))
    nbytes = lib.mi_conv_workspace_bytes(geom.ref)
    assert nbytes > 0
    for env in ({}, {"MI_STEM_WGRAD_F32": "1"}):               # the bf16x3 and the f32 kernel: the same walk, written twice
        switch(monkeypatch, env)
        dws = []
        for fill in (0x00, 0xFF):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
            dw = torch.full((7, 7, 7, 1, 64), float("nan"), device="cuda")
            L.check(lib.mi_conv_wgrad_f32(L.ptr(xc), L.ptr(dyc), L.ptr(dw), geom.ref, L.ptr(ws), ws.numel(), None, L.stream()), "wgrad")
            assert last_kernel() == "stem_wgrad"
            dws.append(dw.permute(4, 3, 0, 1, 2).cpu())
        assert bool(torch.isfinite(dws[1]).all()), env
        assert torch.equal(dws[0], dws[1]), env
        equivalent(dws[1].numpy(), gw32.numpy(), gw64.numpy(), what="stem wgrad, NaN workspace %s %s" % (shape, env))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. shapes the stem kernels decline
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,co", [((2, 8, 8, 24), 64),        # Wo = 12
                                      ((2, 10, 8, 16), 64),       # Do = 5
                                      ((2, 8, 8, 16), 32)])       # Co = 32
def test_shapes_the_stem_kernels_decline_stay_correct(shape, co, monkeypatch):
    """The silently generic cases: forward and weight gradient f32-equivalent to float64, and not on a stem kernel."""
    from cet_pick_amd import hipops as H
    n, d, h, w_ = shape
    switch(monkeypatch, {})
    g = torch.Generator().manual_seed(4000 + sum(shape) + co)
    x = wide(g, n, 1, d, h, w_)
    param, w = make_w(co, 1, 7, g)
    dy = torch.randn(n, co, out_extent(d), out_extent(h), out_extent(w_), generator=g)

    def chain(dt):
        ww = w.to(dt).requires_grad_(True)
        y = F.conv3d(x.to(dt), ww, stride=2, padding=3)
        return y.detach().permute(0, 2, 3, 4, 1), torch.autograd.grad(y, ww, dy.to(dt))[0]
    with cpu_reference():
        ref64, cpu32 = chain(torch.float64), chain(torch.float32)
    y = H.conv_fwd(cl(x), param, 7, 2, 3)
    names = [last_kernel()]
    param.grad = None
    H.conv_wgrad_into(cl(x), cl(dy), param, 7, 2, 3)
    names.append(last_kernel())
    for i, (got, what) in enumerate(((y, "fwd"), (param.grad.detach(), "wgrad"))):
        assert names[i] != "none" and not names[i].startswith("stem_"), names
        e = equivalent(got.cpu().numpy(), cpu32[i].numpy(), ref64[i].numpy(), what="declined %s %s" % (shape, what))
        print("declined %s Co %d %-5s kernel %-24s GPU %.3e  CPU fp32 %.3e" % (shape, co, what, names[i], e[0], e[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the stem tail: BatchNorm (training mode) + ReLU + MaxPool3d(3, 2, 1)
# ---------------------------------------------------------------------------------------------------------------------------
# (N, D, H, W, C) -> seed.  All four have Wi * C / 4 == 256 and, by mi_maxpool3d_bwd's own formula 2 (band / 2 + 1) Wo C 5 with the
# band clipped to the plane's height, at most 25.6 KB of LDS at any band tried here - (2, 2, 2, 64, 16) has Hi = 2, a band of 2 and
# 10 KB -, so all four take maxpool_bwd_k3s2_kernel unless MI_MAXPOOL_BWD_GENERIC is set.
# The seeds are chosen (on the CPU) so that the float64 and the fp32 chain take the same ReLU decision at every unit and find the same
# arg-max in every pool window; the test asserts it: a flip is a discrete change that no tolerance should absorb.
TAIL_CASES = {(2, 5, 7, 16, 64): 0, (1, 9, 3, 8, 128): 6, (3, 10, 12, 32, 32): 16, (2, 2, 2, 64, 16): 15}
TAIL_NAMES = ("y", "dx", "dweight", "dbias", "running_mean", "running_var")


@functools.lru_cache(maxsize=None)
def _tail_case(shape):
    """Inputs of a tail case and, for float64 and fp32 on the CPU: the six results (channels-last), the ReLU decisions, the arg-max."""
    n, d, h, w_, c = shape
    g = torch.Generator().manual_seed(5000 + TAIL_CASES[shape])
    x = wide(g, n, c, d, h, w_)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    rm0, rv0 = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    dy = torch.randn(n, c, (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w_ - 1) // 2 + 1, generator=g)

    def chain(dt):
        xr, gm, bt = (t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
        rm, rv = rm0.to(dt).clone(), rv0.to(dt).clone()
        pre = F.batch_norm(xr, rm, rv, gm, bt, True, 0.1, 1e-5)
        y, idx = F.max_pool3d(F.relu(pre), 3, 2, 1, return_indices=True)
        gx, gg, gb = torch.autograd.grad(y, (xr, gm, bt), dy.to(dt))
        return ((y.detach().permute(0, 2, 3, 4, 1), gx.permute(0, 2, 3, 4, 1), gg, gb, rm, rv), pre.detach() > 0, idx)
    return (x, gamma, beta, rm0, rv0, dy), chain(torch.float64), chain(torch.float32)


def _tail_gpu(shape, inputs):
    from cet_pick_amd import hipops as H
    x, gamma, beta, rm0, rv0, dy = inputs
    bn = H.HipBatchNorm(shape[-1])
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn = bn.cuda().train()
    xc = cl(x).requires_grad_(True)
    y = H.bn_relu_maxpool3d(xc, bn, 3, 2, 1)
    y.backward(cl(dy))
    assert int(bn.num_batches_tracked) == 1
    return tuple(t.detach().cpu() for t in (y, xc.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var))


@pytest.mark.parametrize("shape", list(TAIL_CASES))
def test_stem_tail_matches_float64(shape, monkeypatch):
    inputs, (ref64, relu64, arg64), (cpu32, relu32, arg32) = _tail_case(shape)
    assert torch.equal(relu64, relu32) and torch.equal(arg64, arg32)       # the condition on the seed
    switch(monkeypatch, {})
    got = _tail_gpu(shape, inputs)
    for name, a, c, r in zip(TAIL_NAMES, got, cpu32, ref64):
        e = equivalent(a.numpy(), c.numpy(), r.numpy(), what="stem tail %s %s" % (shape, name))
        print("stem tail %s %-12s GPU %.3e  CPU fp32 %.3e" % (shape, name, e[0], e[1]))


@pytest.mark.parametrize("shape", list(TAIL_CASES))
def test_stem_tail_tuning_switches(shape, monkeypatch):
    """The pool backward in bands of 2 and 8 rows and on the generic gather kernel visits the same candidates and adds them in the same
    order as the default band of 4: everything behind it is bit-equal.  MI_COLREDUCE_BLOCKS = 1 (the one workgroup's partials are the
    sums) and 3 (partials + finalize) change the grouping of the column sums - BatchNorm's statistics and its backward sums: every
    result stays f32-equivalent to float64."""
    inputs, (ref64, relu64, arg64), (cpu32, relu32, arg32) = _tail_case(shape)
    assert torch.equal(relu64, relu32) and torch.equal(arg64, arg32)
    switch(monkeypatch, {})
    base = _tail_gpu(shape, inputs)
    for env in ({"MI_MAXPOOL_BWD_BAND": "2"}, {"MI_MAXPOOL_BWD_BAND": "8"}, {"MI_MAXPOOL_BWD_GENERIC": "1"}):
        switch(monkeypatch, env)
        for name, a, b in zip(TAIL_NAMES, _tail_gpu(shape, inputs), base):
            assert torch.equal(a, b), (env, name)
    for blocks in ("1", "3"):
        switch(monkeypatch, {"MI_COLREDUCE_BLOCKS": blocks})
        for name, a, c, r in zip(TAIL_NAMES, _tail_gpu(shape, inputs), cpu32, ref64):
            equivalent(a.numpy(), c.numpy(), r.numpy(), what="stem tail %s %s, %s column-reduce blocks" % (shape, name, blocks))
