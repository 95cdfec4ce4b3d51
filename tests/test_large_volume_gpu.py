"""Inference at real tomogram sizes: 1024 x 1024 planes, operands past 2 GiB, volumes past 2^29 and 2^31 voxels.

The kernels address an operand with 32-bit byte offsets; each volume entry has its own size limit, and above it the call
takes another path or refuses:
- detector 3-D head (models/networks/unet_small.py `head_z_slabs`): every launch's operand below 0x7fff0000 bytes - the
  d32 convolution declines above it (conv_d32.hip:352), so do the small-K one (hipops.py:380) and direct3
  (conv_direct3.hip:1177), and the implicit GEMM refuses a batch of one (conv_igemm.hip:1173).  The forward runs the head
  per batch item on z-slabs of (0x7fff0000 - 1) // plane - 6 planes and a three-plane halo.
- mi_dog_pick: below 2^31 voxels (infer_greedy.hip:1332), refused above.  The fused z + x | y chain takes volumes below
  2^29 voxels (infer_dogf.hip:370); above it, 512-wide rows go to the DoG + NMS x-pass kernel (infer_dogx.hip:282, no size
  predicate), wider rows to the generic march chain.  Rows wider than 512 get the 60-voxel xy border (infer_greedy.hip,
  `bxy_f` / `bxy`).  The wrapper's default max_out grows with the volume past 2^27 voxels (utils/image.py `dog_pick`);
  more picks than max_out raise.
- mi_sigmoid_nms_topk: below 2^32 voxels (infer_nms.hip:749); its peak3 march below 2^32 as well (infer_peak3.hip:263),
  MI_NO_PEAK3 selects the window march.

Every comparison is against a plain reference: the float64 oracles, the same net on a 7-plane window (under every
limit, pinned to the oracle by test_unet_gpu.py), or the defining properties of greedy NMS.
"""
import numpy as np
import pytest
import torch

from cet_pick_amd.synthetic import make_tomo

pytestmark = pytest.mark.gpu

HEADS = {"hm": 1, "proj": 32}
SIGMAS = (3, 5)
RADIUS = int(4.0 * SIGMAS[-1] + 0.5)          # the larger Gaussian's radius (truncate = 4): a DoG plane reads +-20 planes


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    from cet_pick_amd import _lib as L
    for tag in ("dog", "decode", "greedy"):      # cached workspaces of these sizes run to tens of GB
        L.drop_workspace(torch.device("cuda", torch.cuda.current_device()), tag)
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------------- detector
@pytest.fixture(scope="module")
def net():
    from cet_pick_amd.models.networks.unet_small import TomoConvUNet
    from cet_pick_amd.synthetic import seeded_state_dict
    m = TomoConvUNet(4, HEADS, 32, 3)
    m.load_state_dict(seeded_state_dict(m, seed=321))
    return m.cuda().eval()


def _planes_to_check(b, d):
    """First and last planes, both sides of every slab seam, and the planes whose feature-volume byte offset crosses
    2^31 and 2^32 (32-channel 512 x 512 planes of 32 MiB, batch items back to back)."""
    from cet_pick_amd.models.networks.unet_small import head_z_slabs
    plane = 4 * 512 * 512 * 32
    want = set()
    for i in range(b):
        want |= {(i, 0), (i, d - 1)}
    for i, z0, _, _, _ in head_z_slabs(b, d, plane) or []:
        if z0 > 0:
            want |= {(i, z0 - 1), (i, z0)}
    for crossing in (1 << 31, 1 << 32):
        flat = crossing // plane
        for f in (flat - 1, flat):
            if 0 <= f < b * d:
                want.add(divmod(f, d))
    return sorted(want)


@pytest.mark.parametrize("b,d", [(1, 63), (1, 64), (1, 65), (1, 160), (2, 40)])
def test_detector_1024x1024_equals_7_plane_windows(net, b, d):
    """A plane's head outputs read three input planes on either side: the net on the 7-plane window [z-3, z+3] (the volume's
    own zero padding at its ends) gives them under every operand limit.  d >= 64 puts a 2 GiB feature volume in front of the
    head, b = 2 one of 2.5 GiB across two batch items."""
    g = torch.Generator(device="cuda").manual_seed(1000 + 7 * d + b)
    x = torch.randn(b, d, 1024, 1024, device="cuda", generator=g)
    with torch.no_grad():
        out = net(x)[0]
        for h, c in HEADS.items():
            assert tuple(out[h].shape) == (b, c, d, 512, 512)
        for i, z in _planes_to_check(b, d):
            lo, hi = max(0, z - 3), min(d, z + 4)
            ref = net(x[i:i + 1, lo:hi])[0]
            for h in HEADS:
                r = ref[h][0, :, z - lo]
                err = float((out[h][i, :, z] - r).abs().max())
                assert err <= 2e-6 * max(1.0, float(r.abs().max())), (h, i, z, err)
    del out, x
    torch.cuda.empty_cache()


def test_detector_1024x1024_vs_float64_oracle(net):
    """Two planes of a 160-plane 1024 x 1024 tomogram, one in the last head slab, against the float64 oracle on their
    7-plane windows."""
    from cet_pick_amd.models.networks.unet_small import head_z_slabs
    from oracle import unet_ref as O
    d = 160
    slabs = head_z_slabs(1, d, 4 * 512 * 512 * 32)
    assert slabs is not None and len(slabs) >= 3
    last = slabs[-1][1]
    g = torch.Generator(device="cuda").manual_seed(1160)
    x = torch.randn(1, d, 1024, 1024, device="cuda", generator=g)
    with torch.no_grad():
        out = net(x)[0]
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    for z in (slabs[1][1] + 2, last + 20):
        lo, hi = z - 3, z + 4
        ref = O.tomo_conv_unet_forward(sd, x[:, lo:hi].cpu().double(), 4, HEADS)
        for h in HEADS:
            r = ref[h][0, :, z - lo].numpy()
            got = out[h][0, :, z].double().cpu().numpy()
            np.testing.assert_allclose(got, r, rtol=0, atol=3e-4 * np.abs(r).max(), err_msg="%s z=%d" % (h, z))
    del out, x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------- DoG picker
def _assert_heat_close(got, ref, what):
    """The NMS'd DoG map, fp32 against float64: values equal to rounding where both keep the voxel; the kept / zeroed
    decisions differ only on near-ties (a handful per ten million voxels)."""
    got = np.asarray(got, np.float64)
    scale = float(np.abs(ref).max())
    kg, kr = got != 0, ref != 0
    both = kg & kr
    err = float(np.abs(got[both] - ref[both]).max()) if both.any() else 0.0
    assert err <= 2e-5 * scale, (what, err, scale)
    flips = int((kg != kr).sum())
    assert flips <= 16 + ref.size // 100000, (what, flips, ref.size)


def _strong_picks_agree(s, c, so, co, cut):
    strong_o = {tuple(r) for r, sc in zip(co, so) if sc > cut * 1.01}
    strong_g = {tuple(r) for r, sc in zip(c, s) if sc > cut * 1.01}
    assert strong_o == strong_g
    assert abs(len(s) - len(so)) <= max(2, len(so) // 100)


@pytest.mark.parametrize("shape", [(40, 600, 1030), (48, 1024, 1024)])
def test_dog_pick_wider_than_512_vs_oracle(shape):
    """Planes wider than 512: the 60-voxel xy border, rows the fused 512-wide kernels do not take (1030) or do (1024)."""
    from oracle import infer_ref as O
    from cet_pick_amd.utils import image as Im
    vol, _ = make_tomo(shape, seed=331)
    s, c, n, cut, heat = Im.dog_pick(torch.as_tensor(vol).cuda(), list(SIGMAS), return_heat=True)
    n = int(n.item())
    assert n > 20
    s, c, cut, heat = s[:n].cpu().numpy(), c[:n].cpu().numpy(), float(cut.item()), heat.cpu().numpy()
    heat_o = O.dog_nms_heat(vol.astype(np.float64), SIGMAS)
    cut_o = O.pos_threshold(heat_o)
    so, co = O.non_maximum_suppression_3d(heat_o, 14, threshold=cut_o)
    assert abs(cut - cut_o) <= 1e-5 * abs(cut_o), (cut, cut_o)
    _assert_heat_close(heat, heat_o, shape)
    assert not heat[:, :60].any() and not heat[:, -60:].any() and not heat[:, :, :60].any() and not heat[:, :, -60:].any()
    _strong_picks_agree(s, c, so, co, cut_o)
    # the host wrapper returns the same picks
    s2, c2 = Im.get_potential_coords_pyramid(vol, sigmas=list(SIGMAS))
    np.testing.assert_array_equal(c2, c)
    np.testing.assert_array_equal(s2, s)


def _ball_max(shape, c, s, r):
    """M[v] = the highest score of a pick within distance r of voxel v (0 where there is none)."""
    D, H, W = shape
    P = torch.zeros(shape, device="cuda")
    P[c[:, 2], c[:, 1], c[:, 0]] = s
    M = torch.zeros_like(P)
    w = int(np.floor(r))
    for dz in range(-w, w + 1):
        for dy in range(-w, w + 1):
            for dx in range(-w, w + 1):
                if dz * dz + dy * dy + dx * dx > r * r:
                    continue
                dst = M[max(0, dz):D + min(0, dz), max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)]
                src = P[max(0, -dz):D + min(0, -dz), max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
                torch.maximum(dst, src, out=dst)
    del P
    return M


def _windows(D, plane_bytes):
    """z-windows of 2 * RADIUS + 2 planes at the start, the middle, the 2^31-byte plane and the end, each with the planes
    of it that the window's own ends do not disturb (at least RADIUS planes from an end that is not the volume's)."""
    out = []
    for zc in (0, D // 2, (1 << 31) // plane_bytes, D):
        lo = min(max(0, zc - RADIUS - 1), D - 2 * RADIUS - 2)
        hi = lo + 2 * RADIUS + 2
        keep = [z for z in range(lo, hi) if (lo == 0 or z - lo >= RADIUS) and (hi == D or hi - 1 - z >= RADIUS)]
        if (lo, hi) not in [(a, b) for a, b, _ in out]:
            out.append((lo, hi, keep))
    return out


@pytest.mark.parametrize("shape", [(2080, 512, 512), (520, 1024, 1024)])
def test_dog_pick_past_2gib(shape):
    """More than 2^29 voxels (2.03 GiB of fp32): the fused chain declines and the picker runs its fallback chain.  The heat
    map against the float64 oracle on z-windows, the cutoff against its definition, the picks against the definition of
    greedy NMS (the oracle's own greedy pass would take minutes here)."""
    from oracle import infer_ref as O
    from cet_pick_amd import _lib as L
    from cet_pick_amd.utils import image as Im
    D, H, W = shape
    bxy = 60 if (H > 512 and W > 512) else 30
    vol, _ = make_tomo(shape, seed=332)
    v = torch.as_tensor(vol).cuda()
    s, c, n, cut, heat = Im.dog_pick(v, list(SIGMAS), max_out=1 << 21, return_heat=True)
    n = int(n.item())
    assert n > (1 << 17), n
    s, c, cut = s[:n], c[:n].long(), float(cut.item())
    # the default max_out holds every pick of such a tomogram (both sizes give more than 128 Ki, the cap it once had)
    s2, c2 = Im.get_potential_coords_pyramid(v, sigmas=list(SIGMAS))
    np.testing.assert_array_equal(c2, c.int().cpu().numpy())
    np.testing.assert_array_equal(s2, s.cpu().numpy())
    # and a max_out below the pick count: an overflow code from the device call, an error from the wrapper
    _, _, n_small, _, _ = Im.dog_pick(v, list(SIGMAS), max_out=64)
    assert int(n_small.item()) < 0
    with pytest.raises(L.HipExtensionError):
        Im.get_potential_coords_pyramid(v, sigmas=list(SIGMAS), max_out=64)
    del v
    L.drop_workspace(heat.device, "dog")                                        # (~37 GB: the checks below need room)
    torch.cuda.empty_cache()
    # the heat map, window by window
    for lo, hi, keep in _windows(D, 4 * H * W):
        ref = O.dog_nms_heat(vol[lo:hi].astype(np.float64), SIGMAS)
        k = np.asarray(keep) - lo
        _assert_heat_close(heat[lo:hi].cpu().numpy()[k], ref[k], (shape, lo, hi))
    z0 = heat[:10].abs().max(), heat[-10:].abs().max(), heat[:, :bxy].abs().max(), heat[:, :, -bxy:].abs().max()
    assert all(float(t) == 0.0 for t in z0)
    # the cutoff: mean + 0.5 x (unbiased) std of the positive heat, in float64
    pos = heat[heat > 0].double()
    thr = float(pos.mean() + 0.5 * pos.std())
    del pos
    assert abs(cut - thr) <= 1e-5 * abs(thr), (cut, thr)
    # the picks: sorted, above the cutoff, carrying their heat value
    assert torch.all(s[:-1] >= s[1:]) and float(s[-1]) > cut
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    assert torch.all((z >= 10) & (z < D - 10) & (y >= bxy) & (y < H - bxy) & (x >= bxy) & (x < W - bxy))
    assert torch.equal(heat[z, y, x], s)
    # no pick within d / 2 = 7 of a higher one (the greedy order: of an earlier one)
    p = c.float()
    for i0 in range(0, n, 4096):
        i1 = min(n, i0 + 4096)
        dist = torch.cdist(p[i0:i1], p[:i1])                                     # (each pair once, itself excluded)
        dist[:, i0:i1].masked_fill_(torch.ones(i1 - i0, i1 - i0, dtype=torch.bool, device="cuda").triu(), 1e9)
        assert float(dist.min()) > 7.0, i0
    del dist
    # every voxel above the cutoff that is not a pick lies within d / 2 of a pick at least as high
    M = _ball_max(shape, c, s, 7.0)
    bad = int(((heat > cut) & (M < heat)).sum())
    del M
    assert bad == 0, bad
    del heat


def test_dog_pick_refuses_2_pow_31_voxels():
    """2^31 voxels: refused by the size predicate, before any workspace of the volume's size is allocated (the input is
    never read: torch.empty)."""
    from cet_pick_amd import _lib as L
    from cet_pick_amd.utils import image as Im
    v = torch.empty((2048, 1024, 1024), device="cuda")
    before = torch.cuda.memory_allocated()
    with pytest.raises(L.HipExtensionError):
        Im.dog_pick(v, list(SIGMAS))
    assert torch.cuda.memory_allocated() - before < (1 << 24)
    del v


# ------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("peak3", [True, False])
def test_decode_past_2_pow_31_voxels(peak3, monkeypatch):
    """2056 x 1024 x 1024 (2^31 + 2^23 voxels, 8.6 GB of logits): the top-K are planted in the last 8 planes, past the
    2^31st element - distinct after the sigmoid's clamp, above every background voxel - and come back in order, with the
    exact coordinates and their heat values; the heat map is the float64 sigmoid, clamped."""
    from cet_pick_amd.models import decode as Dm
    if not peak3:
        monkeypatch.setenv("MI_NO_PEAK3", "1")
    D, H, W = 2056, 1024, 1024
    K = 64
    g = torch.Generator(device="cuda").manual_seed(2056)
    logits = torch.empty((1, 1, D, H, W), device="cuda")
    for z0 in range(0, D, 256):
        blk = logits[0, 0, z0:z0 + 256]
        torch.rand(blk.shape, device="cuda", generator=g, out=blk)
        blk.mul_(-6.0).sub_(1.0)                                                # background in (-7, -1]
    i = torch.arange(K, device="cuda")
    zs, ys, xs = 2048 + i % 8, 40 + 29 * (i // 8), 60 + 13 * i                  # >= 2 apart: each its own 3 x 3 x 3 maximum
    vals = 2.0 + 0.1 * i.float()                                                # 2.0 .. 8.3 (< 9: distinct after the clamp)
    logits[0, 0, zs, ys, xs] = vals
    assert int(zs.min()) * H * W >= (1 << 31)
    heat, dets = Dm.sigmoid_tomo_decode(logits, kernel=3, K=K)
    d = dets[0]
    order = torch.argsort(vals, descending=True)
    assert torch.equal(d[:, 0], xs[order].float() + 0.25)
    assert torch.equal(d[:, 1], ys[order].float() + 0.25)
    assert torch.equal(d[:, 2], zs[order].float())
    assert torch.equal(d[:, 3], d[:, 4])
    assert torch.equal(d[:, 3], heat[0, 0, zs[order], ys[order], xs[order]])
    want = torch.clamp(torch.sigmoid(vals[order].double()), 1e-4, 1 - 1e-4)
    assert float((d[:, 3].double() - want).abs().max()) <= 2e-6
    assert torch.all(d[:-1, 3] > d[1:, 3])
    worst = 0.0
    for z0 in range(0, D, 128):
        ref = torch.clamp(torch.sigmoid(logits[0, 0, z0:z0 + 128].double()), 1e-4, 1 - 1e-4)
        worst = max(worst, float((heat[0, 0, z0:z0 + 128].double() - ref).abs().max()))
    assert worst <= 2e-6, worst
    del logits, heat
