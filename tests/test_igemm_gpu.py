"""Float64 parity of the implicit-GEMM convolution (csrc/conv_igemm.hip), schedule by schedule: border classes, the parity classes of
the stride-2 data gradient, fold, the weight gradient's voxel box, split-K with its reduce epilogue, every tile instantiation, the
one-input-channel template outside 7^3 and the multiply-shift row decoding.  Every call asserts the kernel family
(mi_debug_last_conv_kernel) and the plan fields the case exists for (mi_debug_last_conv_plan; tests/igemm_cases.py restates the host
rules they follow from), so a case whose schedule is not the intended one fails.

Reference: torch.nn.functional.conv3d on the CPU in float64 with its autograd, the epilogue in float64; arbiter: the same chain in CPU
fp32 through conftest.f32_equivalent (factor 2, floor 2e-6) - for both arithmetics and every tile.  Inputs span a wide dynamic range
(randn * exp(2 randn)).  Each pass runs twice: through hipops (conv_fwd / conv_bias_fwd / conv_dgrad / conv_wgrad_into, .grad None)
and through the C entry into a NaN-filled output with a NaN-filled workspace of exactly mi_conv_workspace_bytes - the two are one
schedule and must agree bit for bit, which no row, tap or slab left unwritten would.

Two schedules of one arithmetic: bit-identical where only zero terms leave an unchanged summation order (fold on / off always; border
classes on / off when neither run is split: a dropped tap is whole slices of exact zeros), else (the voxel box regroups the weight
gradient's slices, a split count regroups every reduction) max|a - b| / max|ref| < 2e-6 sqrt(K / 1728), K the reduction length."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import igemm_cases as C
from igemm_cases import DGRAD, FWD, WGRAD

pytestmark = pytest.mark.gpu

SWITCHES = ("MI_CONV_ARITH", "MI_CONV_NO_BORDER", "MI_CONV_NO_FOLD", "MI_CONV_SPLITS", "MI_CONV_BM", "MI_CONV_BN", "MI_CONV_BK",
            "MI_CONV_NARROW", "MI_CONV_NO_STEM", "MI_CONV_NO_DIRECT", "MI_NO_D32", "MI_CUBE2_REDUCE")
OPS = {FWD: ("fwd", "fwd_res_relu"), DGRAD: ("dgrad", "dgrad_res_mask"), WGRAD: ("wgrad",)}
MODE_OF = {"fwd": FWD, "fwd_res_relu": FWD, "fwd_bias_relu": FWD, "dgrad": DGRAD, "dgrad_res_mask": DGRAD, "wgrad": WGRAD}
ERRORS = {}            # group -> [largest GPU-vs-float64, largest CPU-fp32-vs-float64 error] (printed by the last test)


@pytest.fixture(autouse=True)
def generic_only(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MI_CONV_NO_DIRECT", "1")       # no direct kernel takes the shape ...
    monkeypatch.setenv("MI_CONV_NO_STEM", "1")
    monkeypatch.setenv("MI_NO_D32", "1")               # ... nor an inference kernel conv_bias_fwd's


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


class Problem:
    """One case's tensors (CPU, NCDHW as torch wants them), its float64 / CPU fp32 chains and the device copies."""

    def __init__(self, c):
        from cet_pick_amd import hipops as H
        self.c = c
        g = torch.Generator().manual_seed(1000 + sum(c[:6]) + 7 * sum(c.k3) + c.stride)
        wide = lambda *s: torch.randn(*s, generator=g) * torch.exp(2 * torch.randn(*s, generator=g))
        do, ho, wo = C.out_extent(c)
        self.x = wide(c.n, c.ci, c.d, c.h, c.w)
        self.w = torch.randn(c.co, c.ci, *c.k3, generator=g) * (2.0 / (c.ci * C.taps(c))) ** 0.5
        self.dy = wide(c.n, c.co, do, ho, wo)
        self.res_y, self.bias = torch.randn(c.n, c.co, do, ho, wo, generator=g), torch.randn(c.co, generator=g)
        self.res_x, self.mask = torch.randn(self.x.shape, generator=g), torch.randn(self.x.shape, generator=g)
        self.ref64, self.cpu32 = self.chain(torch.float64), self.chain(torch.float32)
        cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().cuda()
        self.dev = {k: cl(getattr(self, k)) for k in ("x", "dy", "res_y", "res_x", "mask")}
        self.dev["bias"] = self.bias.cuda()
        self.param = H.convnd_weight_param(c.co, c.ci, c.k3)
        with torch.no_grad():
            self.param.copy_(self.w)
        self.param.data = self.param.data.cuda()
        assert H._phys_ok(self.param)
        self.geom = H._Geom((c.n, c.d, c.h, c.w, c.ci), c.co, c.k3, c.stride, c.p3, c.d3)

    def chain(self, dt):
        c = self.c
        x, w = self.x.to(dt).requires_grad_(True), self.w.to(dt).requires_grad_(True)
        # torch's own convolution, not oneDNN's: its fp32 weight gradient does not return for a 7^3 window on a 5 x 6 x 7 volume
        # (only the `enabled` flag is touched, and put back)
        with torch.backends.mkldnn.flags(enabled=False, deterministic=None, allow_tf32=None, fp32_precision=None):
            y = F.conv3d(x, w, stride=c.stride, padding=c.p3, dilation=c.d3)
            gx, gw = torch.autograd.grad(y, (x, w), self.dy.to(dt))
        y = y.detach()
        cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
        return {"fwd": cl(y), "fwd_res_relu": cl(F.relu(y + self.res_y.to(dt))),
                "fwd_bias_relu": cl(F.relu(y + self.bias.to(dt).view(1, -1, 1, 1, 1))),
                "dgrad": cl(gx), "dgrad_res_mask": cl((gx + self.res_x.to(dt)) * (self.mask > 0)), "wgrad": gw}


_PROBLEMS = {}


def problem(c):
    if c not in _PROBLEMS:                # one reference per case, shared by every test that uses it, never written to
        _PROBLEMS[c] = Problem(c)
    return _PROBLEMS[c]


def last_plan():
    from cet_pick_amd import _lib as L
    buf = (ctypes.c_int * 16)()
    n = L.lib().mi_debug_last_conv_plan(ctypes.cast(buf, ctypes.c_void_p), 16)
    assert n == len(C.PLAN_FIELDS)
    plan = dict(zip(C.PLAN_FIELDS, list(buf)[:n]))
    name = L.lib().mi_debug_last_conv_kernel().decode()
    assert name.startswith("implicit GEMM"), name
    return plan


def run_hipops(pb, op):
    """One pass through the public hipops entry; (result on the CPU, plan)."""
    from cet_pick_amd import hipops as H
    c, d = pb.c, pb.dev
    dil = None if c.d3 == (1, 1, 1) else c.d3
    mode = MODE_OF[op]
    route = H.conv_route(mode, (c.n, c.d, c.h, c.w, c.ci), c.ci, c.co, c.k3, c.stride, c.p3, dil, inference=op == "fwd_bias_relu",
                         has_res=op in ("fwd_res_relu", "dgrad_res_mask"), has_bias=op == "fwd_bias_relu", relu=op.endswith("relu"))
    assert route == H.Route("generic", 0), route
    if op == "fwd":
        out = H.conv_fwd(d["x"], pb.param, c.k3, c.stride, c.p3, dil=dil)
    elif op == "fwd_res_relu":
        out = H.conv_fwd(d["x"], pb.param, c.k3, c.stride, c.p3, d["res_y"], True, dil=dil)
    elif op == "fwd_bias_relu":
        with torch.no_grad():
            out = H.conv_bias_fwd(d["x"], pb.param, d["bias"], c.k3, c.stride, c.p3, relu=True)
    elif op == "dgrad":
        out = H.conv_dgrad(d["dy"], pb.param, (c.n, c.d, c.h, c.w, c.ci), c.k3, c.stride, c.p3, dil=dil)
    elif op == "dgrad_res_mask":
        out = H.conv_dgrad(d["dy"], pb.param, (c.n, c.d, c.h, c.w, c.ci), c.k3, c.stride, c.p3, d["res_x"], d["mask"], dil=dil)
    else:
        pb.param.grad = None
        H.conv_wgrad_into(d["x"], d["dy"], pb.param, c.k3, c.stride, c.p3, dil=dil)
        out = pb.param.grad
        pb.param.grad = None
    out = out.detach().cpu()
    return out, last_plan()


def run_entry(pb, op, ws_bytes=None, expect_rc=0):
    """The same pass through the C entry: output and workspace pre-filled with NaN, the workspace exactly as long as
    mi_conv_workspace_bytes asks (ws_bytes: that many bytes of it instead).  (result on the CPU, plan)."""
    from cet_pick_amd import _lib as L
    lib, c, d, g = L.lib(), pb.c, pb.dev, pb.geom
    need = int(lib.mi_conv_workspace_bytes(g.ref))
    assert need > 0
    ws = torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    nbytes = need if ws_bytes is None else ws_bytes
    mode = MODE_OF[op]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    if mode == FWD:
        out = nan(c.n, *C.out_extent(c), c.co)
        res, is_bias = {"fwd": (None, 0), "fwd_res_relu": (d["res_y"], 0), "fwd_bias_relu": (d["bias"], 1)}[op]
        rc = lib.mi_conv_fwd_f32(L.ptr(d["x"]), L.ptr(pb.param), L.ptr(out), L.ptr(res), is_bias, int(op != "fwd"), g.ref, L.ptr(ws),
                                 nbytes, L.stream())
    elif mode == DGRAD:
        out = nan(c.n, c.d, c.h, c.w, c.ci)
        res, mask = (d["res_x"], d["mask"]) if op == "dgrad_res_mask" else (None, None)
        rc = lib.mi_conv_dgrad_f32(L.ptr(d["dy"]), L.ptr(pb.param), L.ptr(out), L.ptr(res), L.ptr(mask), g.ref, L.ptr(ws), nbytes,
                                   L.stream())
    else:
        phys = nan(*c.k3, c.ci, c.co)
        rc = lib.mi_conv_wgrad_f32(L.ptr(d["x"]), L.ptr(d["dy"]), L.ptr(phys), g.ref, L.ptr(ws), nbytes, None, L.stream())
        out = phys.permute(4, 3, 0, 1, 2)
    torch.cuda.synchronize()
    assert rc == expect_rc, rc
    if rc:
        return None, None
    return out.cpu(), last_plan()


def check_plan(plan, mode, c, env, **fields):
    """The fields that follow from shape and switches (igemm_cases.expected_plan), the block count, and the fields the case pins."""
    want = C.expected_plan(mode, c, env)
    rt, ct = want.pop("row_tiles"), want.pop("col_tiles")
    got = {k: plan[k] for k in want}
    assert got == want, (plan, want)
    if "MI_CONV_SPLITS" in env:
        assert plan["splits"] == int(env["MI_CONV_SPLITS"]), plan
    assert plan["splits"] >= 1 and plan["blocks"] == rt * ct * plan["splits"], (plan, rt, ct)
    for k, v in fields.items():
        assert plan[k] == v, (k, plan)


def parity(group, pb, op, got, what):
    from conftest import f32_equivalent
    e_g, e_c = f32_equivalent(got.numpy(), pb.cpu32[op].numpy(), pb.ref64[op].numpy(), what="%s %s %s" % (what, C.case_id(pb.c), op))
    print("igemm %s %s %s: GPU %.3e CPU fp32 %.3e from float64" % (group, C.case_id(pb.c), what + " " + op, e_g, e_c))
    worst = ERRORS.setdefault(group, [0.0, 0.0])
    worst[0], worst[1] = max(worst[0], e_g), max(worst[1], e_c)


def run_checked(group, pb, op, env, what="", **fields):
    """Both paths of one pass: plan, float64 parity, no value left unwritten; the result."""
    out, plan = run_hipops(pb, op)
    check_plan(plan, MODE_OF[op], pb.c, env, **fields)
    parity(group, pb, op, out, what)
    raw, plan2 = run_entry(pb, op)
    assert plan2 == plan, (plan, plan2)
    assert bool(torch.isfinite(raw).all()), "%s %s: values left unwritten" % (C.case_id(pb.c), op)
    assert torch.equal(raw, out), "%s %s: the C entry and hipops disagree" % (C.case_id(pb.c), op)
    return out, plan


def two_orders(pb, op, a, b, what):
    """two fp32 summation orders of one arithmetic: the bound of test_conv_direct3_matches_igemm_and_float64, scaled by sqrt(K)"""
    k = C.reduction_length(MODE_OF[op], pb.c)
    diff = float((a - b).abs().max()) / float(pb.ref64[op].abs().max())
    bound = 2e-6 * (k / 1728.0) ** 0.5
    print("igemm %s %s %s: %.3e (bound %.3e, K = %d)" % (what, C.case_id(pb.c), op, diff, bound, k))
    assert diff < bound, (what, op, diff, bound)


# ---- A: border classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("c,border", C.BORDER, ids=[C.case_id(c) for c, _ in C.BORDER])
def test_border_classes(c, border, arith, monkeypatch):
    """Forward and stride-1 data gradient (with residual + mask) by border class and, MI_CONV_NO_BORDER=1, over the full window: each
    against float64, the two bit-identical where neither is split."""
    pb = problem(c)
    out = {}
    for forced in ({}, {"MI_CONV_SPLITS": "1"}):           # the load model's split count, then both runs unsplit
        for off in (0, 1):
            env = dict(forced, MI_CONV_ARITH=arith, MI_CONV_NO_BORDER=str(off))
            monkeypatch.delenv("MI_CONV_SPLITS", raising=False)
            set_env(monkeypatch, env)
            for op in ("fwd", "fwd_res_relu", "dgrad_res_mask"):
                out[len(forced), off, op] = run_checked("A", pb, op, env, "no_border=%d %s" % (off, arith), border=0 if off else border,
                                                        fold=0 if off else border)
    for op in ("fwd", "fwd_res_relu", "dgrad_res_mask"):
        assert torch.equal(out[1, 0, op][0], out[1, 1, op][0]), (C.case_id(c), op)
        (a, pa), (b, pb_) = out[0, 0, op], out[0, 1, op]
        if pa["splits"] == 1 and pb_["splits"] == 1:
            assert torch.equal(a, b), (C.case_id(c), op)
        else:
            two_orders(pb, op, a, b, "border on/off")


# ---- B: parity classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("c", C.PARITY, ids=C.case_id)
def test_parity_classes(c, arith, monkeypatch):
    """Stride-2 data gradient, with and without residual + mask: 8 classes (some without rows, some without taps), folded."""
    pb = problem(c)
    env = {"MI_CONV_ARITH": arith}
    set_env(monkeypatch, env)
    classes = C.parity_classes(c)
    for op in OPS[DGRAD]:
        out, plan = run_checked("B", pb, op, env, arith, n_classes=8, border=0, fold=1)
        if op == "dgrad" and any(t == 0 and r > 0 for r, t in classes):
            # rows of a class without taps are written, and exactly zero
            reached = pb.ref64["dgrad"].abs().amax(dim=-1) > 0
            assert int((~reached).sum()) * c.ci == sum(r for r, t in classes if t == 0) * c.ci
            assert bool((out[~reached] == 0).all())


# ---- C: the weight gradient's voxel box -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("c,switches,wbox", C.WBOX, ids=[C.case_id(c) + "".join("_%s%s" % (k[8:], v) for k, v in s.items())
                                                         for c, s, _ in C.WBOX])
def test_wgrad_voxel_box(c, switches, wbox, arith, monkeypatch):
    """Weight gradient over the tile's voxel box (Ci % BM == 0) and, MI_CONV_NO_BORDER=1 or a tile that spans taps, over every output voxel."""
    pb = problem(c)
    out = {}
    for off in (0, 1):
        env = dict(switches, MI_CONV_ARITH=arith, MI_CONV_NO_BORDER=str(off))
        set_env(monkeypatch, env)
        out[off], plan = run_checked("C", pb, "wgrad", env, "no_border=%d %s" % (off, arith), wbox=0 if off else wbox,
                                     bm=int(switches.get("MI_CONV_BM", 64)))
        for a in range(c.k3[0]):           # a tap plane that never meets the input (depth 1, padding 1): exactly zero
            if not any(0 <= o * c.stride - c.p3[0] + a * c.d3[0] < c.d for o in range(C.out_extent(c)[0])):
                assert bool((out[off][:, :, a] == 0).all()), (C.case_id(c), a)
    two_orders(pb, "wgrad", out[0], out[1], "voxel box on/off")


# ---- D: split-K -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("c", C.SPLIT_LAYERS, ids=C.case_id)
def test_split_k(c, arith, monkeypatch):
    """MI_CONV_SPLITS 1, 2, 3, a count that divides no slice count and one above the shortest reductions' slice counts (empty splits:
    slabs of zeros), in the three passes with the reduce kernel's epilogues - residual + ReLU, bias row + ReLU, residual + mask."""
    pb = problem(c)
    ops = ("fwd_res_relu", "fwd_bias_relu", "dgrad_res_mask", "wgrad")
    out = {}
    for sp in C.SPLITS:
        env = {"MI_CONV_ARITH": arith, "MI_CONV_SPLITS": str(sp)}
        set_env(monkeypatch, env)
        for op in ops:
            out[sp, op], _ = run_checked("D", pb, op, env, "splits=%d %s" % (sp, arith), splits=sp)
    for sp in C.SPLITS[1:]:
        for op in ops:
            two_orders(pb, op, out[1, op], out[sp, op], "splits 1/%d" % sp)


@pytest.mark.parametrize("c", C.SPLIT_LAYERS, ids=C.case_id)
def test_split_k_short_workspace(c, monkeypatch):
    """A workspace one byte short of the slabs: MI_OK, the unsplit schedule (plan splits == 1) and its exact values."""
    pb = problem(c)
    for op in ("fwd_res_relu", "fwd_bias_relu", "dgrad_res_mask", "wgrad"):
        monkeypatch.setenv("MI_CONV_SPLITS", "1")
        want, plan1 = run_entry(pb, op)
        assert plan1["splits"] == 1
        monkeypatch.setenv("MI_CONV_SPLITS", "3")
        full, plan3 = run_entry(pb, op)
        assert plan3["splits"] == 3
        out_elems = want.numel()
        got, plan = run_entry(pb, op, ws_bytes=4 * out_elems * 3 - 1)
        assert plan["splits"] == 1 and plan["blocks"] * 3 == plan3["blocks"], (plan, plan3)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want), (C.case_id(c), op)
        parity("D", pb, op, got, "short workspace")


# ---- E: tiles ---------------------------------------------------------------------------------------------------------------------
def _sw_id(s):
    return "_".join("%s%s" % (k[8:], v) for k, v in s.items()) or "default"


def _tiles(group, c, switches, arith, monkeypatch):
    pb = problem(c)
    env = dict(switches, MI_CONV_ARITH=arith)
    set_env(monkeypatch, env)
    seen = {}
    for mode in (FWD, DGRAD, WGRAD):
        for op in OPS[mode]:
            _, plan = run_checked(group, pb, op, env, "%s %s" % (_sw_id(switches), arith))
        seen[mode] = (plan["bm"], plan["bn"], plan["bk"], plan["bf16x3"])
    return seen


@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("switches", C.TILE_SWITCHES, ids=_sw_id)
@pytest.mark.parametrize("c", C.TILE_SHAPES, ids=C.case_id)
def test_tile_overrides(c, switches, arith, monkeypatch):
    """64/128 x 64/128 x 16/32/64 through MI_CONV_BM / BN / BK under both arithmetics, rows M with M % 64 = 1, 63 and M < 64; the
    (bm, bn, bk, bf16x3 kernel) of each pass as make_plan and launch_mode choose them (check_plan), the corners spelled out here."""
    seen = _tiles("E", c, switches, arith, monkeypatch)
    bf = int(arith == "bf16x3")
    if not switches:
        assert seen[FWD] == seen[DGRAD] == seen[WGRAD] == (64, 64, 32, bf)
    if switches == {"MI_CONV_BM": "128", "MI_CONV_BK": "64"}:
        assert seen[FWD] == seen[DGRAD] == seen[WGRAD] == (128, 64, 64, 0)
    if switches == {"MI_CONV_BK": "64"}:                   # 64-deep slices only with 128-row tiles
        assert seen[FWD] == (64, 64, 32, bf)
    if switches == {"MI_CONV_BM": "128", "MI_CONV_BN": "128"}:
        assert seen[FWD] == seen[WGRAD] == (128, 128, 32, 0)
        assert seen[DGRAD] == ((128, 128, 32, 0) if c.ci % 128 == 0 else (128, 64, 32, 0))
    if switches == {"MI_CONV_BN": "128"}:
        assert seen[FWD] == (64, 128, 32, 0)
    if switches == {"MI_CONV_BK": "16"}:
        assert seen[FWD] == seen[WGRAD] == (64, 64, 16, bf)


@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("switches", C.RAGGED_SWITCHES, ids=_sw_id)
@pytest.mark.parametrize("c", C.RAGGED_CHANNELS, ids=C.case_id)
def test_tile_ragged_channels(c, switches, arith, monkeypatch):
    """Co 16, 48, 80: a column tile partly empty or ragged; Ci 16, 48: 16-deep slices, which MI_CONV_BK=32 cannot widen."""
    seen = _tiles("E", c, switches, arith, monkeypatch)
    bm = int(switches.get("MI_CONV_BM", 64))
    bf = int(arith == "bf16x3" and bm == 64)
    assert seen[FWD] == (bm, 64, 32 if c.ci % 32 == 0 else 16, bf)
    assert seen[DGRAD] == (bm, 64, 32 if c.co % 32 == 0 else 16, bf)
    assert seen[WGRAD] == (bm, 64, 32, bf)


# ---- F: one input channel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.STEM, ids=C.case_id)
def test_stem_template(c, monkeypatch):
    """Ci = 1 with 27, 125 and 343 taps (less than one 32-deep slice, ragged last slices), stride 1 and 2: forward and weight
    gradient on the f32-MFMA stem template; no data gradient."""
    pb = problem(c)
    env = {}
    for op in ("fwd", "fwd_res_relu", "wgrad"):
        run_checked("F", pb, op, env, stem=1, bf16x3=0, bk=32, bn=64, border=0, n_classes=1, wbox=0)
    run_entry(pb, "dgrad", expect_rc=-3)                   # MI_E_UNSUPPORTED


# ---- G: fold ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,mode,splits", C.FOLD, ids=["%s_%s" % (C.case_id(c), m) for c, m, _ in C.FOLD])
def test_fold(c, mode, splits, monkeypatch):
    """A class launch of more than 512 blocks, no multiple of 256: groups of 256 workgroups walk the work list from both ends.
    MI_CONV_NO_FOLD=1 only places the workgroups differently: bit-identical."""
    pb = problem(c)
    out = {}
    for off in (0, 1):
        env = {"MI_CONV_SPLITS": str(splits), "MI_CONV_NO_FOLD": str(off)}
        set_env(monkeypatch, env)
        for op in OPS[mode]:
            out[off, op], plan = run_checked("G", pb, op, env, "no_fold=%d" % off, fold=1 - off, splits=splits)
            assert plan["blocks"] > 512 and plan["blocks"] % 256 != 0, plan
    for op in OPS[mode]:
        assert torch.equal(out[0, op], out[1, op]), (C.case_id(c), op)


# ---- H: row decoding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_border", [0, 1])
@pytest.mark.parametrize("c", C.DECODE, ids=C.case_id)
def test_row_decoding(c, no_border, monkeypatch):
    """Prime and non-power-of-two extents: the multiply-shift division of the row index by W, H, D - the host's constants on the plain
    schedule, the kernel's own per class."""
    pb = problem(c)
    env = {"MI_CONV_NO_BORDER": str(no_border)}
    set_env(monkeypatch, env)
    for mode in (FWD, DGRAD):
        for op in OPS[mode]:
            run_checked("H", pb, op, env, "no_border=%d" % no_border, border=1 - no_border)


def test_zz_report():
    """The largest errors seen per group (pytest -s shows them)."""
    for group in sorted(ERRORS):
        print("igemm group %s: largest GPU-vs-float64 %.3e, largest CPU-fp32-vs-float64 %.3e" % (group, *ERRORS[group]))
