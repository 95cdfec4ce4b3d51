"""Characterisation of the convolution routing in cet_pick_amd/hipops.py: for every case of tests/conv_route_cases.py the public
function is called once on small random tensors with the loaded library wrapped in a proxy that logs every mi_* entry called and
its scalar arguments.  The sequence of launching entries, mi_debug_last_conv_kernel() and (under bench.py's roofline pass) the
PROFILE records must equal tests/golden/conv_routes.json, which this same test wrote in its record mode
(CONV_ROUTE_RECORD=<file> CONV_ROUTE_COMMIT=<hash>, test_record) at the commit named inside the file.

Logged per entry: its Python int / float arguments in order; pointer arguments and the c_size_t ones (workspace sizes: they
depend on what the workspace cache held before) are left out, a geometry passed by reference is logged as its sixteen ints."""
import ctypes
import json
import os

import pytest
import torch

from conftest import GOLDEN
from conv_route_cases import CASES

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "conv_routes.json")
NOT_LAUNCHING = ("_bytes", "_usable", "_kind")
SWITCHES = ("MI_CONV_ARITH", "MI_CUBE2_REDUCE", "MI_NO_P2D", "MI_NO_P2D_WGRAD", "MI_NO_STEM2D", "MI_NO_D32", "MI_CONV_NO_DIRECT",
            "MI_CONV_NO_STEM", "MI_D32_1X1_256")


class LoggingLib:
    """Stands in for the ctypes library object: attribute lookup of an mi_* entry returns a wrapper that logs the call."""

    def __init__(self, real, signatures):
        self._real, self._sig, self.log = real, signatures, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("mi_"):
            return fn
        argtypes = self._sig[name][1]

        def logged(*args):
            scalars = []
            for a, t in zip(args, argtypes):
                if t is ctypes.c_void_p or t is ctypes.c_size_t:
                    continue
                if hasattr(a, "_obj"):                              # byref(mi_conv_geom)
                    scalars += [int(getattr(a._obj, f)) for f, _ in a._obj._fields_]
                elif isinstance(a, (int, float)):
                    scalars.append(a if isinstance(a, float) else int(a))
            self.log.append([name, scalars])
            return fn(*args)
        return logged


def _weight(co, ci, k3, nd5, param):
    phys = (torch.randn(*k3, ci, co) if nd5 else torch.randn(k3[1], k3[2], ci, co)).cuda() / (ci * k3[0] * k3[1] * k3[2]) ** 0.5
    w = phys.permute(4, 3, 0, 1, 2) if nd5 else phys.permute(3, 2, 0, 1)
    return torch.nn.Parameter(w) if param else w


def _out_buffer(kind, shape):
    if kind == "dense":
        return torch.empty(shape, device="cuda"), None
    wide = torch.empty(tuple(shape[:-1]) + (2 * shape[-1],), device="cuda")
    return wide[..., shape[-1]:], wide


def run_case(case, H, monkeypatch):
    """Call the case's public function once (the caller has the logging proxy in place); returns what it returned."""
    torch.manual_seed(7)
    shape, co = tuple(case["shape"]), case["co"]
    nd5, ci = len(shape) == 5, shape[-1]
    k, stride, pad, dil = case["k"], case["stride"], case["pad"], case.get("dil")
    k3, p3 = H._k3(k, nd5), H._p3(pad, nd5)
    d3 = H._k3(dil, nd5) if dil is not None else (1, 1, 1)
    sp = shape[1:-1] if nd5 else (1,) + shape[1:-1]
    osp = tuple((v + 2 * p - dl * (kk - 1) - 1) // stride + 1 for v, kk, p, dl in zip(sp, k3, p3, d3))
    oshape = (shape[0],) + (osp if nd5 else osp[1:]) + (co,)
    op = case["op"]
    images = None
    if op in ("s2_fwd", "s2_dgrad"):
        w, w_ds = _weight(co, ci, (3, 3, 3), True, False), _weight(co, ci, (1, 1, 1), True, False)
        if case.get("images"):
            images = H.WeightImages()
            images.add("g", "s2", w, op == "s2_dgrad", w_ds)
            images.refresh_all()
        declined = "declined" in case["id"]          # (no launch: the operands are never read, one float stands for them)
        make = (lambda s: torch.zeros(1, device="cuda").expand(s)) if declined else (lambda s: torch.randn(s, device="cuda"))
    elif op in ("fwd", "bias_fwd", "dgrad", "wgrad"):
        w = _weight(co, ci, k3, nd5, op == "wgrad")
        if case.get("images"):
            images = H.WeightImages()
            for dgrad in (False, True):
                images.add("g", "direct" if nd5 else "p2d", w, dgrad)
            images.refresh_all()
    for name, value in (case.get("attrs") or {}).items():
        monkeypatch.setattr(H, name, value)
    for name, value in (case.get("env") or {}).items():
        monkeypatch.setenv(name, value)
    if case.get("images") == "active":
        monkeypatch.setattr(H, "ACTIVE_IMAGES", images)
    if case.get("profile"):
        monkeypatch.setattr(H, "PROFILE", [])
    res_of = lambda s: torch.randn(s, device="cuda") if case.get("res") else None
    with torch.no_grad():
        if op == "fwd":
            return H.conv_fwd(torch.randn(shape, device="cuda"), w, k, stride, pad, res_of(oshape), bool(case.get("relu")), dil=dil,
                              inference=bool(case.get("inference")))
        if op == "bias_fwd":
            out = _out_buffer(case["out"], oshape)[0] if case.get("out") else None
            return H.conv_bias_fwd(torch.randn(shape, device="cuda"), w, torch.randn(co, device="cuda"), k, stride, pad,
                                   bool(case.get("relu")), out=out, pool=bool(case.get("pool")))
        if op == "dgrad":
            mask = torch.randn(shape, device="cuda") if case.get("mask") else None
            return H.conv_dgrad(torch.randn(oshape, device="cuda"), w, shape, k, stride, pad, res_of(shape), mask, dil=dil)
        if op == "wgrad":
            if case.get("acc"):
                w.grad = torch.zeros_like(w)
            if case.get("deferred"):
                monkeypatch.setattr(H, "DEFERRED_WGRADS", [])
            H.conv_wgrad_into(torch.randn(shape, device="cuda"), torch.randn(oshape, device="cuda"), w, k, stride, pad, dil=dil)
            if case.get("deferred"):
                H.flush_wgrad_reduces()
            return w.grad
        if op == "s2_fwd":
            return H.conv_fwd_s2_block(make(shape), w, w_ds)
        if op == "s2_dgrad":
            mask = torch.randn(shape, device="cuda") if case.get("mask") else None
            return H.conv_dgrad_s2_block(make(oshape), make(oshape), w, w_ds, shape, res_of(shape), mask)
        bn = H.HipBatchNorm(co).cuda().eval()
        bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
        if op == "upconv":
            up = H.HipConvTranspose2x2(ci, co).cuda()
            n, h, wd, _ = shape
            if case.get("cat"):
                cat = torch.randn(n, 2 * h, 2 * wd, 2 * co, device="cuda")
                return H.upconv_bn_relu_concat(up, bn, torch.randn(shape, device="cuda"), cat[..., co:], cat=cat)
            return H.upconv_bn_relu_concat(up, bn, torch.randn(shape, device="cuda"), torch.randn(n, 2 * h, 2 * wd, co, device="cuda"))
        conv = H.HipConv2d(ci, co, k, stride, pad).cuda()
        if op == "skip_ok":
            return bool(H.skip_into_concat_ok(conv, bn, torch.randn(shape, device="cuda"), 32 if co == 48 else co))
        assert op == "conv_bn"
        out = _out_buffer(case["out"], oshape)[0] if case.get("out") else None
        return H.conv_bn(conv, bn, torch.randn(shape, device="cuda"), relu=bool(case.get("relu")), pool=bool(case.get("pool")), out=out)


def observe(case, monkeypatch):
    """What the case does: launching entries with their scalars, the library's kernel name, the result's form, PROFILE records."""
    from cet_pick_amd import hipops as H, _lib as L
    real = L.lib()
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    # a fixed generic convolution first: entries that leave mi_debug_last_conv_kernel alone then show its name, not the last case's
    H.conv_fwd(torch.zeros(1, 3, 3, 3, 16, device="cuda"), _weight(32, 16, (1, 1, 1), True, False), 1, 1, 0)
    proxy = LoggingLib(real, L.SIGNATURES)
    with monkeypatch.context() as mp:
        mp.setattr(L, "_lib", proxy)
        got = run_case(case, H, mp)
        profile = H.PROFILE
    torch.cuda.synchronize()
    if isinstance(got, bool):
        form = got
    elif got is None:
        form = None
    else:
        form = [list(t.shape) for t in (got if isinstance(got, tuple) else (got,))]
    seen = {"calls": [c for c in proxy.log if not c[0].endswith(NOT_LAUNCHING)], "last_kernel": real.mi_debug_last_conv_kernel().decode(),
            "returns": form}
    if profile is not None:
        seen["profile"] = [[p[0], p[1], p[4]] for p in profile]
    return seen


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.skipif(not os.environ.get("CONV_ROUTE_RECORD"), reason="record mode only (CONV_ROUTE_RECORD=<file> CONV_ROUTE_COMMIT=<hash>)")
def test_record(monkeypatch):
    rec = {"recorded_at_commit": os.environ["CONV_ROUTE_COMMIT"], "cases": []}
    for case in CASES:
        with monkeypatch.context() as mp:
            rec["cases"].append({"case": case, "seen": observe(case, mp)})
    with open(os.environ["CONV_ROUTE_RECORD"], "w") as f:
        json.dump(rec, f, indent=0, separators=(",", ":"))
        f.write("\n")


def test_record_has_every_case(record):
    assert [c["case"] for c in record["cases"]] == json.loads(json.dumps(list(CASES)))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_route_is_the_recorded_one(index, record, monkeypatch):
    entry = record["cases"][index]
    assert entry["case"]["id"] == CASES[index]["id"]
    seen = json.loads(json.dumps(observe(CASES[index], monkeypatch)))
    want = entry["seen"]
    assert [c[0] for c in seen["calls"]] == [c[0] for c in want["calls"]]
    assert seen == want


def test_record_covers_every_family_and_switch(record):
    """The condition on the case list: every launching family in every pass where it exists, every switch in both positions."""
    by_id = {e["case"]["id"]: e for e in record["cases"]}
    entries = lambda i: [c[0] for c in by_id[i]["seen"]["calls"]]
    ops = {}
    for e in record["cases"]:
        for name, _ in e["seen"]["calls"]:
            ops.setdefault(name, set()).add(e["case"]["op"])
    assert {"fwd", "bias_fwd"} <= ops["mi_conv_fwd_f32"] and "dgrad" in ops["mi_conv_dgrad_f32"] and "wgrad" in ops["mi_conv_wgrad_f32"]
    assert {"fwd", "dgrad"} <= ops["mi_conv3d_cube2_f32"] and {"fwd", "dgrad"} <= ops["mi_conv3d_direct_f32"]
    assert {"fwd", "dgrad"} <= ops["mi_conv2d_p2d_f32"] and "wgrad" in ops["mi_conv2d_p2d_wgrad_f32"]
    assert "fwd" in ops["mi_conv2d_stem3_fwd_f32"] and "wgrad" in ops["mi_conv2d_stem3_wgrad_f32"]
    assert "bias_fwd" in ops["mi_stem2d_fwd_bias_f32"]
    for name in ("mi_conv3d_s2_fwd_f32", "mi_conv3d_s2_fwd_img_f32", "mi_conv3d_s2_dgrad_f32", "mi_conv3d_s2_dgrad_img_f32",
                 "mi_conv_d32_fwd_pool_strided_f32", "mi_conv_d32_upconv_fwd_f32", "mi_upconv_tail_fwd", "mi_splitk_reduce_batch"):
        assert name in ops, name
    for name in ("mi_conv_d32_fwd_f32", "mi_conv_d64_fwd_f32", "mi_conv_d32_1x1_fwd_f32", "mi_smallk_fwd_f32"):
        assert {"fwd", "bias_fwd"} <= ops[name], name
    kinds = {c[1][-1] for e in record["cases"] for c in e["seen"]["calls"] if c[0] == "mi_conv_d32_fwd_f32"}
    taps = {c[1][4] for e in record["cases"] for c in e["seen"]["calls"] if c[0] == "mi_smallk_fwd_f32"}
    assert kinds == {1, 2} and taps == {1, 3}
    assert by_id["s2_fwd_declined"]["seen"] == dict(by_id["s2_fwd_declined"]["seen"], calls=[], returns=None)
    assert by_id["s2_dgrad_declined"]["seen"]["calls"] == [] and by_id["s2_dgrad_declined"]["seen"]["returns"] is None
    kernels = {e["seen"]["last_kernel"] for e in record["cases"]}
    for prefix in ("stem_fwd", "direct3", "direct3s", "cube2", "implicit GEMM", "direct3_wgrad", "pair_wgrad"):
        assert any(k.startswith(prefix) for k in kernels), prefix
    # every switch moves its case off the family the case takes without it
    for on, off in (("cube2_fwd", "cube2_fwd_reduce"), ("cube2_fwd", "cube2_fwd_f32"), ("cube2_dgrad", "cube2_dgrad_reduce"),
                    ("cube2_dgrad", "cube2_dgrad_f32"), ("direct_fwd", "direct_fwd_profile"), ("direct_fwd", "direct_fwd_idle"),
                    ("direct_dgrad", "direct_dgrad_profile"), ("direct_dgrad", "direct_dgrad_idle"), ("direct_fwd", "direct_fwd_f32"),
                    ("stem3_fwd", "stem3_fwd_off"), ("stem3_wgrad", "stem3_wgrad_off"), ("stem3_fwd", "stem3_fwd_co48"),
                    ("stem3_wgrad", "stem3_wgrad_co48"), ("p2d_fwd", "p2d_off_fwd"), ("p2d_dgrad", "p2d_off_dgrad"),
                    ("p2d_wgrad", "p2d_off_wgrad"), ("p2d_wgrad", "p2d_wgrad_switch"), ("p2d_fwd", "p2d_f32_fwd"),
                    ("p2d_dgrad", "p2d_f32_dgrad"), ("p2d_wgrad", "p2d_f32_wgrad"), ("stem2d", "stem2d_off"),
                    ("smallk1_fwd", "smallk1_fwd_nosmallk"), ("smallk3_bias_fwd", "smallk3_bias_fwd_nosmallk"),
                    ("kind1_pool_fused", "kind1_pool_unfused"), ("kind3_pool_fused_slice", "kind3_pool_unfused_slice"),
                    ("kind1_fwd", "kind1_fwd_inference_res"), ("kind4_fwd", "kind4_fwd_inference_res"), ("kind1_fwd", "kind1_fwd_f32"),
                    ("conv_bn_folded", "conv_bn_unfolded"), ("upconv_fused", "upconv_tail"), ("s2_fwd", "s2_fwd_image"),
                    ("s2_fwd_image", "s2_fwd_image_profile")):
        assert entries(on) != entries(off), (on, off)
    assert by_id["skip_ok"]["seen"]["returns"] is True and by_id["skip_ok_64"]["seen"]["returns"] is True
    for i in ("skip_no_width", "skip_no_channels", "skip_no_f32", "skip_no_pool_unfused"):
        assert by_id[i]["seen"]["returns"] is False, i
    assert sum(1 for e in record["cases"] if e["seen"].get("profile")) >= 6
