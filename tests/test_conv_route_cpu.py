"""hipops.conv_route without a GPU: for every convolution case of tests/golden/conv_routes.json (recorded on the GPU by
tests/test_conv_route_gpu.py) the route computed from the case's integers and flags names the entry the recorded call launched.
A pull request that means to move a route edits the record and, for a new family, the table below."""
import itertools
import json
import os

import pytest
import torch

from conftest import GOLDEN

# (family, pass, parameter) -> the compute entry of include/cetpick_hip.h the route launches; pass "pool": forward with the pooled output
ENTRY = {
    ("d32", "fwd", 1): "mi_conv_d32_fwd_f32", ("d32", "fwd", 2): "mi_conv_d32_fwd_f32", ("d32", "fwd", 3): "mi_conv_d64_fwd_f32",
    ("d32", "fwd", 4): "mi_conv_d32_1x1_fwd_f32",
    ("d32", "pool", 1): "mi_conv_d32_fwd_pool_strided_f32", ("d32", "pool", 3): "mi_conv_d32_fwd_pool_strided_f32",
    ("smallk", "fwd", 1): "mi_smallk_fwd_f32", ("smallk", "fwd", 3): "mi_smallk_fwd_f32",
    ("stem3", "fwd", 0): "mi_conv2d_stem3_fwd_f32", ("stem3", "wgrad", 0): "mi_conv2d_stem3_wgrad_f32",
    ("stem2d", "fwd", 0): "mi_stem2d_fwd_bias_f32",
    ("p2d", "fwd", 0): "mi_conv2d_p2d_f32", ("p2d", "fwd", 1): "mi_conv2d_p2d_f32",
    ("p2d", "dgrad", 0): "mi_conv2d_p2d_f32", ("p2d", "dgrad", 1): "mi_conv2d_p2d_f32", ("p2d", "wgrad", 0): "mi_conv2d_p2d_wgrad_f32",
    ("direct", "fwd", 0): "mi_conv3d_direct_f32", ("direct", "dgrad", 0): "mi_conv3d_direct_f32",
    ("cube2", "fwd", 0): "mi_conv3d_cube2_f32", ("cube2", "dgrad", 0): "mi_conv3d_cube2_f32",
    ("s2", "fwd", 0): "mi_conv3d_s2_fwd_f32", ("s2", "fwd", 1): "mi_conv3d_s2_fwd_img_f32",
    ("s2", "dgrad", 0): "mi_conv3d_s2_dgrad_f32", ("s2", "dgrad", 1): "mi_conv3d_s2_dgrad_img_f32",
    ("generic", "fwd", 0): "mi_conv_fwd_f32", ("generic", "dgrad", 0): "mi_conv_dgrad_f32",
    ("generic", "wgrad", 0): "mi_conv_wgrad_f32", ("generic", "wgrad", 1): "mi_conv_wgrad_f32",
}
PASS = {"fwd": "fwd", "bias_fwd": "fwd", "dgrad": "dgrad", "wgrad": "wgrad", "s2_fwd": "fwd", "s2_dgrad": "dgrad"}

with open(os.path.join(GOLDEN, "conv_routes.json")) as _f:
    RECORD = [e for e in json.load(_f)["cases"] if e["case"]["op"] in PASS]


@pytest.fixture(scope="module")
def H():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import hipops
    return hipops


def route_of(H, case, monkeypatch):
    shape = tuple(case["shape"])
    nd5, op = len(shape) == 5, case["op"]
    for name, value in (case.get("attrs") or {}).items():
        monkeypatch.setattr(H, name, value)
    for name in ("MI_CONV_ARITH", "MI_CUBE2_REDUCE", "MI_NO_P2D", "MI_NO_P2D_WGRAD", "MI_NO_STEM2D", "MI_NO_D32"):
        monkeypatch.delenv(name, raising=False)
    for name, value in (case.get("env") or {}).items():
        monkeypatch.setenv(name, value)
    image = None
    if case.get("images") == "active":
        image = "s2" if op.startswith("s2") else "direct" if nd5 else "p2d"
    dil = case.get("dil")
    return H.conv_route(PASS[op], shape, shape[-1], case["co"], H._k3(case["k"], nd5), case["stride"], H._p3(case["pad"], nd5),
                        H._k3(dil, nd5) if dil is not None else None, inference=bool(case.get("inference")) or op == "bias_fwd",
                        has_res=bool(case.get("res")), has_bias=op == "bias_fwd", relu=bool(case.get("relu")), pool=bool(case.get("pool")),
                        image=image, profile=bool(case.get("profile")), shortcut=op.startswith("s2"),
                        accumulates=bool(case.get("acc")), deferred=bool(case.get("deferred")))


@pytest.mark.parametrize("entry", RECORD, ids=[e["case"]["id"] for e in RECORD])
def test_route_names_the_recorded_entry(entry, H, monkeypatch):
    case, seen = entry["case"], entry["seen"]
    def no_tensor(*a, **k):
        raise AssertionError("conv_route made a tensor")
    with monkeypatch.context() as mp:
        for name in ("empty", "zeros", "ones", "tensor", "empty_like", "as_tensor", "full"):
            mp.setattr(torch, name, no_tensor)
        route = route_of(H, case, mp)
    assert route.family in H.ROUTE_FAMILIES and hash(route) == hash(H.Route(*route)) and {route: 1}[H.Route(*route)] == 1
    launched = [c for c in seen["calls"] if "_prep" not in c[0]]
    if route.family is None:
        assert launched == [] and seen["returns"] is None
        return
    name, scalars = launched[0]
    assert name == ENTRY[(route.family, "pool" if case.get("pool") else PASS[case["op"]], route.param)]
    if name == "mi_conv_d32_fwd_f32":
        assert scalars[-1] == route.param                # the kind
    if name == "mi_smallk_fwd_f32":
        assert scalars[4] == route.param                 # the taps


def test_slab_form_truth_table(H, monkeypatch):
    """The weight gradient's slab form (route.param of a "generic" wgrad route) over every combination of its inputs, against the
    condition as conv_wgrad_into stated it before the route function existed."""
    from cet_pick_amd import _lib as L
    lib = L.lib()
    shapes = [((4, 8, 8, 8, 64), 64, (3, 3, 3), 1, (1, 1, 1)),          # conv_direct3.hip's shape: usable == 1
              ((4, 4, 4, 4, 128), 128, (3, 3, 3), 1, (1, 1, 1)),        # usable == 2
              ((2, 6, 6, 6, 16), 32, (3, 3, 3), 1, (1, 1, 1)),          # not usable
              ((64, 32, 32, 32, 1), 64, (7, 7, 7), 2, (3, 3, 3)),       # more rows than SIDE_ROWS_MAX
              ((2, 6, 6, 6, 16), 32, (3, 1, 1), 1, (1, 0, 0))]          # no cube
    for (shape, co, k3, stride, p3), d3, acc, profile, deferred, side, batch in itertools.product(
            shapes, (None, (1, 1, 1), (1, 2, 2)), (False, True), (False, True), (False, True), (False, True), (False, True)):
        monkeypatch.setattr(H, "WGRAD_BATCH", batch)
        n, d, h, wd, ci = shape
        dd = d3 or (1, 1, 1)
        rows = n
        for v, k, p, dl in zip(shape[1:4], k3, p3, dd):
            rows *= (v + 2 * p - dl * (k - 1) - 1) // stride + 1
        slab_form = not acc and dd == (1, 1, 1) and (not profile or (deferred and side and rows <= H.SIDE_ROWS_MAX))
        want = bool(slab_form and (deferred or (batch and lib.mi_conv3d_direct_usable(n, d, h, wd, ci, co, k3[0], stride, p3[0]) in (1, 2)
                                                and k3[0] == k3[1] == k3[2] and p3[0] == p3[1] == p3[2])))
        route = H.conv_route("wgrad", shape, ci, co, k3, stride, p3, d3, accumulates=acc, profile=profile, deferred=deferred, side=side)
        assert route == H.Route("generic", int(want)), (shape, d3, acc, profile, deferred, side, batch)


def test_stem3_needs_a_width_that_divides_the_block(H, monkeypatch):
    """Conv2d(1, co, 3, padding 1): co = 16 takes stem3, co = 12 (256 % (12 // 4) != 0) falls to the generic entry, in both passes (the
    library's generic entry wants co % 16 == 0, so the GPU record holds co = 48 for this rule)."""
    monkeypatch.delenv("MI_NO_P2D", raising=False)
    for pass_ in ("fwd", "wgrad"):
        assert H.conv_route(pass_, (2, 12, 20, 1), 1, 16, (1, 3, 3), 1, (0, 1, 1)).family == "stem3"
        assert H.conv_route(pass_, (2, 12, 20, 1), 1, 12, (1, 3, 3), 1, (0, 1, 1)) == H.Route("generic", 0)
