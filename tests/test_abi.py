"""The C-ABI library loads and exports every symbol include/cetpick_hip.h declares (CPU only:
no compute calls)."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "cetpick_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", txt)))


def _header_geom_fields():
    """field names of `mi_conv_geom`, in the header's order (every one an int)"""
    txt = open(os.path.join(REPO, "include", "cetpick_hip.h")).read()
    body = re.search(r"typedef struct mi_conv_geom \{(.*?)\} mi_conv_geom;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        assert decl.startswith("int "), decl
        fields += [f.strip() for f in decl[4:].split(",")]
    return fields


def _header_prototypes():
    """[(return type, name, [parameter declarations])] of every `mi_*` prototype of the header, comments removed"""
    txt = open(os.path.join(REPO, "include", "cetpick_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    protos = re.findall(r"([A-Za-z_][\w \*]*?)\b(mi_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)
    return [(" ".join(ret.split()).replace(" *", "*"), name, [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in protos]


def _param_class(decl, L):
    """The class of one C parameter declaration: a POINTER(...) type for a pointer to a struct _lib mirrors, "ptr" for every other
    pointer, "stream" for mi_stream_t, else "int" | "i64" | "u64" | "float" | "double"."""
    import ctypes
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        mirrored = {"mi_conv_geom": L.ConvGeom, "mi_aug2d3d_ranges": L.Aug2d3dRanges, "mi_aug3d_ranges": L.Aug3dRanges,
                    "mi_plot_layout": L.PlotLayout}
        return ctypes.POINTER(mirrored[words[0]]) if words[0] in mirrored else "ptr"
    assert len(words) == 2, "a scalar parameter is `type name`: %r" % decl
    return {"mi_stream_t": "stream", "int": "int", "long": "i64", "int64_t": "i64", "size_t": "u64", "uint64_t": "u64",
            "float": "float", "double": "double"}[words[0]]


def _ctypes_class(t, L):
    import ctypes
    if t is L._S:
        return "stream"
    if t is ctypes.c_void_p:
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_long: "i64", ctypes.c_int64: "i64", ctypes.c_size_t: "u64", ctypes.c_uint64: "u64",
            ctypes.c_float: "float", ctypes.c_double: "double"}.get(t, t)          # (a POINTER(...) type stands for itself)


def test_signatures_match_the_header_prototypes():
    """Every prototype of the header against _lib.SIGNATURES: the number of parameters, the class of each, the return type, and the
    stream marker exactly where the last parameter is mi_stream_t (it is never anywhere else)."""
    import ctypes
    from cet_pick_amd import _lib as L
    protos = _header_prototypes()
    assert len(protos) == len(L.SIGNATURES) == len(_header_symbols()) == len({name for _, name, _ in protos})
    returns = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
    for ret, name, params in protos:
        res, args = L.SIGNATURES[name]
        assert res is returns[ret], name
        want = [_param_class(p, L) for p in params]
        assert [_ctypes_class(t, L) for t in args] == want, (name, params)
        assert "stream" not in want[:-1], name
        streamed, pointers = L._ENTRIES[name]
        assert streamed == (want[-1:] == ["stream"]), name
        assert list(pointers) == [i for i, c in enumerate(want) if c == "ptr"], name          # where call() takes a tensor
    assert sum(s for s, _ in L._ENTRIES.values()) == sum(1 for _, _, params in protos if params and params[-1].startswith("mi_stream_t"))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    L = _lib.lib()
    syms = _header_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(L, s), "missing export " + s
    assert set(syms) == set(_lib.SIGNATURES), (set(syms) ^ set(_lib.SIGNATURES))
    assert L.mi_abi_version() == 4
    assert L.mi_build_arch() == b"gfx950"


def test_conv_geom_struct_matches_header():
    import ctypes
    from cet_pick_amd import _lib
    fields = _header_geom_fields()
    assert len(fields) == 16
    assert [f for f, _ in _lib.ConvGeom._fields_] == fields
    assert all(t is ctypes.c_int for _, t in _lib.ConvGeom._fields_)
    assert ctypes.sizeof(_lib.ConvGeom) == 16 * 4


def test_conv_workspace_bytes_refuses_bad_geometries():
    """mi_conv_workspace_bytes needs no device: 0 for a geometry the convolution entries refuse, a size otherwise."""
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    size = _lib.lib().mi_conv_workspace_bytes
    #                      N  D  H   W   Ci  Co  window   s  padding  dilation
    assert size(_lib.ConvGeom(1, 6, 20, 24, 32, 32, 3, 3, 3, 2, 1, 4, 4, 1, 4, 4)) == 0        # dilated and stride 2
    assert size(_lib.ConvGeom(1, 8, 8, 8, 8, 16, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1)) == 0           # Ci = 8
    assert size(_lib.ConvGeom(1, 6, 20, 24, 32, 32, 3, 3, 3, 1, 1, 4, 4, 1, 4, 4)) > 0
    assert size(_lib.ConvGeom(64, 8, 8, 8, 64, 64, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1)) > 0


def test_product_path_has_no_cpu_fallback():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cet_pick_amd import _lib
    from cet_pick_amd.utils import image as Im
    with pytest.raises(_lib.HipExtensionError):
        Im.get_potential_coords_pyramid(np.zeros((30, 80, 80), np.float32), sigmas=[2, 4])


def test_product_does_not_import_oracle():
    pkg = os.path.join(REPO, "cet_pick_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
