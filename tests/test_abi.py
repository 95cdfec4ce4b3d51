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
