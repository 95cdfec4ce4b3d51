"""The size limit of the pick grouping (csrc/pick_groups.hip) is answered without a device: by the workspace query of the library
and by the Python wrappers, before any tensor has to be on the GPU."""
import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from cet_pick_amd import _lib
    return _lib


def test_workspace_bytes_knows_the_limit():
    size = _lib().lib().mi_pick_workspace_bytes
    assert size(4096) > 0
    assert size(4096) >= 4096 * 64 * 8           # the adjacency bit matrix
    assert size(1) > 0 and size(0) > 0
    assert size(4097) == 0
    assert size(-1) == 0


def test_wrappers_refuse_4097_points_without_a_device():
    L = _lib()
    from cet_pick_amd import hipops
    pts = torch.zeros(4097, 3, dtype=torch.float64)           # on the host: the limit is checked first
    with pytest.raises(L.HipExtensionError, match="more than 4096 points"):
        hipops.pick_components(pts, 15)
    lab = torch.zeros(4097, dtype=torch.int32)
    with pytest.raises(L.HipExtensionError, match="more than 4096 points"):
        hipops.pick_fiber_fit(pts, lab, lab, 30, 0.03, 2, 0)


def test_post_process_device_forms_refuse_4097_points_without_a_device():
    L = _lib()
    from cet_pick_amd.utils import post_process as PP
    dets = [[i, 0, 0, 0.5] for i in range(4097)]
    with pytest.raises(L.HipExtensionError, match="more than 4096 points"):
        PP.tomo_group_postprocess_device(dets, device="cpu")
    with pytest.raises(L.HipExtensionError, match="more than 4096 points"):
        PP.tomo_fiber_postprocess_device([d[:3] for d in dets], device="cpu")


def test_empty_inputs_need_no_device():
    from cet_pick_amd.utils import post_process as PP
    assert PP.tomo_group_postprocess_device([]) == []
    assert PP.tomo_fiber_postprocess_device([]) == []
