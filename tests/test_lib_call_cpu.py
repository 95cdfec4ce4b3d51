"""_lib.call against a stub library: what reaches an entry, what is refused before it, how a status comes back (CPU only)."""
import ctypes

import pytest
import torch

from cet_pick_amd import _lib as L

# an entry with a stream parameter (pointers, floats, a long), one with a struct pointer in it, one without a stream
STREAMED, GEOM, PLAIN = "mi_sgd_step", "mi_conv_fwd_f32", "mi_graph_node_counts"
STREAM = ctypes.c_void_p(0x5712)


class StubLib:
    """Stands in for the ctypes library object: every mi_* attribute records its arguments and returns `status`."""

    def __init__(self, status=0):
        self.status, self.calls = status, []

    def __getattr__(self, name):
        if not name.startswith("mi_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry


@pytest.fixture
def stub(monkeypatch):
    s = StubLib()
    monkeypatch.setattr(L, "_lib", s)
    monkeypatch.setattr(L, "stream", lambda: STREAM)
    return s


def test_the_entries_are_what_the_tests_take_them_for():
    P, F, I, Z = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_size_t
    assert L.SIGNATURES[STREAMED][1] == [P, P, P, F, F, F, ctypes.c_long, L._S]
    assert L.SIGNATURES[GEOM][1] == [P, P, P, P, I, I, ctypes.POINTER(L.ConvGeom), P, Z, L._S]
    assert L.SIGNATURES[PLAIN][1] == [P, P]


def test_host_tensor_is_refused_before_the_library(stub):
    with pytest.raises(L.HipExtensionError, match=r"%s: argument 1 is a tensor on cpu" % STREAMED):
        L.call(STREAMED, None, torch.zeros(3), None, 0.1, 0.0, 1.0, 3)
    assert stub.calls == []


def test_arguments_arrive_unchanged_and_none_stays_none(stub):
    geom, addr = ctypes.byref(L.ConvGeom()), ctypes.c_void_p(64)
    assert L.call(GEOM, None, addr, 1 << 40, None, 3, 1, geom, None, 4096) is True
    assert L.call(STREAMED, None, None, None, 2.5, 0.0, 1.0, 7) is True
    (name, args), (_, args2) = stub.calls
    assert name == GEOM and len(args) == 10 and args[0] is None and args[3] is None and args[7] is None
    assert args[1] is addr and args[2] == 1 << 40 and type(args[2]) is int and args[6] is geom
    assert (args[4], args[5], args[8]) == (3, 1, 4096) and all(type(a) is int for a in (args[4], args[5], args[8]))
    assert args2[3] == 2.5 and type(args2[3]) is float and args2[6] == 7


def test_stream_is_appended_only_where_the_entry_takes_one(stub):
    L.call(STREAMED, None, None, None, 0.1, 0.0, 1.0, 3)
    L.call(PLAIN, None, None)
    assert stub.calls[0] == (STREAMED, (None, None, None, 0.1, 0.0, 1.0, 3, STREAM)) and stub.calls[0][1][-1] is STREAM
    assert stub.calls[1] == (PLAIN, (None, None))


@pytest.mark.parametrize("status, kind", [(-1, "bad argument"), (-2, "workspace too small"), (-3, "unsupported"), (700, "hipError 700")])
def test_status_raises_with_the_entry_name(stub, status, kind):
    stub.status = status
    with pytest.raises(L.HipExtensionError, match=r"^%s failed: %s$" % (PLAIN, kind)):
        L.call(PLAIN, None, None)
    assert len(stub.calls) == 1


def test_may_decline_turns_unsupported_alone_into_false(stub):
    stub.status = -3
    assert L.call(PLAIN, None, None, may_decline=True) is False
    stub.status = -1
    with pytest.raises(L.HipExtensionError, match=r"^%s failed: bad argument$" % PLAIN):
        L.call(PLAIN, None, None, may_decline=True)


def test_unknown_entry_and_missing_arguments_raise(stub):
    with pytest.raises(L.HipExtensionError, match="mi_no_such_entry"):
        L.call("mi_no_such_entry", 1)
    with pytest.raises(L.HipExtensionError, match=r"%s takes 2 arguments, got 1" % PLAIN):
        L.call(PLAIN, None)
    assert stub.calls == []
