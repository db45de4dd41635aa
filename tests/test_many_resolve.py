"""Group re-solve of many small LPs, the parts that need no GPU (include/hprlp_amd.h: hprlp_solver_set_data_many,
hprlp_solver_resolve_many, hprlp_last_resolve_many_counts; csrc/group_pack.cpp: the packing layout; DESIGN.md "Many small LPs",
group re-solve): the entry points exist with the header's signatures, the refusals that need no handle return -1 with a message
that names the entry point and the cause and leave the output alone, and the packing layout passes its self-test."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import hprlp
from test_resolve import header_prototypes

CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "const hprlp_member_data *": C.POINTER(hprlp.CMemberData),
            "const hprlp_member_start *": C.POINTER(hprlp.CMemberStart), "HPRLP_results *": C.POINTER(hprlp.CResults),
            "long *": C.POINTER(C.c_long)}
WANT = {
    "hprlp_solver_set_data_many": ["hprlp_solver * *", "int", "const hprlp_member_data *"],
    "hprlp_solver_resolve_many": ["hprlp_solver * *", "int", "const hprlp_member_start *", "HPRLP_results *"],
    "hprlp_last_resolve_many_counts": ["long *"],
}


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_member_structs_have_the_headers_layout():
    """Six pointers; two pointers and a double: the fields of the header in its order."""
    assert [f for f, _ in hprlp.CMemberData._fields_] == ["c", "obj_constant", "AL", "AU", "l", "u"]
    assert [f for f, _ in hprlp.CMemberStart._fields_] == ["x0", "y0", "sigma"]
    assert C.sizeof(hprlp.CMemberData) == 6 * C.sizeof(C.c_void_p) and C.sizeof(hprlp.CMemberStart) == 2 * C.sizeof(C.c_void_p) + 8


def test_python_has_the_group_methods():
    for f in ("set_data_many", "resolve_many"):
        assert callable(getattr(hprlp.Solver, f)), f
    assert callable(hprlp.last_resolve_many_counts)
    assert len(hprlp.RESOLVE_MANY_KEYS) == 8 and set(hprlp.last_resolve_many_counts()) == set(hprlp.RESOLVE_MANY_KEYS)


def test_counts_refuse_null_and_are_zero_on_a_fresh_thread():
    L = hprlp.lib()
    assert L.hprlp_last_resolve_many_counts(None) == -1
    got = {}

    def run():
        got["counts"] = hprlp.last_resolve_many_counts()

    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert got["counts"] and all(v == 0 for v in got["counts"].values()), got


def test_refusals_that_need_no_handle():
    """-1, the entry point and the cause in the message; the results array keeps its bytes."""
    L = hprlp.lib()
    data = (hprlp.CMemberData * 2)()
    start = (hprlp.CMemberStart * 2)()
    res = (hprlp.CResults * 2)()
    C.memset(res, 0x5A, C.sizeof(res))
    before = bytes(res)
    none = (C.c_void_p * 2)()   # two NULL members
    cases = [
        (lambda: L.hprlp_solver_set_data_many(None, 2, data), "hprlp_solver_set_data_many", "null solver list"),
        (lambda: L.hprlp_solver_resolve_many(None, 2, start, res), "hprlp_solver_resolve_many", "null solver list"),
        (lambda: L.hprlp_solver_set_data_many(none, 0, data), "hprlp_solver_set_data_many", "count must be positive"),
        (lambda: L.hprlp_solver_set_data_many(none, -3, data), "hprlp_solver_set_data_many", "count must be positive"),
        (lambda: L.hprlp_solver_resolve_many(none, 0, start, res), "hprlp_solver_resolve_many", "count must be positive"),
        (lambda: L.hprlp_solver_resolve_many(none, -3, start, res), "hprlp_solver_resolve_many", "count must be positive"),
        (lambda: L.hprlp_solver_set_data_many(none, 2, data), "hprlp_solver_set_data_many", "member 0 is null"),
        (lambda: L.hprlp_solver_resolve_many(none, 2, start, res), "hprlp_solver_resolve_many", "member 0 is null"),
        (lambda: L.hprlp_solver_resolve_many(none, 2, None, res), "hprlp_solver_resolve_many", "member 0 is null"),
        (lambda: L.hprlp_solver_set_data_many(none, 2, None), "hprlp_solver_set_data_many", "null data"),
        (lambda: L.hprlp_solver_resolve_many(none, 2, start, None), "hprlp_solver_resolve_many", "null results"),
    ]
    for call, entry, cause in cases:
        assert call() == -1, (entry, cause)
        msg = hprlp.last_error()
        assert entry in msg and cause in msg, (entry, cause, msg)
        assert bytes(res) == before, (entry, cause)
    assert all(v == 0 for v in hprlp.last_resolve_many_counts().values())


class _Stub:
    """What the length checks of the Python methods read of a solver; no handle is ever reached."""
    h = None

    class model:
        m, n = 3, 4


def test_python_raises_value_error_on_length_mismatches():
    two = [_Stub(), _Stub()]
    with pytest.raises(ValueError, match="one dict"):
        hprlp.Solver.set_data_many(two, [{}])
    with pytest.raises(ValueError, match="unknown keys"):
        hprlp.Solver.set_data_many(two, [{"b": np.zeros(3)}, None])
    for name in ("x", "y", "sigma"):
        with pytest.raises(ValueError, match=name):
            hprlp.Solver.resolve_many(two, **{name: [None]})


def test_packing_layout_selftest():
    """Ranges disjoint and inside their block, absent vectors take no room, a pack / unpack round trip on host memory returns
    what went in (csrc/group_pack.cpp lists the numbered checks)."""
    assert hprlp.lib().hprlp_group_pack_selftest() == 0


def test_group_table_selftest():
    """The host side of a group recording: table and map offsets aligned and disjoint, the {task, lb} map of grids {3, 0, 2}, a
    one-task kind with and without the own-launch rule, repeat_last(2, 20), the launch list against recorded_launches(), an empty
    trailing stage (csrc/group_table.cpp lists the numbered checks)."""
    assert hprlp.lib().hprlp_group_table_selftest() == 0
