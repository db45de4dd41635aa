"""Group device re-solve of many small LPs, the parts that need no GPU (include/hprlp_amd.h: hprlp_solver_set_data_many_device,
hprlp_solver_resolve_many_device, hprlp_solver_set_matrix_values_many_device, hprlp_last_many_device_counts; DESIGN.md "Many small
LPs", group device re-solve): the entry points exist with the header's signatures, hprlp_member_out mirrors the header, the Python
methods exist, the refusals that need no handle return -1 with a message that names the entry point and the cause, the counts
refuse NULL and are zero on a fresh thread, and the table builder's self-test passes with the check stage of the device entries."""
import ctypes as C
import threading

import pytest

from conftest import hprlp
from test_resolve import header_prototypes

SET_DATA = "hprlp_solver_set_data_many_device"
RESOLVE = "hprlp_solver_resolve_many_device"
SET_MATRIX = "hprlp_solver_set_matrix_values_many_device"
COUNTS = "hprlp_last_many_device_counts"
CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "void *": C.c_void_p, "long *": C.POINTER(C.c_long),
            "const hprlp_member_data *": C.POINTER(hprlp.CMemberData), "const hprlp_member_start *": C.POINTER(hprlp.CMemberStart),
            "const hprlp_member_values *": C.POINTER(hprlp.CMemberValues), "HPRLP_results *": C.POINTER(hprlp.CResults)}
WANT = {SET_DATA: ["hprlp_solver * *", "int", "const hprlp_member_data *", "void *"],
        RESOLVE: ["hprlp_solver * *", "int", "const hprlp_member_start *", "const hprlp_member_out *", "void *", "HPRLP_results *"],
        SET_MATRIX: ["hprlp_solver * *", "int", "const hprlp_member_values *", "void *"],
        COUNTS: ["long *"]}


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    ctype_of = dict(CTYPE_OF, **{"const hprlp_member_out *": C.POINTER(hprlp.CMemberOut)})
    assert list(fn.argtypes) == [ctype_of[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_member_out_has_the_headers_layout():
    """typedef struct hprlp_member_out { double *x, *y, *z; }: three pointers in that order, no padding."""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "hprlp_amd.h")).read()
    mm = re.search(r"typedef struct hprlp_member_out \{([^}]*)\} hprlp_member_out;", text)
    assert mm and re.sub(r"\s+", " ", mm.group(1)).strip() == "double *x, *y, *z;", mm and mm.group(1)
    assert [f for f, _ in hprlp.CMemberOut._fields_] == ["x", "y", "z"]
    assert [getattr(hprlp.CMemberOut, f).offset for f in ("x", "y", "z")] == [0, C.sizeof(C.c_void_p), 2 * C.sizeof(C.c_void_p)]
    assert C.sizeof(hprlp.CMemberOut) == 3 * C.sizeof(C.c_void_p)


def test_python_has_the_group_methods_and_the_named_counts():
    for name in ("set_data_many_tensors", "resolve_many_tensors", "set_matrix_many_tensors"):
        assert callable(getattr(hprlp.Solver, name)), name
    assert callable(hprlp.last_many_device_counts)
    assert len(hprlp.MANY_DEVICE_KEYS) == 7 and set(hprlp.last_many_device_counts()) == set(hprlp.MANY_DEVICE_KEYS)


def test_counts_refuse_null_and_are_zero_on_a_fresh_thread():
    assert hprlp.lib().hprlp_last_many_device_counts(None) == -1
    got = {}

    def run():
        got["counts"] = hprlp.last_many_device_counts()
        raw = (C.c_long * 8)(*([7] * 8))
        assert hprlp.lib().hprlp_last_many_device_counts(raw) == 0
        got["raw"] = list(raw)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert got["counts"] and all(v == 0 for v in got["counts"].values()), got
    assert got["raw"] == [0] * 8, got   # (the eighth slot is written too)


def test_refusals_that_need_no_handle():
    L = hprlp.lib()
    data, values = (hprlp.CMemberData * 2)(), (hprlp.CMemberValues * 2)()
    start, dst, res = (hprlp.CMemberStart * 2)(), (hprlp.CMemberOut * 2)(), (hprlp.CResults * 2)()
    none = (C.c_void_p * 2)()   # two NULL members
    cases = [(SET_DATA, lambda: L.hprlp_solver_set_data_many_device(None, 2, data, None), "null solver list"),
             (SET_DATA, lambda: L.hprlp_solver_set_data_many_device(none, 0, data, None), "count must be positive"),
             (SET_DATA, lambda: L.hprlp_solver_set_data_many_device(none, -1, data, None), "count must be positive"),
             (SET_DATA, lambda: L.hprlp_solver_set_data_many_device(none, 2, None, None), "null data"),
             (SET_DATA, lambda: L.hprlp_solver_set_data_many_device(none, 2, data, None), "member 0 is null"),
             (RESOLVE, lambda: L.hprlp_solver_resolve_many_device(None, 2, start, dst, None, res), "null solver list"),
             (RESOLVE, lambda: L.hprlp_solver_resolve_many_device(none, 0, start, dst, None, res), "count must be positive"),
             (RESOLVE, lambda: L.hprlp_solver_resolve_many_device(none, 2, start, dst, None, None), "null results"),
             (RESOLVE, lambda: L.hprlp_solver_resolve_many_device(none, 2, None, None, None, res), "member 0 is null"),
             (SET_MATRIX, lambda: L.hprlp_solver_set_matrix_values_many_device(None, 2, values, None), "null solver list"),
             (SET_MATRIX, lambda: L.hprlp_solver_set_matrix_values_many_device(none, 0, values, None), "count must be positive"),
             (SET_MATRIX, lambda: L.hprlp_solver_set_matrix_values_many_device(none, 2, None, None), "null data"),
             (SET_MATRIX, lambda: L.hprlp_solver_set_matrix_values_many_device(none, 2, values, None), "member 0 is null")]
    for entry, call, cause in cases:
        assert call() == -1, (entry, cause)
        msg = hprlp.last_error()
        assert msg.startswith(entry + ":") and cause in msg, (entry, cause, msg)
        assert all(v == 0 for v in hprlp.last_many_device_counts().values())
    assert all(v == 0 for v in hprlp.last_resolve_many_counts().values())
    assert all(v == 0 for v in hprlp.last_values_many_counts().values())


def test_python_raises_value_error_before_the_library_is_called():
    class Stub:
        """What the checks of the Python methods read of a solver; no handle is ever reached."""
        h = None
        _tensor = hprlp.Solver._tensor

        class model:
            m, n = 3, 4

    two = [Stub(), Stub()]
    with pytest.raises(ValueError, match="one dict"):
        hprlp.Solver.set_data_many_tensors(two, [None])
    with pytest.raises(ValueError, match="unknown keys"):
        hprlp.Solver.set_data_many_tensors(two, [{"b": None}, None])
    with pytest.raises(ValueError, match="one dict"):
        hprlp.Solver.set_matrix_many_tensors(two, [None])
    with pytest.raises(ValueError, match="unknown keys"):
        hprlp.Solver.set_matrix_many_tensors(two, [None, {"vals": None}])
    with pytest.raises(ValueError, match="one entry"):
        hprlp.Solver.resolve_many_tensors(two, x=[None])


def test_group_table_selftest_with_the_device_check_stage():
    """csrc/group_table.cpp lists the numbered checks; 11 is the check stage of the device entries."""
    assert hprlp.lib().hprlp_group_table_selftest() == 0
