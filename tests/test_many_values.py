"""Group matrix values of many small LPs, the parts that need no GPU (include/hprlp_amd.h: hprlp_solver_set_matrix_values_many,
hprlp_last_values_many_counts; csrc/group_pack.cpp: the packing layout with matrix values in it; DESIGN.md "Many small LPs", group
matrix values): the entry points exist with the header's signatures, the struct mirrors the header, the refusals that need no
device return -1 with a message that names the entry point and the cause, and without a GPU the call fails loudly."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import hprlp
from test_resolve import header_prototypes

ENTRY = "hprlp_solver_set_matrix_values_many"
CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "const hprlp_member_values *": C.POINTER(hprlp.CMemberValues),
            "long *": C.POINTER(C.c_long)}
WANT = {ENTRY: ["hprlp_solver * *", "int", "const hprlp_member_values *"], "hprlp_last_values_many_counts": ["long *"]}


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_member_struct_has_the_headers_layout():
    """A pointer, a long, six pointers: the fields of the header in its order, no padding on an LP64 machine."""
    assert [f for f, _ in hprlp.CMemberValues._fields_] == ["val", "nnz", "c", "obj_constant", "AL", "AU", "l", "u"]
    assert hprlp.CMemberValues.nnz.offset == C.sizeof(C.c_void_p) and hprlp.CMemberValues.c.offset == C.sizeof(C.c_void_p) + C.sizeof(C.c_long)
    assert C.sizeof(hprlp.CMemberValues) == 7 * C.sizeof(C.c_void_p) + C.sizeof(C.c_long)


def test_python_has_the_group_method_and_the_named_counts():
    assert callable(hprlp.Solver.set_matrix_many) and callable(hprlp.last_values_many_counts)
    assert len(hprlp.VALUES_MANY_KEYS) == 8 and set(hprlp.last_values_many_counts()) == set(hprlp.VALUES_MANY_KEYS)


def test_counts_refuse_null_and_are_zero_on_a_fresh_thread():
    assert hprlp.lib().hprlp_last_values_many_counts(None) == -1
    got = {}

    def run():
        got["counts"] = hprlp.last_values_many_counts()

    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert got["counts"] and all(v == 0 for v in got["counts"].values()), got


def test_refusals_that_need_no_device():
    L = hprlp.lib()
    data = (hprlp.CMemberValues * 2)()
    none = (C.c_void_p * 2)()   # two NULL members
    cases = [(lambda: L.hprlp_solver_set_matrix_values_many(None, 2, data), "null solver list"),
             (lambda: L.hprlp_solver_set_matrix_values_many(none, 2, None), "null data"),
             (lambda: L.hprlp_solver_set_matrix_values_many(none, 0, data), "count must be positive"),
             (lambda: L.hprlp_solver_set_matrix_values_many(none, -3, data), "count must be positive"),
             (lambda: L.hprlp_solver_set_matrix_values_many(none, 2, data), "member 0 is null")]
    for call, cause in cases:
        assert call() == -1, cause
        msg = hprlp.last_error()
        assert ENTRY in msg and cause in msg, (cause, msg)
    assert all(v == 0 for v in hprlp.last_values_many_counts().values())


class _Stub:
    """What the length checks of the Python method read of a solver; no handle is ever reached."""
    h = None
    _data_vector = hprlp.Solver._data_vector

    class model:
        m, n = 3, 4


def test_python_raises_value_error_before_the_library_is_called():
    two = [_Stub(), _Stub()]
    with pytest.raises(ValueError, match="one dict"):
        hprlp.Solver.set_matrix_many(two, [None])
    with pytest.raises(ValueError, match="unknown keys"):
        hprlp.Solver.set_matrix_many(two, [{"b": np.zeros(3)}, None])
    with pytest.raises(ValueError, match="length 4"):
        hprlp.Solver.set_matrix_many(two, [None, {"c": np.zeros(3)}])


def test_packing_layout_selftest_with_the_values_checks():
    """csrc/group_pack.cpp lists the numbered checks; 8 is the matrix values' place in the data block."""
    assert hprlp.lib().hprlp_group_pack_selftest() == 0


def test_group_table_selftest():
    assert hprlp.lib().hprlp_group_table_selftest() == 0


def test_without_a_gpu_the_call_fails_loudly():
    """No device in sight (HIP_VISIBLE_DEVICES hides any there may be, in a child process so that this one's runtime is left
    alone): the solver cannot be created, let alone given values -- nothing returns 0."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    script = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import hprlp, lpgen
import ctypes as C
lp = lpgen.planted_lp(30, 50, 200, 1)
mod = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
L = hprlp.lib()
try:
    pair = [hprlp.Solver(mod, hprlp.Parameters(use_presolve=False)) for _ in range(2)]
    for s in pair:
        s.scale()
except Exception as e:
    print("NO-SOLVER", type(e).__name__)
    sys.exit(0)
d = dict(values=lp["values"], c=lp["c"], AL=lp["AL"], AU=lp["AU"], l=lp["l"], u=lp["u"])
try:
    hprlp.Solver.set_matrix_many(pair, [d, d])
except RuntimeError as e:
    print("REFUSED", e)
    sys.exit(0)
print("RETURNED-0")
''' % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert "RETURNED-0" not in r.stdout, (r.stdout, r.stderr[-800:])
    assert r.returncode != 0 or "NO-SOLVER" in r.stdout or "REFUSED" in r.stdout, (r.returncode, r.stdout, r.stderr[-800:])
