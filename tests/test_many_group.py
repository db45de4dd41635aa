"""Group launches for check step, evaluation and restart of many small LPs, the part that needs no GPU (include/hprlp_amd.h "many
small LPs", DESIGN.md "Many small LPs"): the three new entry points exist with the header's signatures, the Python methods exist,
and wrong arguments are refused with a message naming the entry point before any device work.  The refusals that need a live
handle are in tests/test_gpu_many_group.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import hprlp
from test_resolve import header_prototypes

WANT = {
    "hprlp_solver_residuals_many": ["hprlp_solver * *", "int", "const int *", "const int *", "double *"],
    "hprlp_solver_restart_many": ["hprlp_solver * *", "int", "const double *", "double *"],
    "hprlp_last_run_many_counts": ["long *"],
}
CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "const int *": hprlp.c_int_p, "double *": hprlp.c_dbl_p,
            "const double *": hprlp.c_dbl_p, "long *": C.POINTER(C.c_long)}


def test_the_three_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in WANT:
        assert s in names, s


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_have_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_python_has_the_group_methods():
    assert callable(hprlp.last_run_many_counts)
    for f in ("residuals_many", "restart_many"):
        assert callable(getattr(hprlp.Solver, f)), f


def test_counts_of_a_thread_that_ran_no_group_are_zero_and_null_is_refused():
    L = hprlp.lib()
    assert L.hprlp_last_run_many_counts(None) == -1
    c = hprlp.last_run_many_counts()
    assert set(c) == {"rounds", "waits", "group_launches", "copies", "own", "served"}
    assert all(isinstance(v, int) and v >= 0 for v in c.values())


def test_wrong_arguments_are_refused_with_a_message():
    """A NULL list, count <= 0, a NULL member, a NULL iter / compute_gap / in / out, a negative iter[k]: -1 and a message naming
    the entry point, with or without a GPU (nothing is launched: no handle exists that anything could be launched for)."""
    L = hprlp.lib()
    it, neg, cg = np.array([1, 1], np.int32), np.array([1, -2], np.int32), np.zeros(2, np.int32)
    out, six, sig = np.zeros(16), np.ones(12), np.zeros(2)
    hs = (C.c_void_p * 2)(None, None)
    I = lambda a: a.ctypes.data_as(hprlp.c_int_p)
    D = lambda a: a.ctypes.data_as(hprlp.c_dbl_p)
    res = "hprlp_solver_residuals_many"
    cases = [
        (res, lambda: L.hprlp_solver_residuals_many(None, 2, I(it), I(cg), D(out)), "null solver list"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 0, I(it), I(cg), D(out)), "count must be positive"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, -3, I(it), I(cg), D(out)), "count must be positive"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 2, I(it), I(cg), D(out)), "member 0 is null"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 2, None, I(cg), D(out)), "null iter"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 2, I(it), None, D(out)), "null compute_gap"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 2, I(it), I(cg), None), "null out"),
        (res, lambda: L.hprlp_solver_residuals_many(hs, 2, I(neg), I(cg), D(out)), "iter[1] is negative"),
    ]
    rst = "hprlp_solver_restart_many"
    cases += [
        (rst, lambda: L.hprlp_solver_restart_many(None, 2, D(six), D(sig)), "null solver list"),
        (rst, lambda: L.hprlp_solver_restart_many(hs, 0, D(six), D(sig)), "count must be positive"),
        (rst, lambda: L.hprlp_solver_restart_many(hs, 2, D(six), D(sig)), "member 0 is null"),
        (rst, lambda: L.hprlp_solver_restart_many(hs, 2, None, D(sig)), "null in"),
    ]
    for name, call, word in cases:
        assert call() == -1, (name, word)
        assert name in hprlp.last_error() and word in hprlp.last_error(), (name, word, hprlp.last_error())
    assert np.array_equal(out, np.zeros(16)) and np.array_equal(sig, np.zeros(2))
    with pytest.raises(ValueError):
        hprlp.Solver.residuals_many([], [1], [0])
    with pytest.raises(ValueError):
        hprlp.Solver.restart_many([], [[1.0] * 5])
