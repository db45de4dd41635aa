"""Many small LPs at once, the part that needs no GPU (include/hprlp_amd.h "many small LPs", DESIGN.md "Many small LPs"): the four
entry points exist with the header's signatures, wrong arguments are refused with a message before any device work, and
hprlp_solve_many on a host without a GPU fails loudly member by member.  The refusals that need a live handle (the same handle
twice, a sharded solver, a solver never scaled, a negative count) are in tests/test_gpu_many.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_resolve import header_prototypes

SYMBOLS = ("hprlp_solver_power_iteration_many", "hprlp_solver_iterate_many", "hprlp_solver_run_many", "hprlp_solve_many")
WANT = {
    "hprlp_solver_power_iteration_many": ["hprlp_solver * *", "int", "int", "double", "double *", "int *"],
    "hprlp_solver_iterate_many": ["hprlp_solver * *", "int", "const int *", "int"],
    "hprlp_solver_run_many": ["hprlp_solver * *", "int", "HPRLP_results *"],
    "hprlp_solve_many": ["const LP_info_cpu *const *", "int", "const HPRLP_parameters *", "HPRLP_results *"],
}
CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "double": C.c_double, "double *": hprlp.c_dbl_p,
            "int *": hprlp.c_int_p, "const int *": hprlp.c_int_p, "HPRLP_results *": C.POINTER(hprlp.CResults),
            "const LP_info_cpu *const *": C.POINTER(C.POINTER(hprlp.CLPInfo)), "const HPRLP_parameters *": C.POINTER(hprlp.CParameters)}


def test_the_four_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s


@pytest.mark.parametrize("name", SYMBOLS)
def test_entry_points_have_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_python_has_the_group_methods():
    assert callable(hprlp.solve_many)
    for f in ("power_iteration_many", "iterate_many", "run_many"):
        assert callable(getattr(hprlp.Solver, f)), f


def test_wrong_arguments_are_refused_with_a_message():
    """A NULL list, count <= 0 and a NULL member: -1 and a message naming the entry point, with or without a GPU (nothing is
    launched: no handle exists that anything could be launched for)."""
    L = hprlp.lib()
    lam, its, cnt = np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int32)
    res = (hprlp.CResults * 2)()
    hs = (C.c_void_p * 2)(None, None)
    P, I = lam.ctypes.data_as(hprlp.c_dbl_p), its.ctypes.data_as(hprlp.c_int_p)
    calls = {
        "hprlp_solver_power_iteration_many": lambda h, k: L.hprlp_solver_power_iteration_many(h, k, 100, 1e-4, P, I),
        "hprlp_solver_iterate_many": lambda h, k: L.hprlp_solver_iterate_many(h, k, cnt.ctypes.data_as(hprlp.c_int_p), 0),
        "hprlp_solver_run_many": lambda h, k: L.hprlp_solver_run_many(h, k, res),
    }
    for name, call in calls.items():
        for h, k, word in ((None, 2, "null solver list"), (hs, 0, "count must be positive"), (hs, -3, "count must be positive"),
                           (hs, 2, "member 0 is null")):
            assert call(h, k) == -1, (name, word)
            assert name in hprlp.last_error() and word in hprlp.last_error(), (name, word, hprlp.last_error())
    cp = hprlp.Parameters().to_c()
    ms = (C.POINTER(hprlp.CLPInfo) * 2)()
    for m_, k, r_, word in ((None, 2, res, "null model list"), (ms, 0, res, "count must be positive"), (ms, 2, None, "null results"),
                            (ms, 2, res, "model 0 is null")):
        assert L.hprlp_solve_many(m_, k, C.byref(cp), r_) == -1, word
        assert "hprlp_solve_many" in hprlp.last_error() and word in hprlp.last_error(), (word, hprlp.last_error())
    with pytest.raises(ValueError):
        hprlp.solve_many([])


def test_solve_many_without_a_gpu_fails_loudly_member_by_member(capfd):
    """No CPU fallback exists: every member comes back with status ERROR and no arrays, as solve() does."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    lps = [lpgen.planted_lp(30, 50, 200, seed) for seed in (1, 2, 3)]
    models = [hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"],
                                   lp["c"]) for lp in lps]
    out = hprlp.solve_many(models, hprlp.Parameters(max_iter=100))
    assert [r.status for r in out] == ["ERROR"] * 3
    assert all(r.x is None and r.y is None and r.z is None for r in out)
    assert "hprlp_solve_many: model 2" in hprlp.last_error()
    err = capfd.readouterr().err
    for k in range(3):
        assert f"model {k} failed its set-up" in err
    for m in models:
        m.free()
