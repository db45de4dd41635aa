"""The resident batched solver, the part that needs no GPU (include/hprlp_amd.h hprlp_batched_solver_*, DESIGN.md "Resident
batches"): the five entry points are exported with the header's signatures, the Python wrappers exist, creation without a GPU
returns NULL with a message, and a NULL handle is refused.  tests/test_gpu_batched_resident.py holds the solver to fresh
solve_batched calls on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen
from test_resolve import header_prototypes

CTYPE_OF = {"hprlp_batched_solver *": C.c_void_p, "const double *": hprlp.c_dbl_p, "double *": hprlp.c_dbl_p, "int": C.c_int,
            "long *": C.POINTER(C.c_long), "const LP_info_cpu *": C.POINTER(hprlp.CLPInfo),
            "const HPRLP_parameters *": C.POINTER(hprlp.CParameters), "const hprlp_detection *": C.POINTER(hprlp.CDetection),
            "hprlp_batched_certificates *": C.POINTER(hprlp.CBatchedCertificates),
            "HPRLP_batched_results *": C.POINTER(hprlp.CBatchedResults)}
WANT = {
    "hprlp_batched_solver_destroy": ("void", ["hprlp_batched_solver *"]),
    "hprlp_batched_solver_solve": ("int", ["hprlp_batched_solver *", "int"] + ["const double *"] * 6 + ["const HPRLP_parameters *"]
                                   + ["const double *"] * 2 + ["int", "const hprlp_detection *", "hprlp_batched_certificates *",
                                                               "HPRLP_batched_results *"]),
    "hprlp_batched_solver_info": ("int", ["hprlp_batched_solver *", "long *"]),
    "hprlp_batched_solver_seconds": ("int", ["hprlp_batched_solver *", "double *"]),
}


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    assert protos[name] == WANT[name], protos[name]
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in WANT[name][1]], fn.argtypes
    if WANT[name][0] == "int":
        assert fn.restype is C.c_int


def test_create_is_exported_and_declared():
    # (it returns a pointer: header_prototypes() only lists the functions that return a plain type)
    text = " ".join(open(os.path.join(ROOT, "include", "hprlp_amd.h")).read().split())
    assert "hprlp_batched_solver *hprlp_batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param);" in text
    fn = hprlp.lib().hprlp_batched_solver_create
    assert fn.restype is C.c_void_p and list(fn.argtypes) == [C.POINTER(hprlp.CLPInfo), C.POINTER(hprlp.CParameters)]


def test_python_wrappers_exist():
    for f in ("solve", "info", "seconds", "close"):
        assert callable(getattr(hprlp.BatchedSolver, f)), f
    assert len(hprlp.BatchedSolver._INFO) == 8 and len(hprlp.BatchedSolver._SECONDS) == 6


def test_create_without_a_gpu_returns_null_with_a_message():
    lp = lpgen.planted_lp(30, 40, 200, 3)
    model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"],
                                 lp["c"])
    L = hprlp.lib()
    assert L.hprlp_batched_solver_create(None, None) is None and "null model" in hprlp.last_error()
    if os.path.exists("/dev/kfd"):  # a machine with a GPU: the handle is made (and what it does is the GPU module's business)
        s = hprlp.BatchedSolver(model)
        assert s.info()["solves"] == 0
        s.close()
    else:
        prm = hprlp.Parameters(use_presolve=False).to_c()
        assert L.hprlp_batched_solver_create(model._ptr, C.byref(prm)) is None
        msg = hprlp.last_error()
        assert msg and "GPU" in msg, msg
        with pytest.raises(RuntimeError, match="GPU"):
            hprlp.BatchedSolver(model)
    model.free()


def test_null_handle_is_refused_with_a_message():
    L = hprlp.lib()
    v = np.zeros(4)
    P = v.ctypes.data_as(hprlp.c_dbl_p)
    res = hprlp.CBatchedResults()
    assert L.hprlp_batched_solver_solve(None, 1, P, P, P, P, P, None, None, None, None, 0, None, None, C.byref(res)) == -1
    assert "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_info(None, (C.c_long * 8)()) == -1
    assert "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_seconds(None, (C.c_double * 6)()) == -1
    assert "null solver" in hprlp.last_error()
    L.hprlp_batched_solver_destroy(None)  # (a no-op)
