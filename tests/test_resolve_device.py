"""Device-resident re-solve, the part that needs no GPU (include/hprlp_amd.h hprlp_solver_set_data_device / _resolve_device /
_set_matrix_values_device / _transfer): the prototypes, the exports, the ctypes mirrors and the refusal of a NULL handle."""
import ctypes as C

import numpy as np
import pytest

from conftest import hprlp
from test_resolve import header_prototypes

D, H = "const double *", "double *"
WANT = {
    "hprlp_solver_set_data_device": ["hprlp_solver *"] + [D] * 6 + ["void *"],
    "hprlp_solver_resolve_device": ["hprlp_solver *", "double", D, D, "void *", H, H, H, "HPRLP_results *", "hprlp_trace_row *", "int",
                                    "int *"],
    "hprlp_solver_set_matrix_values_device": ["hprlp_solver *", D, "long"] + [D] * 6 + ["void *"],
    "hprlp_solver_transfer": ["hprlp_solver *", "long *"],
}
# which parameters are HOST arrays (typed pointers in ctypes); every other pointer is a device address or a stream: c_void_p
HOST = {"hprlp_solver_set_data_device": {2: hprlp.c_dbl_p}, "hprlp_solver_resolve_device": {11: hprlp.c_int_p},
        "hprlp_solver_set_matrix_values_device": {4: hprlp.c_dbl_p}, "hprlp_solver_transfer": {1: C.POINTER(C.c_long)}}
PLAIN = {"double": C.c_double, "int": C.c_int, "long": C.c_long, "HPRLP_results *": C.POINTER(hprlp.CResults),
         "hprlp_trace_row *": C.POINTER(hprlp.CTraceRow)}


@pytest.mark.parametrize("name", sorted(WANT))
def test_device_entries_are_declared_exported_and_mirrored(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    want = [HOST[name].get(i, PLAIN.get(p, C.c_void_p)) for i, p in enumerate(params)]
    assert list(fn.argtypes) == want, fn.argtypes
    assert fn.restype is C.c_int


def test_python_solver_has_the_tensor_methods():
    for f in ("set_data_tensors", "resolve_tensors", "set_matrix_tensors", "transfer"):
        assert callable(getattr(hprlp.Solver, f)), f


def test_null_solver_is_refused_by_every_device_entry():
    L = hprlp.lib()
    res = hprlp.CResults()
    out = (C.c_long * 4)()
    one = np.zeros(1)
    calls = {
        "hprlp_solver_set_data_device": lambda: L.hprlp_solver_set_data_device(None, None, one.ctypes.data_as(hprlp.c_dbl_p), None, None, None,
                                                                               None, None),
        "hprlp_solver_resolve_device": lambda: L.hprlp_solver_resolve_device(None, -1.0, None, None, None, None, None, None, C.byref(res),
                                                                             None, 0, None),
        "hprlp_solver_set_matrix_values_device": lambda: L.hprlp_solver_set_matrix_values_device(None, None, 0, None, None, None, None, None,
                                                                                                 None, None),
        "hprlp_solver_transfer": lambda: L.hprlp_solver_transfer(None, out),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name in hprlp.last_error() and "null solver" in hprlp.last_error(), (name, hprlp.last_error())
    assert L.hprlp_solver_transfer(None, None) == -1
