"""ctypes host mirror of the HPR-LP boundary (lib/libhprlp.so, include/HPRLP.h + hprlp_amd.h).

Same names and argument meaning as the reference's Python package (reference
bindings/python/hprlp/{model,parameters,results,solver}.py): Parameters, Model.from_arrays /
Model.from_mps, Model.solve, solve_batched, Results.  Plumbing only: every number is produced by the
HIP library; nothing here falls back to a CPU path, and loading fails loudly when the library (or,
for solves, a GPU) is missing.
"""
import ctypes as C
import os
import time
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("HPRLP_LIB") or os.path.join(_ROOT, "lib", "libhprlp.so")  # HPRLP_LIB: developer builds (kernel shape variants)

c_int_p = C.POINTER(C.c_int)
c_dbl_p = C.POINTER(C.c_double)


class CParameters(C.Structure):  # include/structs.h HPRLP_parameters (40 bytes)
    _fields_ = [
        ("max_iter", C.c_int), ("stop_tol", C.c_double), ("time_limit", C.c_double),
        ("device_number", C.c_int), ("check_iter", C.c_int),
        ("CUSPARSE_spmv", C.c_bool), ("autotune_verbose", C.c_bool), ("use_CR_scaling", C.c_bool),
        ("use_Ruiz_scaling", C.c_bool), ("use_Pock_Chambolle_scaling", C.c_bool),
        ("use_bc_scaling", C.c_bool), ("use_presolve", C.c_bool),
    ]


class CResults(C.Structure):  # HPRLP_results (160 bytes)
    _fields_ = [
        ("residuals", C.c_double), ("primal_obj", C.c_double), ("gap", C.c_double),
        ("time4", C.c_double), ("time6", C.c_double), ("time8", C.c_double), ("time", C.c_double),
        ("iter4", C.c_int), ("iter6", C.c_int), ("iter8", C.c_int), ("iter", C.c_int),
        ("status", C.c_char * 64),
        ("x", c_dbl_p), ("y", c_dbl_p), ("z", c_dbl_p),
    ]


class CBatchedResults(C.Structure):  # HPRLP_batched_results (112 bytes)
    _fields_ = [
        ("m", C.c_int), ("n", C.c_int), ("batch_size", C.c_int),
        ("x", c_dbl_p), ("y", c_dbl_p), ("z", c_dbl_p),
        ("primal_obj", c_dbl_p), ("residuals", c_dbl_p), ("gap", c_dbl_p),
        ("iter", c_int_p), ("status", C.POINTER(C.c_char)),
        ("time", C.c_double), ("setup_time", C.c_double), ("solve_time", C.c_double), ("power_time", C.c_double),
    ]


class CSparseMatrix(C.Structure):
    _fields_ = [("row", C.c_int), ("col", C.c_int), ("numElements", C.c_int),
                ("colIndex", c_int_p), ("rowPtr", c_int_p), ("value", c_dbl_p)]


class CLPInfo(C.Structure):
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("A", C.POINTER(CSparseMatrix)),
                ("AL", c_dbl_p), ("AU", c_dbl_p), ("c", c_dbl_p), ("l", c_dbl_p), ("u", c_dbl_p),
                ("obj_constant", C.c_double)]


class CShard(C.Structure):
    """hprlp_shard (include/hprlp_amd.h): one rank's rows of A and of A^T with its vector slices."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("row_off", C.c_int), ("m_loc", C.c_int), ("col_off", C.c_int),
                ("n_loc", C.c_int), ("A_rowptr", c_int_p), ("A_col", c_int_p), ("A_val", c_dbl_p),
                ("AT_rowptr", c_int_p), ("AT_col", c_int_p), ("AT_val", c_dbl_p),
                ("AL", c_dbl_p), ("AU", c_dbl_p), ("l", c_dbl_p), ("u", c_dbl_p), ("c", c_dbl_p), ("obj_constant", C.c_double)]


class CTraceRow(C.Structure):
    _fields_ = [("iter", C.c_int), ("restart_flag", C.c_int)] + [
        (k, C.c_double)
        for k in ("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt", "sigma", "current_gap", "lambda_max")
    ]


class CMemberData(C.Structure):  # hprlp_member_data (include/hprlp_amd.h)
    _fields_ = [(k, c_dbl_p) for k in ("c", "obj_constant", "AL", "AU", "l", "u")]


class CMemberValues(C.Structure):  # hprlp_member_values
    _fields_ = [("val", c_dbl_p), ("nnz", C.c_long)] + [(k, c_dbl_p) for k in ("c", "obj_constant", "AL", "AU", "l", "u")]


class CMemberStart(C.Structure):  # hprlp_member_start
    _fields_ = [("x0", c_dbl_p), ("y0", c_dbl_p), ("sigma", C.c_double)]


class CMemberOut(C.Structure):  # hprlp_member_out: device buffers for one member's solution (None: not wanted)
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p)]


class CDetection(C.Structure):  # hprlp_detection (include/hprlp_amd.h, 16 bytes)
    _fields_ = [("eps_primal_infeasible", C.c_double), ("eps_dual_infeasible", C.c_double)]


class CCertificate(C.Structure):  # hprlp_certificate (include/hprlp_amd.h, 56 bytes)
    _fields_ = [("kind", C.c_int), ("iter", C.c_int), ("m", C.c_int), ("n", C.c_int),
                ("objective", C.c_double), ("violation", C.c_double), ("y", c_dbl_p), ("z", c_dbl_p), ("d", c_dbl_p)]


class CBatchedCertificates(C.Structure):  # hprlp_batched_certificates (include/hprlp_amd.h, 72 bytes)
    _fields_ = [("batch_size", C.c_int), ("m", C.c_int), ("n", C.c_int), ("kind", c_int_p), ("iter", c_int_p),
                ("objective", c_dbl_p), ("violation", c_dbl_p), ("y", c_dbl_p), ("z", c_dbl_p), ("d", c_dbl_p)]


class CBatchedScalars(C.Structure):  # hprlp_batched_scalars (include/hprlp_amd.h): host arrays of the caller's, B each
    _fields_ = [("primal_obj", c_dbl_p), ("residuals", c_dbl_p), ("gap", c_dbl_p), ("iter", c_int_p), ("status", C.POINTER(C.c_char)),
                ("time", C.c_double), ("setup_time", C.c_double), ("solve_time", C.c_double), ("power_time", C.c_double)]


_lib = None
_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _share_hip_runtime():
    """One HIP runtime per process whichever of this library and torch is loaded first.  torch's wheel brings its own copies of
    the runtime's libraries with the system's SONAMEs but asks for them by their UNVERSIONED file names.  Loaded first, torch's
    copies serve this library too (its versioned names match their SONAMEs).  Loaded second, torch would not find the unversioned
    names among the objects this library brought in, load its own copies beside them, and the second HSA runtime of the process
    sees no GPU.  So the unversioned names are added to the objects already loaded: RTLD_NOLOAD opens nothing new -- where a name
    resolves to another file than the one loaded, or to none, nothing happens."""
    for name in ("librocprofiler-register.so", "libhsa-runtime64.so", "libamdhip64.so"):
        try:
            C.CDLL(name, mode=os.RTLD_NOLOAD)
        except OSError:
            pass


def lib():
    """Load lib/libhprlp.so; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `make` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    _share_hip_runtime()
    L.create_model_from_arrays.restype = C.POINTER(CLPInfo)
    L.create_model_from_arrays.argtypes = [C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_dbl_p, c_dbl_p, c_dbl_p,
                                           c_dbl_p, c_dbl_p, c_dbl_p, C.c_bool]
    L.create_model_from_mps.restype = C.POINTER(CLPInfo)
    L.create_model_from_mps.argtypes = [C.c_char_p]
    L.free_model.argtypes = [C.POINTER(CLPInfo)]
    L.solve.restype = CResults
    L.solve.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters)]
    L.HPRLP_main_solve.restype = CResults
    L.HPRLP_main_solve.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters)]
    L.solve_batched.restype = CBatchedResults
    L.solve_batched.argtypes = [C.POINTER(CLPInfo), C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p,
                                C.POINTER(CParameters)]
    L.free_batched_results.argtypes = [C.POINTER(CBatchedResults)]
    L.hprlp_last_error.restype = C.c_char_p
    L.hprlp_backend.restype = C.c_char_p
    L.hprlp_solver_create.restype = C.c_void_p
    L.hprlp_solver_create.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters)]
    L.hprlp_solver_destroy.argtypes = [C.c_void_p]
    L.hprlp_solver_set_verbose.argtypes = [C.c_void_p, C.c_int]
    L.hprlp_solver_scale.argtypes = [C.c_void_p]
    L.hprlp_solver_power_iteration.restype = C.c_double
    L.hprlp_solver_power_iteration.argtypes = [C.c_void_p, C.c_int, C.c_double, c_int_p]
    L.hprlp_solver_init.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.hprlp_solver_iterate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.hprlp_solver_residuals.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dbl_p]
    L.hprlp_solver_restart.argtypes = [C.c_void_p, c_dbl_p, c_dbl_p]
    L.hprlp_solver_weighted_norm.restype = C.c_double
    L.hprlp_solver_weighted_norm.argtypes = [C.c_void_p]
    L.hprlp_solver_run.argtypes = [C.c_void_p, C.POINTER(CResults), C.POINTER(CTraceRow), C.c_int, c_int_p]
    L.hprlp_solver_get_vector.restype = C.c_long
    L.hprlp_solver_get_vector.argtypes = [C.c_void_p, C.c_char_p, c_dbl_p, C.c_long]
    L.hprlp_solver_set_vector.argtypes = [C.c_void_p, C.c_char_p, c_dbl_p, C.c_long]
    L.hprlp_solver_get_scalars.argtypes = [C.c_void_p, c_dbl_p]
    L.hprlp_solver_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    L.hprlp_solver_time_iterations.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]
    L.hprlp_presolve_run.restype = C.c_void_p
    L.hprlp_presolve_run.argtypes = [C.POINTER(CLPInfo)]
    L.hprlp_presolve_reduced.restype = C.POINTER(CLPInfo)
    L.hprlp_presolve_reduced.argtypes = [C.c_void_p]
    L.hprlp_presolve_stats.argtypes = [C.c_void_p, c_int_p]
    L.hprlp_presolve_postsolve.argtypes = [C.c_void_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]
    L.hprlp_presolve_free.argtypes = [C.c_void_p]
    L.hprlp_original_kkt.argtypes = [C.POINTER(CLPInfo), c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]
    L.hprlp_solve_detect.restype = CResults
    L.hprlp_solve_detect.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters), C.POINTER(CDetection), C.POINTER(CCertificate)]
    L.hprlp_free_certificate.argtypes = [C.POINTER(CCertificate)]
    L.hprlp_solver_set_detection.argtypes = [C.c_void_p, C.POINTER(CDetection)]
    L.hprlp_solver_get_certificate.argtypes = [C.c_void_p, C.POINTER(CCertificate)]
    L.hprlp_solver_ray_step.argtypes = [C.c_void_p, C.c_int, c_dbl_p]
    L.hprlp_solve_batched_detect.restype = CBatchedResults
    L.hprlp_solve_batched_detect.argtypes = [C.POINTER(CLPInfo), C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p,
                                             C.POINTER(CParameters), C.POINTER(CDetection), C.POINTER(CBatchedCertificates)]
    L.hprlp_free_batched_certificates.argtypes = [C.POINTER(CBatchedCertificates)]
    L.hprlp_solve_warm.restype = CResults
    L.hprlp_solve_warm.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters), c_dbl_p, c_dbl_p, C.POINTER(CDetection),
                                   C.POINTER(CCertificate)]
    L.hprlp_solve_batched_warm.restype = CBatchedResults
    L.hprlp_solve_batched_warm.argtypes = [C.POINTER(CLPInfo), C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p,
                                           C.POINTER(CParameters), c_dbl_p, c_dbl_p, C.POINTER(CDetection),
                                           C.POINTER(CBatchedCertificates)]
    L.hprlp_batched_solver_create.restype = C.c_void_p
    L.hprlp_batched_solver_create.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters)]
    L.hprlp_batched_solver_destroy.argtypes = [C.c_void_p]
    L.hprlp_batched_solver_solve.argtypes = [C.c_void_p, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p,
                                             C.POINTER(CParameters), c_dbl_p, c_dbl_p, C.c_int, C.POINTER(CDetection),
                                             C.POINTER(CBatchedCertificates), C.POINTER(CBatchedResults)]
    L.hprlp_batched_solver_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    L.hprlp_batched_solver_seconds.argtypes = [C.c_void_p, c_dbl_p]
    L.hprlp_batched_solver_solve_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [c_dbl_p, C.POINTER(CParameters)] + \
        [C.c_void_p] * 2 + [C.c_int, C.POINTER(CDetection), C.POINTER(CBatchedCertificates)] + [C.c_void_p] * 4 + \
        [C.POINTER(CBatchedScalars)]
    L.hprlp_batched_solver_set_norms.argtypes = [C.c_void_p, C.c_int]
    L.hprlp_batched_solver_scalars.argtypes = [C.c_void_p, c_dbl_p]
    L.hprlp_batched_solver_transfer.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    L.hprlp_batched_solver_ray_step.argtypes = [C.c_void_p, c_int_p, C.c_int, c_dbl_p, c_int_p]
    L.hprlp_batched_solver_get_panel.restype = C.c_long
    L.hprlp_batched_solver_get_panel.argtypes = [C.c_void_p, C.c_char_p, c_dbl_p, C.c_long]
    L.hprlp_batched_solver_set_panel.argtypes = [C.c_void_p, C.c_char_p, c_dbl_p, C.c_long]
    if hasattr(L, "hprlp_batched_solver_solve_stream"):  # (HPRLP_LIB may name a build of an earlier commit: _need_stream() says so)
        L.hprlp_batched_solver_solve_stream.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_dbl_p] * 6 + \
            [C.POINTER(CParameters), c_dbl_p, c_dbl_p, C.POINTER(CDetection), C.POINTER(CBatchedCertificates), C.POINTER(CBatchedResults)]
        L.hprlp_batched_solver_stream_record.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int_p]
        L.hprlp_batched_solver_stream_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        L.hprlp_batched_solver_stream_seconds.argtypes = [C.c_void_p, c_dbl_p]
        L.hprlp_batched_solver_lambda.argtypes = [C.c_void_p, c_dbl_p]
        L.hprlp_stream_schedule_host.argtypes = [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p]
    if hasattr(L, "hprlp_batched_solver_solve_stream_device"):  # (likewise)
        L.hprlp_batched_solver_solve_stream_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + \
            [c_dbl_p, C.POINTER(CParameters)] + [C.c_void_p] * 2 + [C.POINTER(CDetection), C.POINTER(CBatchedCertificates)] + \
            [C.c_void_p] * 4 + [C.POINTER(CBatchedScalars)]
        L.hprlp_batched_solver_stream_memory.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    if hasattr(L, "hprlp_batched_solver_solve_stream_parents"):  # (likewise: _need_parents() says so)
        L.hprlp_batched_solver_solve_stream_parents.argtypes = [C.c_void_p, C.c_int, C.c_int] + [c_dbl_p] * 6 + \
            [C.POINTER(CParameters), c_dbl_p, c_dbl_p, c_int_p, C.POINTER(CDetection), C.POINTER(CBatchedCertificates),
             C.POINTER(CBatchedResults)]
        L.hprlp_batched_solver_solve_stream_parents_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + \
            [c_dbl_p, C.POINTER(CParameters)] + [C.c_void_p] * 2 + [c_int_p, C.POINTER(CDetection), C.POINTER(CBatchedCertificates)] + \
            [C.c_void_p] * 4 + [C.POINTER(CBatchedScalars)]
        L.hprlp_batched_solver_stream_parents_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        L.hprlp_stream_schedule_parents_host.argtypes = [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]
    L.hprlp_batched_prepare_host_rule.argtypes =[C.c_int] * 3 + [c_dbl_p] * 9 + [C.c_int, C.c_int, C.POINTER(CBatchedPrepared)]
    L.hprlp_solver_set_start.argtypes = [C.c_void_p, c_dbl_p, c_dbl_p]
    L.hprlp_solver_set_data.argtypes = [C.c_void_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]
    L.hprlp_solver_resolve.argtypes = [C.c_void_p, C.c_double, c_dbl_p, c_dbl_p, C.POINTER(CResults), C.POINTER(CTraceRow),
                                       C.c_int, c_int_p]
    L.hprlp_solver_data_seconds.argtypes = [C.c_void_p, c_dbl_p]
    L.hprlp_solver_set_matrix_values.argtypes = [C.c_void_p, c_dbl_p, C.c_long] + [c_dbl_p] * 6
    L.hprlp_solver_matrix_seconds.argtypes = [C.c_void_p, c_dbl_p]
    if hasattr(L, "hprlp_solver_transfer"):  # (HPRLP_LIB may name a build of an earlier commit)
        # device arrays travel as addresses (c_void_p), host arrays as before
        L.hprlp_solver_set_data_device.argtypes = [C.c_void_p, C.c_void_p, c_dbl_p] + [C.c_void_p] * 5
        L.hprlp_solver_resolve_device.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 6 + \
            [C.POINTER(CResults), C.POINTER(CTraceRow), C.c_int, c_int_p]
        L.hprlp_solver_set_matrix_values_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, c_dbl_p] + [C.c_void_p] * 5
        L.hprlp_solver_transfer.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    L.hprlp_solver_value_maps.restype = C.c_long
    L.hprlp_solver_value_maps.argtypes = [C.c_void_p, c_int_p, c_int_p, C.c_long]
    L.hprlp_solver_ordering.argtypes = [C.c_void_p, c_int_p, c_int_p]
    L.hprlp_value_maps_host.argtypes = [C.c_int, C.c_int] + [c_int_p] * 6
    L.hprlp_batched_solver_set_matrix_values.argtypes = [C.c_void_p, c_dbl_p, C.c_long]
    L.hprlp_presolve_forward.argtypes = [C.c_void_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]
    L.hprlp_solver_power_iteration_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, c_dbl_p, c_int_p]
    L.hprlp_solver_iterate_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, c_int_p, C.c_int]
    L.hprlp_solver_run_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CResults)]
    L.hprlp_solve_many.argtypes = [C.POINTER(C.POINTER(CLPInfo)), C.c_int, C.POINTER(CParameters), C.POINTER(CResults)]
    L.hprlp_last_solve_many_phases.argtypes = [c_dbl_p]
    if hasattr(L, "hprlp_last_run_many_counts"):  # (HPRLP_LIB may name a build of an earlier commit: the A side of tools/many_ab.py)
        L.hprlp_solver_residuals_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, c_int_p, c_int_p, c_dbl_p]
        L.hprlp_solver_restart_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, c_dbl_p, c_dbl_p]
        L.hprlp_last_run_many_counts.argtypes = [C.POINTER(C.c_long)]
    if hasattr(L, "hprlp_solve_many_detect"):  # (likewise: the A side of tools/many_detect_ab.py)
        L.hprlp_solve_many_detect.argtypes = [C.POINTER(C.POINTER(CLPInfo)), C.c_int, C.POINTER(CParameters), C.POINTER(CDetection),
                                              C.POINTER(CResults), C.POINTER(CCertificate)]
        L.hprlp_solver_ray_step_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, c_int_p, c_dbl_p, c_int_p]
    if hasattr(L, "hprlp_solver_set_group_wide"):  # (likewise: the A side of tools/many_wide_ab.py)
        L.hprlp_solver_set_group_wide.argtypes = [C.c_void_p, C.c_int]
        L.hprlp_solve_many_wide.argtypes = [C.POINTER(C.POINTER(CLPInfo)), C.c_int, C.POINTER(CParameters), C.POINTER(CDetection),
                                            C.POINTER(CResults), C.POINTER(CCertificate)]
        L.hprlp_last_many_wide_counts.argtypes = [C.POINTER(C.c_long)]
        L.hprlp_group_iteration_plan.argtypes = [c_int_p, C.c_int, c_int_p, c_int_p, C.c_int]
    if hasattr(L, "hprlp_solver_create_many"):  # (likewise)
        L.hprlp_solver_create_many.argtypes = [C.POINTER(C.POINTER(CLPInfo)), C.c_int, C.POINTER(CParameters), C.POINTER(C.c_void_p)]
        L.hprlp_solver_scale_many.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.hprlp_solver_destroy_many.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.hprlp_solver_destroy_many.restype = None
        L.hprlp_last_setup_many_counts.argtypes = [C.POINTER(C.c_long)]
    if hasattr(L, "hprlp_solver_resolve_many"):  # (likewise: the A side of tools/many_resolve_ab.py)
        L.hprlp_solver_set_data_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberData)]
        L.hprlp_solver_resolve_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberStart), C.POINTER(CResults)]
        L.hprlp_last_resolve_many_counts.argtypes = [C.POINTER(C.c_long)]
        L.hprlp_group_pack_selftest.argtypes = []
    if hasattr(L, "hprlp_group_table_selftest"):  # (likewise)
        L.hprlp_group_table_selftest.argtypes = []
    if hasattr(L, "hprlp_solver_set_matrix_values_many"):  # (likewise)
        L.hprlp_solver_set_matrix_values_many.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberValues)]
        L.hprlp_last_values_many_counts.argtypes = [C.POINTER(C.c_long)]
    if hasattr(L, "hprlp_solver_resolve_many_device"):  # (likewise)
        L.hprlp_solver_set_data_many_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberData), C.c_void_p]
        L.hprlp_solver_resolve_many_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberStart), C.POINTER(CMemberOut),
                                                       C.c_void_p, C.POINTER(CResults)]
        L.hprlp_solver_set_matrix_values_many_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CMemberValues), C.c_void_p]
        L.hprlp_last_many_device_counts.argtypes = [C.POINTER(C.c_long)]
    _lib = L
    return L


def last_error():
    return lib().hprlp_last_error().decode()


def _need_stream():
    """The streamed-batch entries are in every build of this tree; a library named by HPRLP_LIB may be older."""
    if not hasattr(lib(), "hprlp_batched_solver_solve_stream"):
        raise RuntimeError(f"{LIB_PATH} has no hprlp_batched_solver_solve_stream: a build of an earlier commit (HPRLP_LIB?)")


class Parameters:
    """Solver parameters; defaults of reference include/structs.h:26-39."""

    _names = [f for f, _ in CParameters._fields_]

    def __init__(self, **kw):
        self.max_iter = 2**31 - 1
        self.stop_tol = 1e-4
        self.time_limit = 3600.0
        self.device_number = 0
        self.check_iter = 150
        self.CUSPARSE_spmv = False
        self.autotune_verbose = False
        self.use_CR_scaling = True
        self.use_Ruiz_scaling = True
        self.use_Pock_Chambolle_scaling = True
        self.use_bc_scaling = True
        self.use_presolve = True
        for k, v in kw.items():
            if k not in self._names:
                raise AttributeError(k)
            setattr(self, k, v)

    def to_c(self):
        return CParameters(*[getattr(self, k) for k in self._names])


def _as(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _take(ptr, n):
    """A malloc'd result array as a numpy array (the caller owns HPRLP_results.x/y/z).  Short vectors are copied and freed at
    once; long ones are adopted without a copy -- the array keeps the C buffer and free()s it when the last view is gone (three
    copies of 80 MB were 36 ms of a config-5 solve's wall time on the Python side)."""
    if not ptr:
        return None
    view = np.ctypeslib.as_array(ptr, shape=(n,))
    if n < (1 << 20):
        out = view.copy()
        _libc.free(C.cast(ptr, C.c_void_p))
        return out
    addr = C.cast(ptr, C.c_void_p).value
    buf = (C.c_double * n).from_address(addr)
    weakref.finalize(buf, _libc.free, C.c_void_p(addr))
    return np.frombuffer(buf, dtype=np.float64)  # (its .base keeps `buf` alive)


class Results:
    def __init__(self, cres, m, n):
        self.status = cres.status.decode()
        for k in ("residuals", "primal_obj", "gap", "time4", "time6", "time8", "time", "iter4", "iter6", "iter8", "iter"):
            setattr(self, k, getattr(cres, k))
        self.x = _take(cres.x, n)
        self.y = _take(cres.y, m)
        self.z = _take(cres.z, n)


class Certificate:
    """Infeasibility certificate (hprlp_certificate): kind 0 none, 1 primal infeasible (y, z = -A^T y), 2 dual infeasible (d);
    the ray has infinity norm 1, objective / violation are D(y), V(y) resp. c'd, W(d) of it (include/hprlp_amd.h)."""

    KINDS = {0: None, 1: "PRIMAL_INFEASIBLE", 2: "DUAL_INFEASIBLE"}

    def __init__(self, cc):
        self.kind, self.iter, self.m, self.n = cc.kind, cc.iter, cc.m, cc.n
        self.objective, self.violation = cc.objective, cc.violation
        g = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy() if p else None
        self.y, self.z, self.d = g(cc.y, cc.m), g(cc.z, cc.n), g(cc.d, cc.n)
        lib().hprlp_free_certificate(C.byref(cc))

    @property
    def verdict(self):
        return self.KINDS.get(self.kind)


def _detection(eps_primal, eps_dual):
    return CDetection(float(eps_primal), float(eps_dual))


def _detection_arg(eps_primal, eps_dual):
    """The solve entries' eps arguments as a CDetection (either None: 1e-8), or None when both are None (detection off)."""
    if eps_primal is None and eps_dual is None:
        return None
    return _detection(1e-8 if eps_primal is None else eps_primal, 1e-8 if eps_dual is None else eps_dual)


def _batched_certificates(cc):
    """A filled CBatchedCertificates as the "certificates" dict of solve_batched_detect(); frees the C arrays."""
    B, m, n = cc.batch_size, cc.m, cc.n
    g = lambda q, k, dt=np.float64: None if not q else np.ctypeslib.as_array(q, shape=(k,)).astype(dt, copy=True)
    panel = lambda q, rows: None if not q else g(q, rows * B).reshape(B, rows).T.copy()
    out = dict(kind=g(cc.kind, B, np.int32), iter=g(cc.iter, B, np.int32), objective=g(cc.objective, B),
               violation=g(cc.violation, B), y=panel(cc.y, m), z=panel(cc.z, n), d=panel(cc.d, n))
    lib().hprlp_free_batched_certificates(C.byref(cc))
    return out


def _start_vector(v, length, name):
    """A warm-start vector as a contiguous float64 array of the given length (None stays None: zeros)."""
    if v is None:
        return None
    a = _as(v, np.float64)
    if a.ndim != 1 or a.shape[0] != length:
        raise ValueError(f"warm start: {name} must have length {length}, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"warm start: {name} has a non-finite entry")
    return a


def _start_panel(V, rows, B, name):
    """A batched warm-start panel (rows x B) as a column-major float64 array (None stays None: zeros)."""
    if V is None:
        return None
    a = np.asfortranarray(V, dtype=np.float64)
    if a.shape != (rows, B):
        raise ValueError(f"warm start: {name} must have shape ({rows}, {B}), got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"warm start: {name} has a non-finite entry")
    return a


def _dptr(a):
    return None if a is None else a.ctypes.data_as(c_dbl_p)


class Model:
    """LP model: min c'x s.t. AL <= Ax <= AU, l <= x <= u (wraps LP_info_cpu*)."""

    def __init__(self, ptr):
        if not ptr:
            raise RuntimeError("model creation failed (see stderr)")
        self._ptr = ptr

    @property
    def m(self):
        return self._ptr.contents.m

    @property
    def n(self):
        return self._ptr.contents.n

    @property
    def obj_constant(self):
        return self._ptr.contents.obj_constant

    @property
    def nnz(self):
        return self._ptr.contents.A.contents.numElements

    @staticmethod
    def from_csr(m, n, rowptr, colind, values, AL, AU, l, u, c, is_csc=False):
        rp = _as(rowptr, np.int32); ci = _as(colind, np.int32); v = _as(values, np.float64)
        AL = _as(AL, np.float64); AU = _as(AU, np.float64); l = _as(l, np.float64); u = _as(u, np.float64)
        c = _as(c, np.float64)
        P = lambda a: a.ctypes.data_as(c_dbl_p)
        ptr = lib().create_model_from_arrays(m, n, len(v), rp.ctypes.data_as(c_int_p), ci.ctypes.data_as(c_int_p),
                                             P(v), P(AL), P(AU), P(l), P(u), P(c), bool(is_csc))
        return Model(ptr)

    @staticmethod
    def from_arrays(A, AL, AU, l, u, c):
        """A: dense ndarray or scipy.sparse matrix (reference bindings/python/hprlp/model.py:96-174)."""
        from scipy import sparse
        A = sparse.csr_matrix(A)
        A.sort_indices()
        m, n = A.shape
        return Model.from_csr(m, n, A.indptr, A.indices, A.data, AL, AU, l, u, c)

    @staticmethod
    def from_mps(path):
        return Model(lib().create_model_from_mps(str(path).encode()))

    def csr(self):
        """Host copy of the stored CSR arrays (rowPtr, colIndex, value)."""
        A = self._ptr.contents.A.contents
        rp = np.ctypeslib.as_array(A.rowPtr, shape=(A.row + 1,)).copy()
        ci = np.ctypeslib.as_array(A.colIndex, shape=(A.numElements,)).copy()
        v = np.ctypeslib.as_array(A.value, shape=(A.numElements,)).copy()
        return rp, ci, v

    def vectors(self):
        p = self._ptr.contents
        g = lambda q, k: np.ctypeslib.as_array(q, shape=(k,)).copy()
        return dict(AL=g(p.AL, p.m), AU=g(p.AU, p.m), l=g(p.l, p.n), u=g(p.u, p.n), c=g(p.c, p.n))

    def solve(self, param=None):
        cp = (param or Parameters()).to_c()
        L = lib()
        t0 = time.perf_counter()
        res = L.solve(self._ptr, C.byref(cp))
        wall = time.perf_counter() - t0
        r = Results(res, self.m, self.n)
        r.c_call_wall_s = wall  # the caller's clock around the C call alone (before the solution vectors are wrapped)
        return r

    def solve_detect(self, param=None, eps_primal=1e-8, eps_dual=1e-8):
        """solve() with infeasibility detection (hprlp_solve_detect): status PRIMAL_INFEASIBLE / DUAL_INFEASIBLE with the
        certificate in `.certificate`.  eps_primal=None and eps_dual=None: detection off (exactly solve())."""
        cp = (param or Parameters()).to_c()
        det = _detection_arg(eps_primal, eps_dual)
        cc = CCertificate()
        res = lib().hprlp_solve_detect(self._ptr, C.byref(cp), C.byref(det) if det is not None else None, C.byref(cc))
        r = Results(res, self.m, self.n)
        r.certificate = Certificate(cc)
        return r

    def solve_warm(self, x=None, y=None, param=None, eps_primal=None, eps_dual=None):
        """solve() from the primal-dual point (x, y) in this model's units (hprlp_solve_warm; None: zeros, both None: exactly
        solve()).  eps_primal / eps_dual not None: with infeasibility detection, the certificate in `.certificate`."""
        xs, ys = _start_vector(x, self.n, "x"), _start_vector(y, self.m, "y")
        cp = (param or Parameters()).to_c()
        det = _detection_arg(eps_primal, eps_dual)
        cc = CCertificate()
        res = lib().hprlp_solve_warm(self._ptr, C.byref(cp), _dptr(xs), _dptr(ys), C.byref(det) if det is not None else None,
                                     C.byref(cc))
        r = Results(res, self.m, self.n)
        if det is not None:
            r.certificate = Certificate(cc)
        return r

    def free(self):
        if self._ptr:
            lib().free_model(self._ptr)
            self._ptr = None


class Presolved:
    """Host-side presolve of a model (include/hprlp_amd.h hprlp_presolve_*): `reduced` is a Model view owned by
    this object; postsolve() maps a reduced primal-dual solution back.  Raises if the model is left unchanged."""

    def __init__(self, model):
        self.model = model
        self.h = lib().hprlp_presolve_run(model._ptr)
        if not self.h:
            raise RuntimeError(last_error())
        self.reduced = Model(lib().hprlp_presolve_reduced(self.h))
        out = (C.c_int * 16)()
        lib().hprlp_presolve_stats(self.h, out)
        keys = ("m", "n", "fixed_cols", "empty_cols", "singleton_rows", "empty_rows", "redundant_rows", "passes", "dual_fixed_cols", "slack_cols", "parallel_rows", "parallel_cols", "forcing_rows", "doubleton_rows", "tightened_bounds", "rounds")
        self.stats = dict(zip(keys, [int(v) for v in out]))

    def postsolve(self, xr, yr, zr):
        xr, yr, zr = _as(xr, np.float64), _as(yr, np.float64), _as(zr, np.float64)
        x, y, z = np.zeros(self.model.n), np.zeros(self.model.m), np.zeros(self.model.n)
        P = lambda a: a.ctypes.data_as(c_dbl_p)
        if lib().hprlp_presolve_postsolve(self.h, P(xr), P(yr), P(zr), P(x), P(y), P(z)) != 0:
            raise RuntimeError("postsolve failed")
        return x, y, z

    def forward(self, x, y):
        """(x, y) of the original model -> (xr, yr) of the reduced one (hprlp_presolve_forward)."""
        x, y = _start_vector(x, self.model.n, "x"), _start_vector(y, self.model.m, "y")
        xr, yr = np.zeros(self.reduced.n), np.zeros(self.reduced.m)
        if lib().hprlp_presolve_forward(self.h, _dptr(x), _dptr(y), _dptr(xr), _dptr(yr)) != 0:
            raise RuntimeError("presolve forward map failed")
        return xr, yr

    def free(self):
        if self.h:
            self.reduced._ptr = None  # owned by the presolve object
            lib().hprlp_presolve_free(self.h)
            self.h = None


def last_solve_phases():
    """Phases [s] of this thread's last HPRLP_main_solve (hprlp_last_solve_phases)."""
    out = (C.c_double * 8)()
    L = lib()
    L.hprlp_last_solve_phases.argtypes = [C.POINTER(C.c_double)]
    L.hprlp_last_solve_phases(out)
    keys = ("device_setup", "scaling", "power_iteration", "loop", "collect_solution", "teardown", "whole_call")
    return dict(zip(keys, [float(v) for v in out]))


def original_kkt(model, x, y, z):
    """Relative primal / dual infeasibility and gap of (x, y, z) on the model as given."""
    x, y, z = _as(x, np.float64), _as(y, np.float64), _as(z, np.float64)
    out = np.zeros(5)
    P = lambda a: a.ctypes.data_as(c_dbl_p)
    if lib().hprlp_original_kkt(model._ptr, P(x), P(y), P(z), P(out)) != 0:
        raise RuntimeError("original_kkt failed")
    return dict(primal_feas=out[0], dual_feas=out[1], gap=out[2], primal_obj=out[3], dual_obj=out[4])


def solve(A, AL, AU, l, u, c, param=None):
    model = Model.from_arrays(A, AL, AU, l, u, c)
    try:
        return model.solve(param)
    finally:
        model.free()


def solve_many(models, param=None):
    """Many independent LPs at once (hprlp_solve_many): what Model.solve does without presolve (use_presolve is ignored), with
    the power iterations and the loops of all models advanced together -- Netlib-scale models share their launches, one
    workgroup each.  Returns a list of Results; a model that failed its set-up has status "ERROR"."""
    models = list(models)
    if not models:
        raise ValueError("solve_many: no models")
    cp = (param or Parameters()).to_c()
    ptrs = (C.POINTER(CLPInfo) * len(models))(*[mod._ptr for mod in models])
    res = (CResults * len(models))()
    if lib().hprlp_solve_many(ptrs, len(models), C.byref(cp), res) < 0:
        raise RuntimeError(last_error())
    return [Results(res[k], mod.m, mod.n) for k, mod in enumerate(models)]


def solve_many_detect(models, param=None, eps_primal=1e-8, eps_dual=1e-8):
    """solve_many with infeasibility detection on for every member (hprlp_solve_many_detect).  Returns (results, certificates):
    one Results and one Certificate per model; kind 0 where the member reached no verdict.  eps_primal=None and eps_dual=None:
    detection off (exactly solve_many)."""
    models = list(models)
    if not models:
        raise ValueError("solve_many_detect: no models")
    cp = (param or Parameters()).to_c()
    det = _detection_arg(eps_primal, eps_dual)
    ptrs = (C.POINTER(CLPInfo) * len(models))(*[mod._ptr for mod in models])
    res = (CResults * len(models))()
    ccs = (CCertificate * len(models))()
    if lib().hprlp_solve_many_detect(ptrs, len(models), C.byref(cp), C.byref(det) if det is not None else None, res, ccs) < 0:
        raise RuntimeError(last_error())
    results = [Results(res[k], mod.m, mod.n) for k, mod in enumerate(models)]
    certificates = [Certificate(ccs[k]) for k in range(len(models))]
    for r, k in zip(results, certificates):
        r.certificate = k
    return results, certificates


def solve_many_wide(models, param=None, eps_primal=None, eps_dual=None):
    """solve_many_detect with every member wide (hprlp_solve_many_wide): a model past the single-workgroup size iterates in the
    group launches instead of issuing its own launches inside the lock-step (Solver.set_group_wide; DESIGN.md "Many small LPs",
    wide members).  Same bits per member as Model.solve without presolve.  Detection is off unless eps_primal / eps_dual are
    given.  Returns (results, certificates) as solve_many_detect."""
    models = list(models)
    if not models:
        raise ValueError("solve_many_wide: no models")
    cp = (param or Parameters()).to_c()
    det = _detection_arg(eps_primal, eps_dual)
    ptrs = (C.POINTER(CLPInfo) * len(models))(*[mod._ptr for mod in models])
    res = (CResults * len(models))()
    ccs = (CCertificate * len(models))()
    if lib().hprlp_solve_many_wide(ptrs, len(models), C.byref(cp), C.byref(det) if det is not None else None, res, ccs) < 0:
        raise RuntimeError(last_error())
    results = [Results(res[k], mod.m, mod.n) for k, mod in enumerate(models)]
    certificates = [Certificate(ccs[k]) for k in range(len(models))]
    for r, k in zip(results, certificates):
        r.certificate = k
    return results, certificates


MANY_WIDE_KEYS = ("joined", "refused", "normal_launches", "segments", "member_iterations", "power_launches", "power_waits")


def last_many_wide_counts():
    """Counts of this thread's last *_many call that had a wide member (hprlp_last_many_wide_counts): wide members that joined
    the group launches / that could not, the group launches of their normal iterations (two per iteration of a segment), the
    segments, the member-iterations they served, the group launches of the power iteration and its host waits."""
    out = (C.c_long * 8)()
    lib().hprlp_last_many_wide_counts(out)
    return dict(zip(MANY_WIDE_KEYS, [int(v) for v in out]))


def group_iteration_plan(counts, cap=None):
    """The segments of a round's normal iterations (hprlp_group_iteration_plan; no GPU needed): [(length, min_count), ...], or
    None where the library refuses (a negative count, more segments than cap)."""
    cnt = _as(counts, np.int32).reshape(-1)
    cap = len(cnt) if cap is None else int(cap)
    ln, at = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    n = lib().hprlp_group_iteration_plan(cnt.ctypes.data_as(c_int_p), len(cnt), ln.ctypes.data_as(c_int_p), at.ctypes.data_as(c_int_p), cap)
    return None if n < 0 else [(int(ln[j]), int(at[j])) for j in range(n)]


def last_solve_many_phases():
    """Phases of this thread's last solve_many (hprlp_last_solve_many_phases): seconds, then the loop's counts."""
    out = np.zeros(8)
    lib().hprlp_last_solve_many_phases(out.ctypes.data_as(c_dbl_p))
    keys = ("setup", "scaling", "power", "loop", "call", "rounds", "waits", "launches")
    return dict(zip(keys, [float(v) for v in out]))


def last_run_many_counts():
    """Counts of this thread's last Solver.run_many / solve_many (hprlp_last_run_many_counts); the two counts of the group
    detection are in last_run_many_detect_counts()."""
    out = (C.c_long * 8)()
    lib().hprlp_last_run_many_counts(out)
    keys = ("rounds", "waits", "group_launches", "copies", "own", "served")
    return dict(zip(keys, [int(v) for v in out]))


def last_run_many_detect_counts():
    """All eight slots of hprlp_last_run_many_counts after Solver.run_many / solve_many / solve_many_detect: the six of
    last_run_many_counts(), then the member ray tests served by group launches and the certificates collected through the
    group's block (a library of an earlier commit reports 0 for both)."""
    out = (C.c_long * 8)()
    lib().hprlp_last_run_many_counts(out)
    keys = ("rounds", "waits", "group_launches", "copies", "own", "served", "ray_served", "certs_served")
    return dict(zip(keys, [int(v) for v in out]))


SETUP_MANY_KEYS = ("device allocations", "pinned allocations", "host-to-device copies", "scaling launches", "scaling host waits",
                   "members served by group scaling launches", "members that scaled on their own", "device frees")


def last_setup_many_counts():
    """Counts of this thread's last Solver.create_many / scale_many / close_many (hprlp_last_setup_many_counts): each call fills
    its own slots; solve_many fills all of them."""
    out = (C.c_long * 8)()
    lib().hprlp_last_setup_many_counts(out)
    return dict(zip(SETUP_MANY_KEYS, [int(v) for v in out]))


RESOLVE_MANY_KEYS = ("host-to-device copies", "device-to-host copies", "host waits outside the loop", "launches outside the loop",
                     "memsets", "members served by group launches", "members that went their own way",
                     "loop operations issued for one member")


def last_resolve_many_counts():
    """Counts of this thread's last Solver.set_data_many / resolve_many, whichever came last
    (hprlp_last_resolve_many_counts); the last slot is resolve_many's alone."""
    out = (C.c_long * 8)()
    lib().hprlp_last_resolve_many_counts(out)
    return dict(zip(RESOLVE_MANY_KEYS, [int(v) for v in out]))


VALUES_MANY_KEYS = ("host-to-device copies", "device-to-host copies", "host waits", "kernel launches", "memsets",
                    "members served by group launches", "members that went their own way", "members whose value maps were built")


def last_values_many_counts():
    """Counts of this thread's last Solver.set_matrix_many (hprlp_last_values_many_counts)."""
    out = (C.c_long * 8)()
    lib().hprlp_last_values_many_counts(out)
    return dict(zip(VALUES_MANY_KEYS, [int(v) for v in out]))


MANY_DEVICE_KEYS = ("device pointers checked", "lookups issued to the runtime", "check-kernel launches", "flag words copied back",
                    "members served by group launches", "members on their own", "waits before the first write")


def last_many_device_counts():
    """Counts of this thread's last Solver.set_data_many_tensors / resolve_many_tensors / set_matrix_many_tensors
    (hprlp_last_many_device_counts); a refused call reports what it did up to its refusal."""
    out = (C.c_long * 8)()
    lib().hprlp_last_many_device_counts(out)
    return dict(zip(MANY_DEVICE_KEYS, [int(v) for v in out]))


def _dev_dbl(addr):
    """A device address as the const double * of the member structs (None stays NULL)."""
    return None if addr is None else C.cast(C.c_void_p(addr), c_dbl_p)


# The per-vector converters of the group methods' array builders (Solver._member_data / _member_values / _member_starts): one
# member's vector as (what keeps it alive until the call returns, the pointer for the member struct); None stays (None, None).
# length None: the matrix values -- one-dimensional, of any length (a wrong count is the library's to refuse, naming the member).
def _host_vector(sv, v, length, name, who):
    """numpy in, for the host group entries."""
    if length is None and v is not None:
        a = _as(v, np.float64)
        if a.ndim != 1:
            raise ValueError(f"{who}: {name} must be one-dimensional, got shape {a.shape}")
    else:
        a = sv._data_vector(v, length, name)
    return a, _dptr(a)


def _device_vector(sv, t, length, name, who):
    """torch tensors in, for the device group entries (*_many_tensors)."""
    if length is None and t is not None:
        if getattr(t, "ndim", 0) != 1:
            raise ValueError(f"{who}: {name} must be a one-dimensional tensor")
        length = t.shape[0]
    t, addr = sv._tensor(t, length, name, who)
    return t, _dev_dbl(addr)


def _need_parents():
    if not hasattr(lib(), "hprlp_batched_solver_solve_stream_parents"):
        raise RuntimeError(f"{LIB_PATH} has no hprlp_batched_solver_solve_stream_parents: a build of an earlier commit (HPRLP_LIB?)")


def _parent_array(parent, N):
    """A parent list as a contiguous C int array of N entries (its values: by the library)."""
    a = np.ascontiguousarray(parent, dtype=np.intc)
    if a.shape != (N,):
        raise ValueError(f"parent must have {N} entries, got shape {a.shape}")
    return a


def solve_batched(model, Cmat, AL, AU, l, u, obj_constants=None, param=None):
    """Cmat,l,u: (n,B) arrays; AL,AU: (m,B) arrays (any layout; passed column-major as the ABI asks)."""
    return _batched_call(lambda B, args, cp: lib().solve_batched(model._ptr, B, *args, C.byref(cp)),
                         model, Cmat, AL, AU, l, u, obj_constants, param)


def solve_batched_detect(model, Cmat, AL, AU, l, u, obj_constants=None, param=None, eps_primal=1e-8, eps_dual=1e-8):
    """solve_batched() with infeasibility detection per member (hprlp_solve_batched_detect): statuses PRIMAL_INFEASIBLE /
    DUAL_INFEASIBLE, and "certificates": kind, iter, objective, violation (length B), y (m, B), z and d (n, B) or None; a
    member's columns are zero where its kind does not use them.  eps_primal=None and eps_dual=None: detection off (exactly
    solve_batched())."""
    det = _detection_arg(eps_primal, eps_dual)
    cc = CBatchedCertificates()

    def call(B, args, cp):
        return lib().hprlp_solve_batched_detect(model._ptr, B, *args, C.byref(cp), C.byref(det) if det is not None else None,
                                                C.byref(cc))
    out = _batched_call(call, model, Cmat, AL, AU, l, u, obj_constants, param)
    out["certificates"] = _batched_certificates(cc)
    return out


def solve_batched_warm(model, Cmat, AL, AU, l, u, X0=None, Y0=None, obj_constants=None, param=None, eps_primal=None,
                       eps_dual=None):
    """solve_batched() from per-member starts (hprlp_solve_batched_warm): X0 (n, B) and Y0 (m, B) in each member's units (None:
    zeros; both None: exactly solve_batched()).  eps_primal / eps_dual not None: with detection, "certificates" as in
    solve_batched_detect()."""
    B = np.asarray(Cmat).shape[1]
    X0, Y0 = _start_panel(X0, model.n, B, "X0"), _start_panel(Y0, model.m, B, "Y0")
    det = _detection_arg(eps_primal, eps_dual)
    cc = CBatchedCertificates()

    def call(B, args, cp):
        return lib().hprlp_solve_batched_warm(model._ptr, B, *args, C.byref(cp), _dptr(X0), _dptr(Y0),
                                              C.byref(det) if det is not None else None, C.byref(cc) if det is not None else None)
    out = _batched_call(call, model, Cmat, AL, AU, l, u, obj_constants, param)
    if det is not None:
        out["certificates"] = _batched_certificates(cc)
    return out


class BatchedSolver:
    """A sequence of batches over one matrix (hprlp_batched_solver_*, DESIGN.md "Resident batches"): the scaled matrix, its
    lambda_max, the panels and the captured graphs stay on the GPU between solve() calls.  Raises RuntimeError with the library's
    message where the C call fails (creation without a GPU, a refused solve); a refused solve leaves the solver usable."""

    _INFO = ("m", "n", "solves", "Bp", "Bc", "graph_captures", "graphs_alive", "panel_allocations")
    _SECONDS = ("create_setup", "create_power", "prep", "upload", "loop", "results")

    _TRANSFER = ("staged_h2d_bytes", "staged_d2h_bytes", "device_entry", "device_solves")

    def __init__(self, model, param=None):
        self.model = model
        cp = (param or Parameters(use_presolve=False)).to_c()
        self.device_number = int(cp.device_number)
        self._last_B = 0
        self._h = lib().hprlp_batched_solver_create(model._ptr, C.byref(cp))
        if not self._h:
            raise RuntimeError("hprlp_batched_solver_create failed: " + last_error())

    def solve(self, Cmat, AL, AU, l, u, obj_constants=None, X0=None, Y0=None, carry=False, param=None, eps_primal=None,
              eps_dual=None):
        """One batch, arguments and result as solve_batched_warm() (param None: the constructor's).  carry=True: every member
        starts from the previous solve()'s solution of the same member, taken from the panels on the GPU (no X0 / Y0, same
        batch size).  X0 / Y0 are checked for shape here and for finite entries by the library."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        B = np.asarray(Cmat).shape[1]
        X0, Y0 = self._start(X0, self.model.n, B, "X0"), self._start(Y0, self.model.m, B, "Y0")
        out = self._host_call("hprlp_batched_solver_solve", (), (_dptr(X0), _dptr(Y0), int(bool(carry))), (Cmat, AL, AU, l, u, obj_constants),
                              param, eps_primal, eps_dual)
        self._last_B = B
        return out

    @staticmethod
    def _start(V, rows, B, name):
        """A start panel as a column-major float64 array of shape (rows, B) (None stays None); finite entries: by the library."""
        if V is None:
            return None
        a = np.asfortranarray(V, dtype=np.float64)
        if a.shape != (rows, B):
            raise ValueError(f"warm start: {name} must have shape ({rows}, {B}), got {a.shape}")
        return a

    def _host_call(self, entry, before, after, batch, param, eps_primal, eps_dual):
        """One call of a host entry (solve, solve_stream): entry(handle, B, *before, the batch, param, *after, detection,
        certificates, results).  The results as _batched_call()'s dict, with "certificates" where detection is on; RuntimeError
        with the library's message where the call fails."""
        det = _detection_arg(eps_primal, eps_dual)
        cc = CBatchedCertificates()
        cprm = None if param is None else param.to_c()

        def call(B, args, cp):
            res = CBatchedResults()
            rc = getattr(lib(), entry)(self._h, B, *before, *args, None if cprm is None else C.byref(cprm), *after,
                                       C.byref(det) if det is not None else None, C.byref(cc) if det is not None else None, C.byref(res))
            if rc != 0:
                if det is not None:
                    lib().hprlp_free_batched_certificates(C.byref(cc))
                raise RuntimeError(entry + " failed: " + last_error())
            return res
        out = _batched_call(call, self.model, *batch, param)
        if det is not None:
            out["certificates"] = _batched_certificates(cc)
        return out

    _STREAM_INFO = ("count", "width", "loop_iterations", "evaluations", "refill_evaluations", "refills", "refill_passes",
                    "lambda_bumps")

    def solve_stream(self, Cmat, AL, AU, l, u, obj_constants=None, width=64, X0=None, Y0=None, eps_primal=None, eps_dual=None,
                     prm=None, parent=None):
        """N problems through `width` slots (hprlp_batched_solver_solve_stream, DESIGN.md "Streamed batches"): Cmat, l, u (n, N),
        AL, AU (m, N), X0 (n, N) / Y0 (m, N) or None.  A member that ends hands its slot to the next queued problem at the same
        evaluation.  Returns solve()'s dict for the N problems plus "slot", "event_in", "event_out" (the evaluation, loop iteration
        / check_iter, at which each problem entered and left its slot; event_in -1: never started) and, with detection,
        "certificates".  prm None: the constructor's parameters; max_iter, each member's own limit, must be a multiple of
        check_iter.  carry, ray_step() and get_panel() are refused afterwards until the next solve().
        parent (N ints; hprlp_batched_solver_solve_stream_parents, DESIGN.md "Streamed batches", "Parents"): parent[p] == -1 makes
        problem p a root, else 0 <= parent[p] < p and p starts from the x, y that problem parent[p] returned, whatever its status,
        as soon as that problem has ended and a slot is free.  X0 and Y0 then come together or not at all: with them a root starts
        from its own columns, without them it is a cold member; a child ignores its own columns.  Slots without a ready problem
        stand empty (stream_parents_info() counts them).  A problem below a parent whose final evaluation is not finite is ERROR
        with event_in -1.  parent None: the call without parents, untouched."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        _need_stream()
        N = np.asarray(Cmat).shape[1]
        X0, Y0 = self._start(X0, self.model.n, N, "X0"), self._start(Y0, self.model.m, N, "Y0")
        if parent is None:
            out = self._host_call("hprlp_batched_solver_solve_stream", (int(width),), (_dptr(X0), _dptr(Y0)),
                                  (Cmat, AL, AU, l, u, obj_constants), prm, eps_primal, eps_dual)
        else:
            _need_parents()
            par = _parent_array(parent, N)
            out = self._host_call("hprlp_batched_solver_solve_stream_parents", (int(width),),
                                  (_dptr(X0), _dptr(Y0), par.ctypes.data_as(c_int_p)), (Cmat, AL, AU, l, u, obj_constants), prm, eps_primal,
                                  eps_dual)
        rec = [np.zeros(N, dtype=np.intc) for _ in range(3)]
        if lib().hprlp_batched_solver_stream_record(self._h, *(r.ctypes.data_as(c_int_p) for r in rec)) != N:
            raise RuntimeError("hprlp_batched_solver_stream_record failed: " + last_error())
        out["slot"], out["event_in"], out["event_out"] = rec
        return out

    def stream_info(self):
        """The counts of the last solve_stream(): count, width, loop_iterations (of the call), evaluations, refill_evaluations (those
        at which a slot was refilled), refills (entries after the initial fill), refill_passes (iteration-0 evaluation passes added
        for refills, cascades included), lambda_bumps."""
        _need_stream()
        out = (C.c_long * 8)()
        if lib().hprlp_batched_solver_stream_info(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(zip(self._STREAM_INFO, [int(v) for v in out]))

    _STREAM_PARENTS_INFO = ("roots", "cold_members", "children_started", "idle_slot_events")

    def stream_parents_info(self):
        """The counts of the last solve_stream() / solve_stream_tensors() with parents (hprlp_batched_solver_stream_parents_info):
        roots that entered, cold_members among them, children_started, and idle_slot_events -- summed over the evaluations after
        which the loop went on, the slots that stood empty while a problem was still waiting for its parent.  RuntimeError where
        the last stream call had no parents."""
        _need_parents()
        out = (C.c_long * 4)()
        if lib().hprlp_batched_solver_stream_parents_info(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(zip(self._STREAM_PARENTS_INFO, [int(v) for v in out]))

    def stream_seconds(self):
        """Wall seconds of the last solve_stream()'s loop: its refill passes (harvest, refill, the new members' evaluation), the rest."""
        _need_stream()
        out = (C.c_double * 2)()
        if lib().hprlp_batched_solver_stream_seconds(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(refill_passes=float(out[0]), rest=float(out[1]))

    def lambda_max(self):
        """(lambda_max as created, lambda_max at the end of the last successful solve() / solve_tensors() / solve_stream()): they
        differ where the call raised it (weighted norm)."""
        _need_stream()
        out = (C.c_double * 2)()
        if lib().hprlp_batched_solver_lambda(self._h, out) != 0:
            raise RuntimeError(last_error())
        return float(out[0]), float(out[1])

    def solve_tensors(self, Cmat, AL, AU, l, u, obj_constants=None, X0=None, Y0=None, carry=False, param=None, eps_primal=None,
                      eps_dual=None):
        """solve() for a batch that is on the GPU already (hprlp_batched_solver_solve_device, DESIGN.md "Device-resident batches"):
        Cmat, l, u, X0 (n, B) and AL, AU, Y0 (m, B) are float64 torch tensors on the solver's device.  A tensor whose transpose is
        contiguous (strides (1, rows)) is passed as it is; any other layout costs one copy on the device.  Returns the dict of
        solve() with x, y, z as torch tensors (rows, B) on the device -- views of fresh (B, rows) buffers -- and the per-member
        scalars and statuses on the host as before.  The inputs are taken as ordered on the current torch stream.  ValueError for a
        wrong type, dtype, device or shape, before the library is called; RuntimeError with the library's message for a call it
        refuses, which leaves the solver usable.  The norms of the scaling follow the tree rule (see set_norms)."""
        out = self._device_call("solve_tensors", "hprlp_batched_solver_solve_device", (), (int(bool(carry)),),
                                (Cmat, AL, AU, l, u, obj_constants, X0, Y0), param, eps_primal, eps_dual)
        self._last_B = out["batch_size"]
        return out

    def _device_call(self, who, entry, before, after, batch, param, eps_primal, eps_dual):
        """One call of a device entry (solve_tensors, solve_stream_tensors): entry(handle, B, *before, the five tensors,
        obj_constants, param, X0, Y0, *after, detection, certificates, the torch stream, x, y, z, the scalars).  The tensors are
        checked here, before the library is called (ValueError); RuntimeError with the library's message where the call fails."""
        import torch
        Cmat, AL, AU, l, u, obj_constants, X0, Y0 = batch
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        m, n = self.model.m, self.model.n
        if not isinstance(Cmat, torch.Tensor) or Cmat.dim() != 2:
            raise ValueError(f"{who}: Cmat must be a 2-D torch tensor")
        B = int(Cmat.shape[1])
        if B <= 0:
            raise ValueError(f"{who}: an empty batch")

        def dev(t, rows, name):
            """The tensor as column-major rows x B device memory: (what keeps it alive, its address)."""
            if t is None:
                return None, None
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
            if t.dtype != torch.float64:
                raise ValueError(f"{who}: {name} must be float64, got {t.dtype}")
            if t.device.type != "cuda" or t.device.index != self.device_number:
                raise ValueError(f"{who}: {name} must be on the solver's device cuda:{self.device_number}, got {t.device}")
            if tuple(t.shape) != (rows, B):
                raise ValueError(f"{who}: {name} must have shape ({rows}, {B}), got {tuple(t.shape)}")
            tt = t.T
            if not tt.is_contiguous():
                tt = tt.contiguous()
            return tt, tt.data_ptr()
        keep = [dev(t, rows, name) for t, rows, name in ((Cmat, n, "Cmat"), (AL, m, "AL"), (AU, m, "AU"), (l, n, "l"), (u, n, "u"),
                                                         (X0, n, "X0"), (Y0, m, "Y0"))]
        oc = None if obj_constants is None else _as(obj_constants, np.float64)
        if oc is not None and oc.shape != (B,):
            raise ValueError(f"{who}: obj_constants must have {B} entries")
        det = _detection_arg(eps_primal, eps_dual)
        cc = CBatchedCertificates()
        cprm = None if param is None else param.to_c()
        device = torch.device("cuda", self.device_number)
        xb, yb, zb = (torch.empty((B, rows), dtype=torch.float64, device=device) for rows in (n, m, n))
        res = dict(primal_obj=np.zeros(B), residuals=np.zeros(B), gap=np.zeros(B), iter=np.zeros(B, dtype=np.intc))
        status = C.create_string_buffer(64 * B)
        sc = CBatchedScalars(primal_obj=_dptr(res["primal_obj"]), residuals=_dptr(res["residuals"]), gap=_dptr(res["gap"]),
                             iter=res["iter"].ctypes.data_as(c_int_p), status=C.cast(status, C.POINTER(C.c_char)))
        stream = torch.cuda.current_stream(device).cuda_stream
        ptrs = [p for _, p in keep]
        rc = getattr(lib(), entry)(self._h, B, *before, *ptrs[:5], _dptr(oc), None if cprm is None else C.byref(cprm), ptrs[5], ptrs[6],
                                   *after, C.byref(det) if det is not None else None, C.byref(cc) if det is not None else None, stream,
                                   xb.data_ptr(), yb.data_ptr(), zb.data_ptr(), C.byref(sc))
        if rc != 0:
            if det is not None:
                lib().hprlp_free_batched_certificates(C.byref(cc))
            raise RuntimeError(entry + " failed: " + last_error())
        out = dict(batch_size=B, time=sc.time, setup_time=sc.setup_time, solve_time=sc.solve_time, power_time=sc.power_time,
                   x=xb.T, y=yb.T, z=zb.T, **res)
        out["status"] = [status.raw[64 * k:64 * (k + 1)].split(b"\0")[0].decode() for k in range(B)]
        if det is not None:
            out["certificates"] = _batched_certificates(cc)
        return out

    def solve_stream_tensors(self, Cmat, AL, AU, l, u, obj_constants=None, width=64, X0=None, Y0=None, eps_primal=None, eps_dual=None,
                             prm=None, parent=None):
        """solve_stream() for a queue that is on the GPU already (hprlp_batched_solver_solve_stream_device, DESIGN.md
        "Device-resident streams"): Cmat, l, u, X0 (n, N) and AL, AU, Y0 (m, N) are float64 torch tensors on the solver's device,
        taken as ordered on the current torch stream.  A tensor whose transpose is contiguous is passed as it is; any other layout
        costs one copy on the device.  The queue is not copied: its norms are taken where it lies and a problem is scaled on its
        way into a slot.  Returns solve_stream()'s dict with x, y, z as device tensors (rows, N) -- a problem that never started
        has zero columns -- plus "slot", "event_in", "event_out" and, with detection, "certificates".  ValueError for a numpy array,
        a CPU tensor, a wrong dtype or a wrong shape, before the library is called; RuntimeError with the library's message for a
        call it refuses, which leaves the solver as it was.
        parent (N ints on the host; hprlp_batched_solver_solve_stream_parents_device): as solve_stream()'s.  A child's start is read
        from the returned x, y on the device, where its parent's harvest wrote it: no start crosses the bus.  parent None: the call
        without parents, untouched."""
        if not hasattr(lib(), "hprlp_batched_solver_solve_stream_device"):
            raise RuntimeError(f"{LIB_PATH} has no hprlp_batched_solver_solve_stream_device: a build of an earlier commit (HPRLP_LIB?)")
        if parent is None:
            out = self._device_call("solve_stream_tensors", "hprlp_batched_solver_solve_stream_device", (int(width),), (),
                                    (Cmat, AL, AU, l, u, obj_constants, X0, Y0), prm, eps_primal, eps_dual)
        else:
            _need_parents()
            import torch
            if not isinstance(Cmat, torch.Tensor) or Cmat.dim() != 2:
                raise ValueError("solve_stream_tensors: Cmat must be a 2-D torch tensor")
            par = _parent_array(parent, int(Cmat.shape[1]))
            out = self._device_call("solve_stream_tensors", "hprlp_batched_solver_solve_stream_parents_device", (int(width),),
                                    (par.ctypes.data_as(c_int_p),), (Cmat, AL, AU, l, u, obj_constants, X0, Y0), prm, eps_primal, eps_dual)
        N = out["batch_size"]
        rec = [np.zeros(N, dtype=np.intc) for _ in range(3)]
        if lib().hprlp_batched_solver_stream_record(self._h, *(r.ctypes.data_as(c_int_p) for r in rec)) != N:
            raise RuntimeError("hprlp_batched_solver_stream_record failed: " + last_error())
        out["slot"], out["event_in"], out["event_out"] = rec
        return out

    _STREAM_MEMORY = ("queue_vector_bytes", "result_block_bytes", "scalar_table_bytes", "pinned_host_bytes")

    def stream_memory(self):
        """What the last successful solve_stream() / solve_stream_tensors() held beside the workspace
        (hprlp_batched_solver_stream_memory): device bytes of queue vectors (the staged queue; 0 for solve_stream_tensors), of
        the result / ray block, of per-problem scalars, partials and tables, and pinned host bytes.  A list in that order."""
        out = (C.c_long * 4)()
        if lib().hprlp_batched_solver_stream_memory(self._h, out) != 0:
            raise RuntimeError(last_error())
        return [int(v) for v in out]

    def set_matrix(self, values):
        """New values on the shared matrix' pattern (hprlp_batched_solver_set_matrix_values), in the order of the model's CSR.
        Every later solve() / solve_tensors() gives what a fresh BatchedSolver on the changed model gives; carry is refused
        until the next successful solve.  ValueError for a wrong length, RuntimeError for a call the library refuses."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        v = _as(values, np.float64)
        if v.ndim != 1 or v.shape[0] != self.model.nnz:
            raise ValueError(f"set_matrix: values must have length {self.model.nnz}, got shape {v.shape}")
        if lib().hprlp_batched_solver_set_matrix_values(self._h, _dptr(v), v.shape[0]) != 0:
            raise RuntimeError("hprlp_batched_solver_set_matrix_values failed: " + last_error())

    def set_norms(self, rule):
        """The norm rule of solve() -- the host entry -- on this solver: 0 = the reference's long double sums (the default), 1 = the
        tree rule that solve_tensors() always follows; with 1 the two agree bit for bit."""
        if lib().hprlp_batched_solver_set_norms(self._h, int(rule)) != 0:
            raise RuntimeError(last_error())

    def scalars(self):
        """The BATCH_SCALARS of the last successful solve() / solve_tensors(): a dict of arrays of B."""
        out = np.zeros((len(BATCH_SCALARS), max(self._last_B, 1)))
        B = lib().hprlp_batched_solver_scalars(self._h, _dptr(out))
        if B < 0:
            raise RuntimeError(last_error())
        return dict(zip(BATCH_SCALARS, out.reshape(-1)[:len(BATCH_SCALARS) * B].reshape(len(BATCH_SCALARS), B).copy()))

    RAY_SLOTS = ("DY", "CD", "VY", "WD", "YN", "DN", "DZ", "VZ", "WQ")

    def ray_step(self, active=None, restart=False):
        """One ray test of the detection on the X_bar / Y_bar panels of the last successful solve (hprlp_batched_solver_ray_step),
        for the members with active[k] != 0 (None: all).  restart=True: forgets the stored iterate and only stores the active
        members' X_bar / Y_bar: returns None.  Otherwise a list of B entries: None for a member that was not tested, else the nine
        device scalars by name and the six sums the verdicts are taken from (Solver.ray_step's dict)."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        B = self._last_B
        act = np.ones(B, dtype=np.intc) if active is None else np.ascontiguousarray(active, dtype=np.intc)
        if act.shape != (B,):
            raise ValueError(f"ray_step: active must have {B} entries, got shape {act.shape}")
        out, tested = np.zeros((9, max(B, 1))), np.zeros(max(B, 1), dtype=np.intc)
        rc = lib().hprlp_batched_solver_ray_step(self._h, act.ctypes.data_as(c_int_p), int(bool(restart)), _dptr(out),
                                                 tested.ctypes.data_as(c_int_p))
        if rc < 0:
            raise RuntimeError("hprlp_batched_solver_ray_step failed: " + last_error())
        if rc == 0:
            return None
        res = []
        for k in range(B):
            if not tested[k]:
                res.append(None)
                continue
            s = dict(zip(self.RAY_SLOTS, (float(v) for v in out[:, k])))
            s.update(D=s["DY"] + s["DZ"], V=max(s["VY"], s["VZ"]), cd=s["CD"], W=max(s["WD"], s["WQ"]), yn=s["YN"], dn=s["DN"])
            res.append(s)
        return res

    def get_panel(self, name):
        """A panel of the last successful solve by name (hprlp_batched_solver_get_panel), scaled units: (rows, B) for C, AL, AU, L,
        U, X_bar, Y_bar, ray_d, ray_y, ray_prev_x, ray_prev_y, ray_z, and (read only: what a warm start seeds and forms) X, X_hat,
        last_X, Y, last_Y, Z_bar, Y_obj; a vector for row_norm / col_norm; "raw:" + name: the padded panel as the device holds
        it, flat (element (i, k) at ((k // Bc) * rows + i) * Bc + k % Bc, see info())."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        nm = name.encode()
        count = lib().hprlp_batched_solver_get_panel(self._h, nm, None, 0)
        if count < 0:
            raise RuntimeError("hprlp_batched_solver_get_panel failed: " + last_error())
        out = np.zeros(max(count, 1))
        if lib().hprlp_batched_solver_get_panel(self._h, nm, _dptr(out), count) != count:
            raise RuntimeError("hprlp_batched_solver_get_panel failed: " + last_error())
        out = out[:count]
        if name in ("row_norm", "col_norm") or name.startswith("raw:"):
            return out
        return out.reshape(self._last_B, -1).T

    def set_panel(self, name, values):
        """X_bar or Y_bar of the last successful solve from a (rows, B) array in scaled units (hprlp_batched_solver_set_panel);
        carry=True is refused afterwards until the next successful solve."""
        if not self._h:
            raise RuntimeError("BatchedSolver: closed")
        a = np.asfortranarray(values, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != self._last_B:
            raise ValueError(f"set_panel: values must have shape (rows, {self._last_B}), got {a.shape}")
        if lib().hprlp_batched_solver_set_panel(self._h, name.encode(), a.ctypes.data_as(c_dbl_p), a.size) != 0:
            raise RuntimeError("hprlp_batched_solver_set_panel failed: " + last_error())

    def transfer(self):
        """The last successful call's staging traffic in bytes, host to device and back (the batch's way in and the solution's way
        out; not the loop's scalar fetches), whether it was a solve_tensors() call, and how many of those there have been."""
        out = (C.c_long * 4)()
        if lib().hprlp_batched_solver_transfer(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(zip(self._TRANSFER, [int(v) for v in out]))

    def info(self):
        out = (C.c_long * 8)()
        if lib().hprlp_batched_solver_info(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(zip(self._INFO, [int(v) for v in out]))

    def seconds(self):
        out = (C.c_double * 6)()
        if lib().hprlp_batched_solver_seconds(self._h, out) != 0:
            raise RuntimeError(last_error())
        return dict(zip(self._SECONDS, [float(v) for v in out]))

    def close(self):
        if self._h:
            lib().hprlp_batched_solver_destroy(self._h)
            self._h = None


def stream_schedule(events, width, parent=None):
    """The schedule BatchedSolver.solve_stream() follows (hprlp_stream_schedule_host; host only, no GPU), from each problem's
    length in evaluations (iter // check_iter; 0: it ends at its iteration-0 evaluation): (slot, event_in, event_out), arrays of
    len(events).  The makespan in evaluations is event_out.max().  parent (len(events) ints, -1 for a root; DESIGN.md "Streamed
    batches", "Parents"): the schedule of solve_stream(..., parent=parent) (hprlp_stream_schedule_parents_host); all -1 gives what
    None gives.  ValueError for what the library refuses."""
    _need_stream()
    ev = np.ascontiguousarray(events, dtype=np.intc)
    if ev.ndim != 1:
        raise ValueError("stream_schedule: events must be one-dimensional")
    out = [np.zeros(max(ev.shape[0], 1), dtype=np.intc) for _ in range(3)]
    if parent is not None:
        _need_parents()
        par = _parent_array(parent, ev.shape[0])
        rc = lib().hprlp_stream_schedule_parents_host(ev.shape[0], int(width), ev.ctypes.data_as(c_int_p), par.ctypes.data_as(c_int_p),
                                                      *(o.ctypes.data_as(c_int_p) for o in out))
        if rc < 0:
            raise ValueError("hprlp_stream_schedule_parents_host: " + last_error())
        return tuple(o[:ev.shape[0]] for o in out)
    rc = lib().hprlp_stream_schedule_host(ev.shape[0], int(width), ev.ctypes.data_as(c_int_p), *(o.ctypes.data_as(c_int_p) for o in out))
    if rc < 0:
        raise ValueError("hprlp_stream_schedule_host: " + last_error())
    return tuple(o[:ev.shape[0]] for o in out)


def _batched_call(fn, model, Cmat, AL, AU, l, u, obj_constants, param):
    """fn(B, (C, AL, AU, l, u, obj_constants) as pointers, CParameters) -> HPRLP_batched_results, as a dict of arrays."""
    Cmat = np.asfortranarray(Cmat, dtype=np.float64)
    B = Cmat.shape[1]
    F = lambda a: np.asfortranarray(a, dtype=np.float64)
    AL, AU, l, u = F(AL), F(AU), F(l), F(u)
    P = lambda a: a.ctypes.data_as(c_dbl_p)
    oc = None if obj_constants is None else _as(obj_constants, np.float64)
    cp = (param or Parameters()).to_c()
    res = fn(B, (P(Cmat), P(AL), P(AU), P(l), P(u), None if oc is None else P(oc)), cp)
    m, n = model.m, model.n
    g = lambda q, k: None if not q else np.ctypeslib.as_array(q, shape=(k,)).copy()
    out = dict(batch_size=res.batch_size, time=res.time, setup_time=res.setup_time, solve_time=res.solve_time,
               power_time=res.power_time)
    out["x"] = None if not res.x else g(res.x, n * B).reshape(B, n).T
    out["y"] = None if not res.y else g(res.y, m * B).reshape(B, m).T
    out["z"] = None if not res.z else g(res.z, n * B).reshape(B, n).T
    out["primal_obj"] = g(res.primal_obj, B); out["residuals"] = g(res.residuals, B); out["gap"] = g(res.gap, B)
    out["iter"] = None if not res.iter else np.ctypeslib.as_array(res.iter, shape=(B,)).copy()
    raw = C.string_at(res.status, 64 * res.batch_size) if res.status else b""
    out["status"] = [raw[64 * k:64 * (k + 1)].split(b"\0")[0].decode() for k in range(res.batch_size if raw else 0)]
    lib().free_batched_results(C.byref(res))
    return out


class CFormBuilt(C.Structure):  # include/hprlp_amd.h: hprlp_form_built
    _fields_ = [("ok", C.c_long), ("n_pieces", C.c_long), ("dense_entries", C.c_long), ("n_rem", C.c_long), ("rem_top_share", C.c_double)]


class CFormFacts(C.Structure):  # hprlp_form_facts
    _fields_ = [("rows", C.c_long), ("cols", C.c_long), ("nnz", C.c_long), ("longest_row", C.c_long), ("long_row_share", C.c_double),
                ("line_density", C.c_double), ("xcd_gather_bytes", C.c_double), ("sb_rows", C.c_long), ("slots", C.c_long),
                ("min_dense_override", C.c_double), ("sharded", C.c_long), ("heaviest_block", C.c_long), ("tiling_share", C.c_double),
                ("n_long_rows", C.c_long), ("long_rows_nnz", C.c_long), ("side", CFormBuilt), ("whole", CFormBuilt),
                ("popular_share", C.c_double), ("heaviest_pb_block", C.c_long)]


class CFormHookValue(C.Structure):
    _fields_ = [("set", C.c_int), ("value", C.c_double)]


class CFormHooks(C.Structure):  # hprlp_form_hooks
    _fields_ = [(k, C.c_int) for k in ("no_tiled", "tiled_anyway", "pieces_anyway", "host_tiling", "no_long_side", "no_pb_fallback",
                                       "no_pb_long_rows", "no_pb_kernel", "tiling_check")] + \
               [(k, CFormHookValue) for k in ("tiled_min_rows", "tiled_min_dense", "tiled_min_cols", "pb_min_cols", "pb_min_nnz",
                                              "tile_rows", "tile_cols")]


class CFormDecision(C.Structure):  # hprlp_form_decision
    _fields_ = [("min_rows", C.c_int), ("min_cols", C.c_int), ("min_dense", C.c_double), ("route", C.c_int), ("side_tried", C.c_int),
                ("kept", C.c_int), ("form", C.c_int), ("why", C.c_int), ("long_rows_alone", C.c_int), ("all_remainder_wanted", C.c_int),
                ("note", C.c_char * 96)]


FORM_NAMES = ("stream", "fused", "pieces", "all-remainder")
BLANK_FORM_FACTS = dict(rows=0, cols=0, nnz=0, longest_row=0, long_row_share=0.0, line_density=1.0, xcd_gather_bytes=0.0, sb_rows=8192,
                        slots=512, min_dense_override=-1.0, sharded=0, heaviest_block=-1, tiling_share=-1.0, n_long_rows=-1,
                        long_rows_nnz=-1, side=dict(ok=-1, n_pieces=0, dense_entries=0, n_rem=0, rem_top_share=0.0),
                        whole=dict(ok=-1, n_pieces=0, dense_entries=0, n_rem=0, rem_top_share=0.0), popular_share=-1.0,
                        heaviest_pb_block=-1)


def _struct_dict(s):
    return {k: (_struct_dict(getattr(s, k)) if isinstance(getattr(s, k), C.Structure) else getattr(s, k)) for k, _ in s._fields_}


def form_select(facts, hooks=None):
    """Host only (hprlp_form_select): the staged decisions of the kernel-form selection for a facts record (a dict with the fields
    of hprlp_form_facts; missing ones as in BLANK_FORM_FACTS) under test hooks {name: True or value}.  Returns a dict with
    min_rows, min_cols, min_dense, route, side_tried, kept, form (a FORM_NAMES entry), why, long_rows_alone, all_remainder_wanted, note."""
    f = CFormFacts()
    for k, v in dict(BLANK_FORM_FACTS, **facts).items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                setattr(getattr(f, k), kk, vv)
        else:
            setattr(f, k, v)
    h = CFormHooks()
    for k, v in (hooks or {}).items():
        if isinstance(getattr(h, k), CFormHookValue):
            getattr(h, k).set, getattr(h, k).value = 1, float(v)
        else:
            setattr(h, k, int(v))
    d = CFormDecision()
    L = lib()
    L.hprlp_form_select.argtypes = [C.POINTER(CFormFacts), C.POINTER(CFormHooks), C.POINTER(CFormDecision)]
    if L.hprlp_form_select(C.byref(f), C.byref(h), C.byref(d)) != 0:
        raise RuntimeError(L.hprlp_last_error().decode())
    out = _struct_dict(d)
    out["note"] = out["note"].decode()
    out["form"] = FORM_NAMES[out["form"]]
    return out


class CBatchedPrepared(C.Structure):  # include/hprlp_amd.h: hprlp_batched_prepared
    _fields_ = [(k, c_dbl_p) for k in ("C", "AL", "AU", "l", "u", "scalars", "X0", "Y0", "X_back", "Y_back", "z_back")] + \
               [("Bp", C.c_int), ("Bc", C.c_int), ("pad", C.c_double), ("panel", c_dbl_p), ("panel_back", c_dbl_p),
                ("panel_index", C.POINTER(C.c_long))]


BATCH_SCALARS = ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org", "sigma")
NORM_SEG, NORM_LANES = 16384, 256  # the tree rule's constants (csrc/batch_prep.h: kNormSeg, kNormLanes)


def batched_prepare_host(rn, cn, Cmat, AL, AU, l, u, X0=None, Y0=None, use_bc_scaling=True, pad=0.0, norm_rule=0):
    """Host only (hprlp_batched_prepare_host): what solve_batched does to a batch's vectors before anything is uploaded.  rn (m) /
    cn (n): the shared matrix' row / column scaling; Cmat, l, u, X0: (n, B); AL, AU, Y0: (m, B).  Returns a dict: the scaled C, AL,
    AU, l, u; the BATCH_SCALARS (B each); X0, Y0 scaled and X_back, Y_back mapped back as a solution is (None without a start);
    z_back (the scaled C mapped as a solution's z); Bp, Bc; panel (the scaled C as a device panel, flat, padding = pad),
    panel_back (n, B) and panel_index (n, B).  norm_rule: 0 = the reference's long double sums, non-zero = that rule of
    hprlp_batched_prepare_host_rule (1: the tree rule of the device entry, NORM_SEG / NORM_LANES)."""
    F = lambda a: None if a is None else np.asfortranarray(a, dtype=np.float64)
    rn, cn = _as(rn, np.float64), _as(cn, np.float64)
    m, n, B = len(rn), len(cn), np.asarray(Cmat).shape[1]
    ins = [F(a) for a in (Cmat, AL, AU, l, u, X0, Y0)]
    for a, rows in zip(ins, (n, m, m, n, n, n, m)):
        if a is not None and a.shape != (rows, B):
            raise ValueError("batched_prepare_host: an array of shape %s where (%d, %d) is expected" % (a.shape, rows, B))
    Bp = (B + 63) // 64 * 64  # room for any padding: the library's Bp is at most the next multiple of 64
    new = lambda rows, cols=B: np.zeros((rows, cols), order="F")
    out = dict(C=new(n), AL=new(m), AU=new(m), l=new(n), u=new(n), scalars=np.zeros((7, B)),
               X0=None if X0 is None else new(n), Y0=None if Y0 is None else new(m),
               X_back=None if X0 is None else new(n), Y_back=None if Y0 is None else new(m), z_back=new(n),
               panel=np.zeros(n * Bp), panel_back=new(n), panel_index=np.zeros((n, B), dtype=np.int64, order="F"))
    P = lambda a: None if a is None else a.ctypes.data_as(c_dbl_p)
    o = CBatchedPrepared(pad=pad, **{k: (v.ctypes.data_as(C.POINTER(C.c_long)) if k == "panel_index" else P(v)) for k, v in out.items()})
    L = lib()
    L.hprlp_batched_prepare_host.argtypes = [C.c_int] * 3 + [c_dbl_p] * 9 + [C.c_int, C.POINTER(CBatchedPrepared)]
    if norm_rule:
        rc = L.hprlp_batched_prepare_host_rule(m, n, B, P(rn), P(cn), *[P(a) for a in ins], int(use_bc_scaling), int(norm_rule), C.byref(o))
    else:
        rc = L.hprlp_batched_prepare_host(m, n, B, P(rn), P(cn), *[P(a) for a in ins], int(use_bc_scaling), C.byref(o))
    if rc != 0:
        raise RuntimeError(L.hprlp_last_error().decode())
    out.update(Bp=o.Bp, Bc=o.Bc, panel=out["panel"][:n * o.Bp])
    out.update(zip(BATCH_SCALARS, out.pop("scalars")))
    return out


def value_maps_host(m, n, rowptr, colind, row_new2old=None, col_new2old=None):
    """Host only (hprlp_value_maps_host): (mapA, mapAT) of a CSR pattern under a locality ordering, or under none -- the rule
    of Solver.value_maps() restated without a GPU."""
    rp, ci = _as(rowptr, np.int32), _as(colind, np.int32)
    if rp.ndim != 1 or rp.shape[0] != m + 1:
        raise ValueError(f"value_maps_host: rowptr must have length {m + 1}, got shape {rp.shape}")
    nnz = int(rp[m])
    if ci.ndim != 1 or ci.shape[0] != nnz:
        raise ValueError(f"value_maps_host: colind must have length {nnz}, got shape {ci.shape}")
    if (row_new2old is None) != (col_new2old is None):
        raise ValueError("value_maps_host: both permutations or neither")
    pr = pc = None
    if row_new2old is not None:
        pr, pc = _as(row_new2old, np.int32), _as(col_new2old, np.int32)
        if pr.shape != (m,) or pc.shape != (n,):
            raise ValueError(f"value_maps_host: the permutations must have length {m} and {n}")
    ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)
    a, t = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.int32)
    if lib().hprlp_value_maps_host(m, n, ip(rp), ip(ci), ip(pr), ip(pc), ip(a), ip(t)) != 0:
        raise RuntimeError(last_error())
    return a[:nnz].copy(), t[:nnz].copy()


def _pattern(what, m, n, rowptr, colind):
    rp, ci = _as(rowptr, np.int32), _as(colind, np.int32)
    if rp.ndim != 1 or rp.shape[0] != m + 1:
        raise ValueError(f"{what}: rowptr must have length {m + 1}, got shape {rp.shape}")
    if ci.ndim != 1 or ci.shape[0] != int(rp[m]):
        raise ValueError(f"{what}: colind must have length {int(rp[m])}, got shape {ci.shape}")
    return rp, ci


def _perms(what, m, n, row_new2old, col_new2old):
    if (row_new2old is None) != (col_new2old is None):
        raise ValueError(f"{what}: both permutations or neither")
    if row_new2old is None:
        return None, None
    pr, pc = _as(row_new2old, np.int32), _as(col_new2old, np.int32)
    if pr.shape != (m,) or pc.shape != (n,):
        raise ValueError(f"{what}: the permutations must have length {m} and {n}")
    return pr, pc


def reorder_steps(m, n, rowptr, colind, device=False, sweeps=3):
    """Test infrastructure (hprlp_reorder_steps): the locality ordering step by step on the host or on the device, without the
    acceptance gates.  Returns a dict: lab_r / lab_c (labels after the majority rounds, -1 = unlabelled), pos0_r / pos0_c (cluster
    positions), pos_r / pos_c (after the sweeps), row_new2old / col_new2old, clusters, components, bfs_levels, share_before,
    share_after."""
    rp, ci = _pattern("reorder_steps", m, n, rowptr, colind)
    L = lib()
    L.hprlp_reorder_steps.argtypes = [C.c_int, C.c_int, c_int_p, c_int_p, C.c_int, C.c_int, c_int_p, c_int_p] + [c_dbl_p] * 4 + \
        [c_int_p, c_int_p, c_dbl_p]
    out = dict(lab_r=np.zeros(m, np.int32), lab_c=np.zeros(n, np.int32), pos0_r=np.zeros(m), pos0_c=np.zeros(n), pos_r=np.zeros(m),
               pos_c=np.zeros(n), row_new2old=np.zeros(m, np.int32), col_new2old=np.zeros(n, np.int32))
    stats = np.zeros(5)
    ptr = lambda a: a.ctypes.data_as(c_int_p if a.dtype == np.int32 else c_dbl_p)
    if L.hprlp_reorder_steps(m, n, ptr(rp), ptr(ci), int(bool(device)), int(sweeps), *[ptr(out[k]) for k in out], ptr(stats)) != 0:
        raise RuntimeError(last_error())
    out.update(clusters=int(stats[0]), components=int(stats[1]), bfs_levels=int(stats[2]), share_before=float(stats[3]),
               share_after=float(stats[4]))
    return out


def permute_csr_device(m, n, rowptr, colind, values, row_new2old, col_new2old):
    """Test infrastructure (hprlp_permute_csr_device): (rowptr, colind, values) of P A Q as a solver's set-up forms it on the device."""
    rp, ci = _pattern("permute_csr_device", m, n, rowptr, colind)
    v = _as(values, np.float64)
    if v.shape != ci.shape:
        raise ValueError("permute_csr_device: one value per entry")
    pr, pc = _perms("permute_csr_device", m, n, row_new2old, col_new2old)
    if pr is None:
        raise ValueError("permute_csr_device: the permutations are required")
    L = lib()
    L.hprlp_permute_csr_device.argtypes = [C.c_int, C.c_int, c_int_p, c_int_p, c_dbl_p, c_int_p, c_int_p, c_int_p, c_int_p, c_dbl_p]
    orp, oci, ov = np.zeros(m + 1, np.int32), np.zeros(len(ci), np.int32), np.zeros(len(ci))
    ip = lambda a: a.ctypes.data_as(c_int_p)
    if L.hprlp_permute_csr_device(m, n, ip(rp), ip(ci), v.ctypes.data_as(c_dbl_p), ip(pr), ip(pc), ip(orp), ip(oci),
                                  ov.ctypes.data_as(c_dbl_p)) != 0:
        raise RuntimeError(last_error())
    return orp, oci, ov


def tiling_share(m, n, rowptr, colind, row_new2old=None, col_new2old=None, device=False):
    """Test infrastructure (hprlp_tiling_share): the tiling test of a pattern as given or permuted, host or device form."""
    rp, ci = _pattern("tiling_share", m, n, rowptr, colind)
    pr, pc = _perms("tiling_share", m, n, row_new2old, col_new2old)
    L = lib()
    L.hprlp_tiling_share.argtypes = [C.c_int, C.c_int] + [c_int_p] * 4 + [C.c_int, c_dbl_p]
    ip = lambda a: None if a is None else a.ctypes.data_as(c_int_p)
    out = C.c_double(0.0)
    if L.hprlp_tiling_share(m, n, ip(rp), ip(ci), ip(pr), ip(pc), int(bool(device)), C.byref(out)) != 0:
        raise RuntimeError(last_error())
    return out.value


class Solver:
    """Step-level handle (include/hprlp_amd.h) used by the parity tests and bench.py."""

    def __init__(self, model, param=None):
        cp = (param or Parameters()).to_c()
        self.model = model
        self.device_number = int(cp.device_number)
        self.h = lib().hprlp_solver_create(model._ptr, C.byref(cp))
        if not self.h:
            raise RuntimeError("hprlp_solver_create failed: " + last_error())

    @classmethod
    def create_many(cls, models, param=None):
        """Solver(model, param) for every model, set up together (hprlp_solver_create_many): one arena, one stream and one copy per
        arena block for the Netlib-scale members.  Returns a list with None where a model failed (last_error() names it)."""
        models = list(models)
        cp = (param or Parameters()).to_c()
        ptrs = (C.POINTER(CLPInfo) * max(len(models), 1))(*[mod._ptr for mod in models])
        hs = (C.c_void_p * max(len(models), 1))()
        if lib().hprlp_solver_create_many(ptrs, len(models), C.byref(cp), hs) < 0:
            raise RuntimeError(last_error())
        out = []
        for k, mod in enumerate(models):
            if not hs[k]:
                out.append(None)
                continue
            sv = cls.__new__(cls)
            sv.model = mod
            sv.device_number = int(cp.device_number)
            sv.h = hs[k]
            out.append(sv)
        return out

    @staticmethod
    def scale_many(solvers):
        """scale() of every solver, one launch per kernel kind and scaling step for the small-path members
        (hprlp_solver_scale_many)."""
        solvers, hs = Solver._handles(solvers)
        if lib().hprlp_solver_scale_many(hs, len(solvers)) < 0:
            raise RuntimeError(last_error())

    @staticmethod
    def close_many(solvers):
        """close() of every solver that is not None (hprlp_solver_destroy_many)."""
        solvers = [sv for sv in solvers if sv is not None and sv.h]
        if not solvers:
            return
        _, hs = Solver._handles(solvers)
        lib().hprlp_solver_destroy_many(hs, len(solvers))
        for sv in solvers:
            sv.h = None

    @classmethod
    def create_dist(cls, model, param, rank, size, unique_id=None):
        """One rank of the row-partitioned solve (hprlp_solver_create_dist).  unique_id: 128-byte numpy
        uint8 array from dist_unique_id() (rank 0) broadcast to every rank."""
        L = lib()
        L.hprlp_solver_create_dist.restype = C.c_void_p
        L.hprlp_solver_create_dist.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters), C.c_int, C.c_int,
                                               C.c_void_p, C.c_int]
        self = cls.__new__(cls)
        self.model = model
        cp = (param or Parameters()).to_c()
        uid = None if unique_id is None else unique_id.ctypes.data_as(C.c_void_p)
        self.h = L.hprlp_solver_create_dist(model._ptr, C.byref(cp), rank, size, uid, 0 if unique_id is None else len(unique_id))
        if not self.h:
            raise RuntimeError("hprlp_solver_create_dist failed: " + last_error())
        self._set_local_sizes(rank, size)
        return self

    @classmethod
    def create_dist_from_shard(cls, shard, param, rank, size, unique_id=None, group=None):
        """One rank of the row-partitioned solve from a shard assembled by the caller (shard.ShardArrays): no rank holds the
        whole matrix.  group: a local_group() handle runs the ranks as threads of this process (tests) instead of RCCL."""
        L = lib()
        self = cls.__new__(cls)
        self.model = shard            # has .m / .n; keeps the arrays alive until the solver is created
        cp = (param or Parameters()).to_c()
        if group is not None:
            L.hprlp_solver_create_local_from_shard.restype = C.c_void_p
            L.hprlp_solver_create_local_from_shard.argtypes = [C.POINTER(CShard), C.POINTER(CParameters), C.c_int, C.c_int, C.c_void_p]
            self.h = L.hprlp_solver_create_local_from_shard(C.byref(shard.c_shard), C.byref(cp), rank, size, group)
        else:
            L.hprlp_solver_create_dist_from_shard.restype = C.c_void_p
            L.hprlp_solver_create_dist_from_shard.argtypes = [C.POINTER(CShard), C.POINTER(CParameters), C.c_int, C.c_int,
                                                              C.c_void_p, C.c_int]
            uid = None if unique_id is None else unique_id.ctypes.data_as(C.c_void_p)
            self.h = L.hprlp_solver_create_dist_from_shard(C.byref(shard.c_shard), C.byref(cp), rank, size, uid,
                                                           0 if unique_id is None else len(unique_id))
        if not self.h:
            raise RuntimeError("hprlp_solver_create_dist_from_shard failed: " + last_error())
        self.row_off, self.m_loc, self.col_off, self.n_loc = shard.row_off, shard.m_loc, shard.col_off, shard.n_loc
        return self

    def _set_local_sizes(self, rank, size):
        """run()/get() of a sharded solver return this rank's slices: rows [row_off, row_off+m_loc), ..."""
        off, cnt = C.c_int(), C.c_int()
        lib().hprlp_partition(self.model.m, size, rank, C.byref(off), C.byref(cnt))
        self.row_off, self.m_loc = off.value, cnt.value
        lib().hprlp_partition(self.model.n, size, rank, C.byref(off), C.byref(cnt))
        self.col_off, self.n_loc = off.value, cnt.value

    @classmethod
    def create_local(cls, model, param, rank, size, group):
        """Rank `rank` of a `size`-rank solve whose ranks are host threads of this process (hprlp_solver_create_local);
        `group` comes from local_group(size).  Call from the rank's own thread."""
        L = lib()
        L.hprlp_solver_create_local.restype = C.c_void_p
        L.hprlp_solver_create_local.argtypes = [C.POINTER(CLPInfo), C.POINTER(CParameters), C.c_int, C.c_int, C.c_void_p]
        self = cls.__new__(cls)
        self.model = model
        cp = (param or Parameters()).to_c()
        self.h = L.hprlp_solver_create_local(model._ptr, C.byref(cp), rank, size, group)
        if not self.h:
            raise RuntimeError("hprlp_solver_create_local failed: " + last_error())
        self._set_local_sizes(rank, size)
        return self

    @staticmethod
    def local_group(size):
        L = lib()
        L.hprlp_local_group_create.restype = C.c_void_p
        L.hprlp_local_group_create.argtypes = [C.c_int]
        g = L.hprlp_local_group_create(size)
        if not g:
            raise RuntimeError(last_error())
        return C.c_void_p(g)

    @staticmethod
    def free_local_group(group):
        L = lib()
        L.hprlp_local_group_destroy.argtypes = [C.c_void_p]
        L.hprlp_local_group_destroy(group)

    def dist_loopback(self, count=100000):
        L = lib()
        L.hprlp_solver_dist_loopback.argtypes = [C.c_void_p, C.c_int]
        self._chk(L.hprlp_solver_dist_loopback(self.h, int(count)))

    def dist_info(self):
        L = lib()
        L.hprlp_solver_dist_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        out = (C.c_long * 8)()
        self._chk(L.hprlp_solver_dist_info(self.h, out))
        keys = ("m_sparse", "m_sent", "m_received", "n_sparse", "n_sent", "n_received", "m_requests", "n_requests")
        return dict(zip(keys, [int(v) for v in out]))

    def dist_comm_info(self):
        """What the transport reports (RCCL: ncclCommCount / ncclCommUserRank / ncclCommCuDevice) for the main communicator
        and for the exchange stream's own one (ranks 0 if there is none)."""
        L = lib()
        L.hprlp_solver_dist_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        out = (C.c_long * 8)()
        self._chk(L.hprlp_solver_dist_comm_info(self.h, out))
        keys = ("comm_ranks", "comm_rank", "comm_device", "xcomm_ranks", "xcomm_rank", "xcomm_device", "hip_device", "overlap")
        return dict(zip(keys, [int(v) for v in out]))

    @staticmethod
    def dist_unique_id(ids=1):
        """ids=2: a second id for the exchange stream's own communicator (one communicator, one stream)."""
        uid = np.zeros(128 * ids, np.uint8)
        if lib().hprlp_dist_unique_id(uid.ctypes.data_as(C.c_void_p), 128 * ids) != 0:
            raise RuntimeError(last_error())
        return uid

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(last_error())
        return rc

    def close(self):
        if self.h:
            lib().hprlp_solver_destroy(self.h)
            self.h = None

    def scale(self):
        self._chk(lib().hprlp_solver_scale(self.h))

    def power_iteration(self, max_iter=5000, tol=1e-4):
        it = C.c_int(0)
        lam = lib().hprlp_solver_power_iteration(self.h, max_iter, tol, C.byref(it))
        if lam < 0:
            raise RuntimeError(last_error())
        return lam, it.value

    def init(self, sigma=-1.0, lambda_max=1.0):
        self._chk(lib().hprlp_solver_init(self.h, sigma, lambda_max))

    def reset(self):
        """All iterates back to zero (hprlp_solver_reset_iterates); follow with init()."""
        L = lib()
        L.hprlp_solver_reset_iterates.argtypes = [C.c_void_p]
        L.hprlp_solver_reset_iterates.restype = C.c_int
        self._chk(L.hprlp_solver_reset_iterates(self.h))

    def iterate(self, normal, then_check=False):
        self._chk(lib().hprlp_solver_iterate(self.h, int(normal), int(bool(then_check))))

    def residuals(self, it, compute_gap=False):
        out = np.zeros(8)
        self._chk(lib().hprlp_solver_residuals(self.h, int(it), int(bool(compute_gap)), out.ctypes.data_as(c_dbl_p)))
        return dict(zip(("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt", "weighted_norm", "lambda_max"), out))

    def restart(self, current_gap, best_gap, best_sigma, err_Rd, err_Rp, rel_gap):
        a = np.array([current_gap, best_gap, best_sigma, err_Rd, err_Rp, rel_gap], dtype=np.float64)
        s = C.c_double(0)
        self._chk(lib().hprlp_solver_restart(self.h, a.ctypes.data_as(c_dbl_p), C.byref(s)))
        return s.value

    def weighted_norm(self):
        return lib().hprlp_solver_weighted_norm(self.h)

    def get(self, name):
        info = self.info()
        cap = max(info["m"], info["n"], info["nnz"], 1)
        buf = np.zeros(cap)
        k = lib().hprlp_solver_get_vector(self.h, name.encode(), buf.ctypes.data_as(c_dbl_p), cap)
        if k < 0:
            raise RuntimeError(last_error())
        return buf[:k].copy()

    def set(self, name, arr):
        a = _as(arr, np.float64)
        self._chk(lib().hprlp_solver_set_vector(self.h, name.encode(), a.ctypes.data_as(c_dbl_p), len(a)))

    def scalars(self):
        out = np.zeros(16)
        self._chk(lib().hprlp_solver_get_scalars(self.h, out.ctypes.data_as(c_dbl_p)))
        keys = ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org", "sigma", "lambda_max",
                "setup_time", "scaling_time", "power_time", "power_iters", "kx", "ky")
        return dict(zip(keys, out))

    def info(self):
        out = (C.c_long * 8)()
        self._chk(lib().hprlp_solver_info(self.h, out))
        keys = ("m", "n", "nnz", "blocks_A", "blocks_AT", "grid_y", "grid_x", "tiled")
        d = dict(zip(keys, [int(v) for v in out]))
        d["reordered"] = bool(d["tiled"] & 8)  # set-up time locality ordering in place (csrc/reorder.cpp)
        d["tiled"] &= 7
        return d

    def describe(self):
        """Which kernel form runs on A and A^T (hprlp_solver_describe)."""
        buf = C.create_string_buffer(2048)
        L = lib()
        L.hprlp_solver_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        self._chk(L.hprlp_solver_describe(self.h, buf, 2048))
        return buf.value.decode()

    def form_facts(self):
        """The facts the kernel-form rules were asked about (hprlp_solver_form_facts): {"A": [pass, ...], "A^T": [...]}, each
        pass a dict for form_select(); the second pass, where there is one, is the all-remainder request."""
        L = lib()
        L.hprlp_solver_form_facts.argtypes = [C.c_void_p, C.c_int, C.POINTER(CFormFacts)]
        out = {}
        for which, name in enumerate(("A", "A^T")):
            buf = (CFormFacts * 2)()
            n = L.hprlp_solver_form_facts(self.h, which, buf)
            self._chk(min(n, 0))
            out[name] = [_struct_dict(buf[i]) for i in range(n)]
        return out

    def run(self, max_trace=4096):
        res = CResults()
        trace = (CTraceRow * max_trace)()
        nt = C.c_int(0)
        self._chk(lib().hprlp_solver_run(self.h, C.byref(res), trace, max_trace, C.byref(nt)))
        r = Results(res, getattr(self, "m_loc", self.model.m), getattr(self, "n_loc", self.model.n))
        r.trace = [{f: getattr(trace[i], f) for f, _ in CTraceRow._fields_} for i in range(nt.value)]
        return r

    @staticmethod
    def _handles(solvers):
        solvers = list(solvers)
        return solvers, (C.c_void_p * max(len(solvers), 1))(*[sv.h for sv in solvers])

    @staticmethod
    def power_iteration_many(solvers, max_iter=5000, tol=1e-4):
        """power_iteration() of every solver, small-path members in one launch per kernel class, wide members (set_group_wide)
        through group launches of the regular kernels (hprlp_solver_power_iteration_many).  Returns [(lambda, iterations), ...]."""
        solvers, hs = Solver._handles(solvers)
        lam = np.zeros(max(len(solvers), 1))
        its = np.zeros(max(len(solvers), 1), dtype=np.int32)
        if lib().hprlp_solver_power_iteration_many(hs, len(solvers), int(max_iter), float(tol), lam.ctypes.data_as(c_dbl_p),
                                                   its.ctypes.data_as(c_int_p)) < 0:
            raise RuntimeError(last_error())
        return [(float(lam[k]), int(its[k])) for k in range(len(solvers))]

    @staticmethod
    def iterate_many(solvers, normals, then_check=False):
        """iterate(normals[k], then_check) of every solver, the normal iterations of small-path members in one launch per
        kernel class, those of wide members (set_group_wide) in group launches, two per iteration (hprlp_solver_iterate_many)."""
        solvers, hs = Solver._handles(solvers)
        cnt = _as(normals, np.int32)
        if cnt.ndim != 1 or cnt.shape[0] != len(solvers):
            raise ValueError("iterate_many: one iteration count per solver")
        if lib().hprlp_solver_iterate_many(hs, len(solvers), cnt.ctypes.data_as(c_int_p), int(bool(then_check))) < 0:
            raise RuntimeError(last_error())

    @staticmethod
    def residuals_many(solvers, iters, compute_gap):
        """residuals(iters[k], compute_gap[k]) of every solver, one launch per kernel for the members of the group launches
        (hprlp_solver_residuals_many).  Returns a list of dicts."""
        solvers, hs = Solver._handles(solvers)
        it, cg = _as(iters, np.int32), _as([int(bool(v)) for v in compute_gap], np.int32)
        if it.ndim != 1 or it.shape[0] != len(solvers) or cg.shape[0] != len(solvers):
            raise ValueError("residuals_many: one iteration and one flag per solver")
        out = np.zeros(8 * max(len(solvers), 1))
        if lib().hprlp_solver_residuals_many(hs, len(solvers), it.ctypes.data_as(c_int_p), cg.ctypes.data_as(c_int_p),
                                             out.ctypes.data_as(c_dbl_p)) < 0:
            raise RuntimeError(last_error())
        keys = ("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt", "weighted_norm", "lambda_max")
        return [dict(zip(keys, out[8 * k:8 * k + 8])) for k in range(len(solvers))]

    @staticmethod
    def restart_many(solvers, inputs):
        """restart(*inputs[k]) of every solver (hprlp_solver_restart_many); inputs[k] = (current_gap, best_gap, best_sigma,
        err_Rd, err_Rp, rel_gap).  Returns the new sigmas."""
        solvers, hs = Solver._handles(solvers)
        a = np.ascontiguousarray(np.asarray(inputs, dtype=np.float64).reshape(-1))
        if a.shape[0] != 6 * len(solvers):
            raise ValueError("restart_many: six inputs per solver")
        sig = np.zeros(max(len(solvers), 1))
        if lib().hprlp_solver_restart_many(hs, len(solvers), a.ctypes.data_as(c_dbl_p), sig.ctypes.data_as(c_dbl_p)) < 0:
            raise RuntimeError(last_error())
        return [float(v) for v in sig[:len(solvers)]]

    @staticmethod
    def run_many(solvers):
        """run() of every solver in lock-step, from its current state (hprlp_solver_run_many).  Returns a list of Results (no
        trace); certificates come from certificate() of each solver."""
        solvers, hs = Solver._handles(solvers)
        res = (CResults * max(len(solvers), 1))()
        if lib().hprlp_solver_run_many(hs, len(solvers), res) < 0:
            raise RuntimeError(last_error())
        return [Results(res[k], sv.model.m, sv.model.n) for k, sv in enumerate(solvers)]

    def set_group_wide(self, on=True):
        """Let this solver, off the small path, join the group launches of the *_many calls (hprlp_solver_set_group_wide).  True:
        it will join; False: the setting is stored but it cannot (a tiled copy, rows past 4096 entries) and goes its own way.  A
        small-path solver joins anyway (True); a sharded solver raises."""
        return self._chk(lib().hprlp_solver_set_group_wide(self.h, int(bool(on)))) == 1

    def set_detection(self, eps_primal=1e-8, eps_dual=1e-8, on=True):
        """Infeasibility detection for the following run() calls (hprlp_solver_set_detection); on=False switches it off."""
        det = _detection(eps_primal, eps_dual) if on else None
        self._chk(lib().hprlp_solver_set_detection(self.h, C.byref(det) if det is not None else None))

    RAY_SLOTS = ("DY", "CD", "VY", "WD", "YN", "DN", "DZ", "VZ", "WQ")

    def ray_step(self, restart=False):
        """One ray test of the detection on the current x_bar / y_bar (hprlp_solver_ray_step).  None where only the iterate was
        stored (the first step after restart=True), else the nine raw slots (RAY_SLOTS) and the sums the verdict reads, as
        Solver::ray_scalars forms them: D, V, cd, W, yn, dn."""
        out = np.zeros(9)
        if self._chk(lib().hprlp_solver_ray_step(self.h, int(bool(restart)), out.ctypes.data_as(c_dbl_p))) == 0:
            return None
        r = dict(zip(self.RAY_SLOTS, (float(v) for v in out)))
        r.update(D=r["DY"] + r["DZ"], V=max(r["VY"], r["VZ"]), cd=r["CD"], W=max(r["WD"], r["WQ"]), yn=r["YN"], dn=r["DN"])
        return r

    @staticmethod
    def ray_step_many(solvers, restart):
        """ray_step(restart[k]) of every solver with one fetch for the group (hprlp_solver_ray_step_many).  Returns one entry per
        solver: None where only the iterate was stored, else ray_step's dict."""
        solvers, hs = Solver._handles(solvers)
        K = len(solvers)
        flags = np.ascontiguousarray([1 if f else 0 for f in restart], dtype=np.int32)
        if flags.shape[0] != K:
            raise ValueError("ray_step_many: one restart flag per solver")
        out, tested = np.zeros(9 * max(K, 1)), np.zeros(max(K, 1), np.int32)
        if lib().hprlp_solver_ray_step_many(hs, K, flags.ctypes.data_as(c_int_p), out.ctypes.data_as(c_dbl_p), tested.ctypes.data_as(c_int_p)) < 0:
            raise RuntimeError(last_error())
        res = []
        for k in range(K):
            if not tested[k]:
                res.append(None)
                continue
            r = dict(zip(Solver.RAY_SLOTS, (float(v) for v in out[9 * k:9 * k + 9])))
            r.update(D=r["DY"] + r["DZ"], V=max(r["VY"], r["VZ"]), cd=r["CD"], W=max(r["WD"], r["WQ"]), yn=r["YN"], dn=r["DN"])
            res.append(r)
        return res

    def set_start(self, x=None, y=None):
        """Warm start of the next run() (hprlp_solver_set_start): after init(), in the model's units and numbering."""
        xs, ys = _start_vector(x, self.model.n, "x"), _start_vector(y, self.model.m, "y")
        self._chk(lib().hprlp_solver_set_start(self.h, _dptr(xs), _dptr(ys)))

    def prepare(self):
        """scale(), power_iteration(), init(-1, 1.01 lambda): ready for run(), and later for set_data() / resolve()."""
        self.scale()
        lam, _ = self.power_iteration()
        self.init(-1.0, 1.01 * lam)

    def _data_vector(self, v, length, name):
        if v is None:
            return None
        a = _as(v, np.float64)
        if a.ndim != 1 or a.shape[0] != length:
            raise ValueError(f"set_data: {name} must have length {length}, got shape {a.shape}")
        return a

    def set_data(self, c=None, obj_constant=None, AL=None, AU=None, l=None, u=None):
        """New data for the LP this solver holds (hprlp_solver_set_data), in the model's units and numbering.  c and / or
        obj_constant; AL, AU, l, u together or not at all.  What is not given stays bit for bit."""
        m, n = self.model.m, self.model.n
        cv, ALv, AUv = self._data_vector(c, n, "c"), self._data_vector(AL, m, "AL"), self._data_vector(AU, m, "AU")
        lv, uv = self._data_vector(l, n, "l"), self._data_vector(u, n, "u")
        oc = None if obj_constant is None else C.byref(C.c_double(float(obj_constant)))
        self._chk(lib().hprlp_solver_set_data(self.h, _dptr(cv), oc, _dptr(ALv), _dptr(AUv), _dptr(lv), _dptr(uv)))

    def resolve(self, x=None, y=None, sigma=-1.0, max_trace=4096):
        """A further solve on this solver (hprlp_solver_resolve): from zero, or from (x, y); sigma > 0 overrides the
        norm_b / norm_c rule.  Returns what run() returns."""
        xs, ys = _start_vector(x, self.model.n, "x"), _start_vector(y, self.model.m, "y")
        res = CResults()
        trace = (CTraceRow * max_trace)()
        nt = C.c_int(0)
        self._chk(lib().hprlp_solver_resolve(self.h, float(sigma), _dptr(xs), _dptr(ys), C.byref(res), trace, max_trace,
                                             C.byref(nt)))
        r = Results(res, self.model.m, self.model.n)
        r.trace = [{f: getattr(trace[i], f) for f, _ in CTraceRow._fields_} for i in range(nt.value)]
        return r

    @staticmethod
    def set_data_many(solvers, data):
        """set_data(**data[k]) of every solver with one copy, one launch per kernel and one host wait for the members that join
        (hprlp_solver_set_data_many).  data: one dict per solver with the keys of set_data; None or {} changes nothing."""
        solvers, hs = Solver._handles(solvers)
        arr, keep = Solver._member_data("set_data_many", solvers, data, _host_vector)  # (keep: alive until the call returns)
        if lib().hprlp_solver_set_data_many(hs, len(solvers), arr) < 0:
            raise RuntimeError(last_error())

    # ---- the array builders of the group methods: a host method and its *_tensors twin differ in the per-vector converter ----------
    @staticmethod
    def _fill_member(who, sv, d, entry, keep, vector, with_values=False):
        """One member's dict into its CMemberData / CMemberValues entry; what the pointers name is appended to keep."""
        unknown = set(d) - ({"c", "obj_constant", "AL", "AU", "l", "u"} | ({"values"} if with_values else set()))
        if unknown:
            raise ValueError(f"{who}: unknown keys {sorted(unknown)}")
        m, n = sv.model.m, sv.model.n
        if with_values and d.get("values") is not None:
            kept, entry.val = vector(sv, d["values"], None, "values", who)
            entry.nnz = kept.shape[0]
            keep.append(kept)
        for key, length in (("c", n), ("AL", m), ("AU", m), ("l", n), ("u", n)):
            kept, ptr = vector(sv, d.get(key), length, key, who)
            keep.append(kept)
            setattr(entry, key, ptr)
        if d.get("obj_constant") is not None:
            oc = C.c_double(float(d["obj_constant"]))
            keep.append(oc)
            entry.obj_constant = C.pointer(oc)

    @staticmethod
    def _member_data(who, solvers, data, vector):
        """(CMemberData array, keep) of set_data_many / set_data_many_tensors; None or {} leaves a member's entry all NULL."""
        data = list(data)
        if len(data) != len(solvers):
            raise ValueError(f"{who}: one dict (or None) per solver")
        arr = (CMemberData * max(len(solvers), 1))()
        keep = []
        for k, (sv, d) in enumerate(zip(solvers, data)):
            Solver._fill_member(f"{who}: member {k}", sv, dict(d or {}), arr[k], keep, vector)
        return arr, keep

    @staticmethod
    def _member_values(who, solvers, data, vector):
        """(CMemberValues array, keep) of set_matrix_many / set_matrix_many_tensors; None skips a member."""
        data = list(data)
        if len(data) != len(solvers):
            raise ValueError(f"{who}: one dict (or None) per solver")
        arr = (CMemberValues * max(len(solvers), 1))()
        keep = []
        for k, (sv, d) in enumerate(zip(solvers, data)):
            if d is not None:
                Solver._fill_member(f"{who}: member {k}", sv, dict(d), arr[k], keep, vector, with_values=True)
        return arr, keep

    @staticmethod
    def _member_starts(who, solvers, vector, **named):
        """(CMemberStart array, keep, lists) of resolve_many / resolve_many_tensors.  named: x, y, sigma and whatever else the
        method takes per solver, each a list (None entries allowed) or None for all; lists: the same, one entry per solver."""
        K = len(solvers)
        lists = {}
        for name, v in named.items():
            v = [None] * K if v is None else list(v)
            if len(v) != K:
                raise ValueError(f"{who}: {name} needs one entry (or None) per solver")
            lists[name] = v
        arr = (CMemberStart * max(K, 1))()
        keep = []
        for k, sv in enumerate(solvers):
            # (lengths are checked here; a non-finite entry is the library's to refuse, naming the member)
            xs, arr[k].x0 = vector(sv, lists["x"][k], sv.model.n, "x", f"{who}: member {k}")
            ys, arr[k].y0 = vector(sv, lists["y"][k], sv.model.m, "y", f"{who}: member {k}")
            keep += [xs, ys]
            arr[k].sigma = -1.0 if lists["sigma"][k] is None else float(lists["sigma"][k])
        return arr, keep, lists

    @staticmethod
    def resolve_many(solvers, x=None, y=None, sigma=None):
        """resolve(x[k], y[k], sigma[k]) of every solver in lock-step (hprlp_solver_resolve_many).  x, y, sigma: lists (None
        entries allowed), or None for all.  Returns a list of Results (no trace)."""
        solvers, hs = Solver._handles(solvers)
        K = len(solvers)
        arr, keep, _ = Solver._member_starts("resolve_many", solvers, _host_vector, x=x, y=y, sigma=sigma)
        res = (CResults * max(K, 1))()
        if lib().hprlp_solver_resolve_many(hs, K, arr, res) < 0:
            raise RuntimeError(last_error())
        return [Results(res[k], sv.model.m, sv.model.n) for k, sv in enumerate(solvers)]

    def data_seconds(self):
        """Seconds of the last set_data(): {upload, kernels, total}."""
        out = np.zeros(3)
        self._chk(lib().hprlp_solver_data_seconds(self.h, out.ctypes.data_as(c_dbl_p)))
        return dict(zip(("upload", "kernels", "total"), out))

    def set_matrix(self, values, c, AL, AU, l, u, obj_constant=None):
        """New matrix values on the resident pattern (hprlp_solver_set_matrix_values), then what prepare() does after scale():
        power_iteration() and init(-1, 1.01 lambda).  values: the nnz values in the order of the model's CSR; all five vectors are
        required, in the model's units and numbering.  Afterwards the solver is bit for bit a fresh Solver on the changed model
        after prepare(); resolve() runs it.  Returns (lambda, power iterations)."""
        m, n = self.model.m, self.model.n
        nnz = self.model.nnz if hasattr(self.model, "nnz") else self.info()["nnz"]
        v = _as(values, np.float64)
        if v.ndim != 1 or v.shape[0] != nnz:
            raise ValueError(f"set_matrix: values must have length {nnz}, got shape {v.shape}")
        vecs = []
        for arr, length, name in ((c, n, "c"), (AL, m, "AL"), (AU, m, "AU"), (l, n, "l"), (u, n, "u")):
            if arr is None:
                raise ValueError(f"set_matrix: {name} is required (length {length})")
            a = _as(arr, np.float64)
            if a.ndim != 1 or a.shape[0] != length:
                raise ValueError(f"set_matrix: {name} must have length {length}, got shape {a.shape}")
            vecs.append(a)
        oc = None if obj_constant is None else C.byref(C.c_double(float(obj_constant)))
        self._chk(lib().hprlp_solver_set_matrix_values(self.h, _dptr(v), nnz, _dptr(vecs[0]), oc, *[_dptr(a) for a in vecs[1:]]))
        lam, its = self.power_iteration()
        self.init(-1.0, 1.01 * lam)
        return lam, its

    @staticmethod
    def set_matrix_many(solvers, data):
        """New matrix values for every solver of a group (hprlp_solver_set_matrix_values_many): one copy, one check and one launch
        per kernel and stage for the members that join; every member ends bit for bit where hprlp_solver_set_matrix_values leaves
        it.  data: per solver None (skipped), or a dict of set_matrix's keyword arguments (values, c, AL, AU, l, u and, optionally,
        obj_constant).  Unlike set_matrix() this is the C call alone: power_iteration_many(), init() and resolve_many() come next,
        as after scale_many()."""
        solvers, hs = Solver._handles(solvers)
        arr, keep = Solver._member_values("set_matrix_many", solvers, data, _host_vector)  # (keep: alive until the call returns)
        if lib().hprlp_solver_set_matrix_values_many(hs, len(solvers), arr) < 0:
            raise RuntimeError(last_error())

    def matrix_seconds(self):
        """Seconds of the last set_matrix() (without its power iteration): {maps (first call only), upload, kernels, scale, total}
        and the calls so far."""
        out = np.zeros(6)
        self._chk(lib().hprlp_solver_matrix_seconds(self.h, out.ctypes.data_as(c_dbl_p)))
        d = dict(zip(("maps", "upload", "kernels", "scale", "total"), out[:5]))
        d["calls"] = int(out[5])
        return d

    # ---- device-resident re-solve (DESIGN.md "Device-resident re-solve"): torch tensors in, torch tensors out ----------------------
    def _tensor(self, t, length, name, who):
        """A caller's tensor as contiguous device memory of `length` doubles: (what keeps it alive, its address)."""
        import torch
        if t is None:
            return None, None
        dev = getattr(self, "device_number", 0)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise ValueError(f"{who}: {name} must be float64, got {t.dtype}")
        if t.device.type != "cuda" or t.device.index != dev:
            raise ValueError(f"{who}: {name} must be on the solver's device cuda:{dev}, got {t.device}")
        if t.dim() != 1 or t.shape[0] != length:
            raise ValueError(f"{who}: {name} must have length {length}, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            t = t.contiguous()
        return t, t.data_ptr()

    def _torch_stream(self):
        import torch
        return torch.cuda.current_stream(torch.device("cuda", getattr(self, "device_number", 0))).cuda_stream

    def set_data_tensors(self, c=None, obj_constant=None, AL=None, AU=None, l=None, u=None):
        """set_data() for vectors that are on the GPU already (hprlp_solver_set_data_device): float64 torch tensors on the solver's
        device, 1-D, taken as ordered on the current torch stream.  A contiguous tensor is passed as it is, any other layout costs
        one copy on the device.  ValueError for a wrong type, dtype, device or length, before the library is called; RuntimeError
        with the library's message for a call it refuses, which leaves the solver as it was.  Same bits as set_data()."""
        m, n = self.model.m, self.model.n
        keep = [self._tensor(t, length, name, "set_data_tensors")
                for t, length, name in ((c, n, "c"), (AL, m, "AL"), (AU, m, "AU"), (l, n, "l"), (u, n, "u"))]
        oc = None if obj_constant is None else C.byref(C.c_double(float(obj_constant)))
        p = [a for _, a in keep]
        self._chk(lib().hprlp_solver_set_data_device(self.h, p[0], oc, p[1], p[2], p[3], p[4], self._torch_stream()))

    def resolve_tensors(self, x=None, y=None, sigma=-1.0, max_trace=4096):
        """resolve() from a start on the GPU, or cold, with the solution left on the GPU (hprlp_solver_resolve_device).  Returns
        the Results of resolve() with x, y, z as fresh float64 tensors on the solver's device; scalars and trace as from resolve()."""
        import torch
        m, n = self.model.m, self.model.n
        xs, ys = self._tensor(x, n, "x", "resolve_tensors"), self._tensor(y, m, "y", "resolve_tensors")
        device = torch.device("cuda", getattr(self, "device_number", 0))
        xo, yo, zo = (torch.empty(k, dtype=torch.float64, device=device) for k in (n, m, n))
        res = CResults()
        trace = (CTraceRow * max_trace)()
        nt = C.c_int(0)
        self._chk(lib().hprlp_solver_resolve_device(self.h, float(sigma), xs[1], ys[1], self._torch_stream(), xo.data_ptr(), yo.data_ptr(),
                                                    zo.data_ptr(), C.byref(res), trace, max_trace, C.byref(nt)))
        r = Results(res, m, n)  # (x, y, z of the C struct are NULL)
        r.x, r.y, r.z = xo, yo, zo
        r.trace = [{f: getattr(trace[i], f) for f, _ in CTraceRow._fields_} for i in range(nt.value)]
        return r

    def set_matrix_tensors(self, values, c, AL, AU, l, u, obj_constant=None):
        """set_matrix() for values and vectors that are on the GPU already (hprlp_solver_set_matrix_values_device), then
        power_iteration() and init(-1, 1.01 lambda) as there.  Returns (lambda, power iterations).  Same bits as set_matrix()."""
        m, n = self.model.m, self.model.n
        nnz = self.model.nnz if hasattr(self.model, "nnz") else self.info()["nnz"]
        keep = []
        for t, length, name in ((values, nnz, "values"), (c, n, "c"), (AL, m, "AL"), (AU, m, "AU"), (l, n, "l"), (u, n, "u")):
            if t is None:
                raise ValueError(f"set_matrix_tensors: {name} is required (length {length})")
            keep.append(self._tensor(t, length, name, "set_matrix_tensors"))
        oc = None if obj_constant is None else C.byref(C.c_double(float(obj_constant)))
        p = [a for _, a in keep]
        self._chk(lib().hprlp_solver_set_matrix_values_device(self.h, p[0], nnz, p[1], oc, p[2], p[3], p[4], p[5], self._torch_stream()))
        lam, its = self.power_iteration()
        self.init(-1.0, 1.01 * lam)
        return lam, its

    # ---- group device re-solve (DESIGN.md "Many small LPs", group device re-solve): the *_many methods with torch tensors ------------
    @staticmethod
    def set_data_many_tensors(solvers, data):
        """set_data_many() for vectors that are on the GPU already (hprlp_solver_set_data_many_device).  data: one dict per solver
        with the keys of set_data_tensors -- float64 torch tensors on the solvers' device, 1-D and contiguous (rows of a 2-D tensor
        and slices of a packed one are welcome: they are views), taken as ordered on the current torch stream; obj_constant is a
        host number; None or {} changes nothing.  No vector is copied.  Same bits as set_data_many()."""
        solvers, hs = Solver._handles(solvers)
        arr, keep = Solver._member_data("set_data_many_tensors", solvers, data, _device_vector)  # (keep: alive until the call returns)
        stream = solvers[0]._torch_stream() if solvers else None
        if lib().hprlp_solver_set_data_many_device(hs, len(solvers), arr, stream) < 0:
            raise RuntimeError(last_error())

    @staticmethod
    def resolve_many_tensors(solvers, x=None, y=None, sigma=None, out=None):
        """resolve_many() from starts on the GPU, or cold, with the solutions left on the GPU (hprlp_solver_resolve_many_device).
        x, y: lists of float64 tensors (None entries allowed) or None for all; sigma: as resolve_many.  out: a list with one
        (x, y, z) triple of tensors to write into per solver -- any of the three, or the whole entry, may be None: not wanted; a
        triple's x and y may be the tensors given as that member's start.  Without out the method allocates ONE tensor per kind
        for the whole group and the members' x, y, z are views of them.  Returns a list of Results (no trace) that carry the
        tensors as x, y, z (None where none was wanted).  No start and no solution is copied.  Same bits as resolve_many()."""
        import torch
        solvers, hs = Solver._handles(solvers)
        K = len(solvers)
        starts, keep, lists = Solver._member_starts("resolve_many_tensors", solvers, _device_vector, x=x, y=y, sigma=sigma, out=out)
        wanted = lists["out"]
        if out is None and K > 0:
            device = torch.device("cuda", getattr(solvers[0], "device_number", 0))
            ns, ms = [sv.model.n for sv in solvers], [sv.model.m for sv in solvers]
            xs_all, zs_all = (torch.empty(sum(ns), dtype=torch.float64, device=device) for _ in range(2))
            ys_all = torch.empty(sum(ms), dtype=torch.float64, device=device)
            an = am = 0
            for k in range(K):
                wanted[k] = (xs_all[an:an + ns[k]], ys_all[am:am + ms[k]], zs_all[an:an + ns[k]])
                an, am = an + ns[k], am + ms[k]
        dst = (CMemberOut * max(K, 1))()
        outs = []
        for k, sv in enumerate(solvers):
            who = f"resolve_many_tensors: member {k}"
            m, n = sv.model.m, sv.model.n
            triple = tuple(wanted[k]) if wanted[k] is not None else (None, None, None)
            if len(triple) != 3:
                raise ValueError(f"{who}: out is an (x, y, z) triple of tensors or Nones")
            for t, length, name in zip(triple, (n, m, n), ("x", "y", "z")):
                if t is not None and (not isinstance(t, torch.Tensor) or not t.is_contiguous()):
                    raise ValueError(f"{who}: out {name} must be a contiguous torch tensor (it is written in place)")
                setattr(dst[k], name, sv._tensor(t, length, "out " + name, who)[1])
            outs.append(triple)
        res = (CResults * max(K, 1))()
        stream = solvers[0]._torch_stream() if solvers else None
        if lib().hprlp_solver_resolve_many_device(hs, K, starts, dst, stream, res) < 0:
            raise RuntimeError(last_error())
        results = []
        for k, sv in enumerate(solvers):
            r = Results(res[k], sv.model.m, sv.model.n)  # (x, y, z of the C struct are NULL)
            r.x, r.y, r.z = outs[k]
            results.append(r)
        return results

    @staticmethod
    def set_matrix_many_tensors(solvers, data):
        """set_matrix_many() for values and vectors that are on the GPU already (hprlp_solver_set_matrix_values_many_device).
        data: per solver None (skipped) or a dict of set_matrix_tensors' keyword arguments (values, c, AL, AU, l, u as float64
        tensors; optionally obj_constant, a host number).  As set_matrix_many() this is the C call alone:
        power_iteration_many(), init() and a re-solve come next.  Same bits as set_matrix_many()."""
        solvers, hs = Solver._handles(solvers)
        arr, keep = Solver._member_values("set_matrix_many_tensors", solvers, data, _device_vector)  # (keep: alive until the call returns)
        stream = solvers[0]._torch_stream() if solvers else None
        if lib().hprlp_solver_set_matrix_values_many_device(hs, len(solvers), arr, stream) < 0:
            raise RuntimeError(last_error())

    def transfer(self):
        """The last successful set_data* / set_matrix* / resolve* call's traffic of model data and solution in bytes, host to
        device and back (not the loop's scalar fetches), whether it was a *_tensors call, and how many of those there have been."""
        out = (C.c_long * 4)()
        self._chk(lib().hprlp_solver_transfer(self.h, out))
        return dict(zip(("h2d_bytes", "d2h_bytes", "device_entry", "device_calls"), [int(v) for v in out]))

    def value_maps(self):
        """(mapA, mapAT) as the solver built them (hprlp_solver_value_maps): the model's CSR position of every entry of A and of
        A^T in the solver's internal numbering."""
        nnz = self.info()["nnz"]
        a, t = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.int32)
        k = lib().hprlp_solver_value_maps(self.h, a.ctypes.data_as(c_int_p), t.ctypes.data_as(c_int_p), nnz)
        if k < 0:
            raise RuntimeError(last_error())
        return a[:k].copy(), t[:k].copy()

    def ordering(self):
        """The locality ordering in place as (row_new2old, col_new2old), or None without one (hprlp_solver_ordering)."""
        r, c = np.zeros(max(self.model.m, 1), np.int32), np.zeros(max(self.model.n, 1), np.int32)
        rc = self._chk(lib().hprlp_solver_ordering(self.h, r.ctypes.data_as(c_int_p), c.ctypes.data_as(c_int_p)))
        return (r[:self.model.m], c[:self.model.n]) if rc == 1 else None

    def power_start(self):
        """Test infrastructure (hprlp_solver_power_start): the power iteration's start vector as the solver forms it, read back in
        the caller's numbering."""
        L = lib()
        L.hprlp_solver_power_start.argtypes = [C.c_void_p, c_dbl_p, C.c_int]
        z = np.zeros(max(self.model.m, 1))
        k = self._chk(L.hprlp_solver_power_start(self.h, z.ctypes.data_as(c_dbl_p), len(z)))
        return z[:k].copy()

    def certificate(self):
        """The certificate of the last run() (kind 0 without a verdict)."""
        cc = CCertificate()
        self._chk(lib().hprlp_solver_get_certificate(self.h, C.byref(cc)))
        return Certificate(cc)

    def time_iterations(self, warmup, steps, mode=0):
        t = C.c_double(0); tx = C.c_double(0); ty = C.c_double(0)
        self._chk(lib().hprlp_solver_time_iterations(self.h, warmup, steps, mode, C.byref(t), C.byref(tx), C.byref(ty)))
        return dict(total_ms=t.value, xhalf_ms=tx.value, yhalf_ms=ty.value)
