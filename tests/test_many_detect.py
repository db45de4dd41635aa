"""Group detection of many small LPs, the parts that need no GPU (include/hprlp_amd.h: hprlp_solve_many_detect,
hprlp_solver_ray_step_many, hprlp_last_run_many_counts; csrc/group_pack.cpp: the certificate block; csrc/group_table.cpp: the shape
of a periodic round with detection; DESIGN.md "Many small LPs", group detection): the entries exist with the header's signatures,
wrong arguments are refused with a message that names the entry before any device work, a host without a GPU gets an error and no
crash, and the two host pieces run clean under the host sanitizers as a stand-alone program.  What needs a GPU is in
tests/test_gpu_many_detect.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen
from test_resolve import header_prototypes

SYMBOLS = ("hprlp_solve_many_detect", "hprlp_solver_ray_step_many")
WANT = {
    "hprlp_solve_many_detect": ["const LP_info_cpu *const *", "int", "const HPRLP_parameters *", "const hprlp_detection *", "HPRLP_results *",
                                "hprlp_certificate *"],
    "hprlp_solver_ray_step_many": ["hprlp_solver * *", "int", "const int *", "double *", "int *"],
}
CTYPE_OF = {"hprlp_solver * *": C.POINTER(C.c_void_p), "int": C.c_int, "double *": hprlp.c_dbl_p, "int *": hprlp.c_int_p,
            "const int *": hprlp.c_int_p, "HPRLP_results *": C.POINTER(hprlp.CResults),
            "const LP_info_cpu *const *": C.POINTER(C.POINTER(hprlp.CLPInfo)), "const HPRLP_parameters *": C.POINTER(hprlp.CParameters),
            "const hprlp_detection *": C.POINTER(hprlp.CDetection), "hprlp_certificate *": C.POINTER(hprlp.CCertificate)}


def small_models(count=3):
    lps = [lpgen.planted_lp(30, 50, 200, seed) for seed in range(1, count + 1)]
    return [hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
            for lp in lps]


def test_the_new_symbols_are_exported():
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


def test_python_has_the_wrappers_and_the_two_new_counts():
    assert callable(hprlp.solve_many_detect) and callable(hprlp.Solver.ray_step_many) and callable(hprlp.last_run_many_detect_counts)
    counts = hprlp.last_run_many_detect_counts()
    assert list(counts) == ["rounds", "waits", "group_launches", "copies", "own", "served", "ray_served", "certs_served"]
    assert all(isinstance(v, int) and v >= 0 for v in counts.values())
    first_six = hprlp.last_run_many_counts()   # (what it always returned: tests/test_many_group.py holds its key set)
    assert first_six == {k: counts[k] for k in list(counts)[:6]}
    with pytest.raises(ValueError):
        hprlp.solve_many_detect([])


def test_wrong_arguments_are_refused_with_a_message_that_names_the_entry():
    """NULL lists, count <= 0, a NULL member, a negative eps: -1 and the entry's name, with or without a GPU (nothing is created or
    launched: the eps is judged before the first model is set up, and no handle exists that anything could be launched for)."""
    L = hprlp.lib()
    cp = hprlp.Parameters().to_c()
    res = (hprlp.CResults * 2)()
    certs = (hprlp.CCertificate * 2)()
    det = hprlp.CDetection(1e-8, 1e-8)
    ms = (C.POINTER(hprlp.CLPInfo) * 2)()
    for m_, k, r_, word in ((None, 2, res, "null model list"), (ms, 0, res, "count must be positive"), (ms, -1, res, "count must be positive"),
                            (ms, 2, None, "null results"), (ms, 2, res, "model 0 is null")):
        for d in (C.byref(det), None):
            assert L.hprlp_solve_many_detect(m_, k, C.byref(cp), d, r_, certs) == -1, word
            assert "hprlp_solve_many_detect" in hprlp.last_error() and word in hprlp.last_error(), (word, hprlp.last_error())
    models = small_models(2)
    ptrs = (C.POINTER(hprlp.CLPInfo) * 2)(*[m._ptr for m in models])
    for bad in (hprlp.CDetection(-1e-8, 1e-8), hprlp.CDetection(1e-8, -1.0), hprlp.CDetection(float("nan"), 1e-8)):
        assert L.hprlp_solve_many_detect(ptrs, 2, C.byref(cp), C.byref(bad), res, certs) == -1
        assert "hprlp_solve_many_detect" in hprlp.last_error() and "must be >= 0" in hprlp.last_error(), hprlp.last_error()
    with pytest.raises(RuntimeError, match="hprlp_solve_many_detect.*must be >= 0"):
        hprlp.solve_many_detect(models, eps_primal=-1.0)
    for m in models:
        m.free()
    # the step-level entry: the plain arrays first, then the list
    flags, tested, out = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(18)
    F, T, O = flags.ctypes.data_as(hprlp.c_int_p), tested.ctypes.data_as(hprlp.c_int_p), out.ctypes.data_as(hprlp.c_dbl_p)
    hs = (C.c_void_p * 2)(None, None)
    for h, k, f, o, t, word in ((hs, 2, None, O, T, "null restart"), (hs, 2, F, None, T, "null out"), (hs, 2, F, O, None, "null tested"),
                                (None, 2, F, O, T, "null solver list"), (hs, 0, F, O, T, "count must be positive"),
                                (hs, -2, F, O, T, "count must be positive"), (hs, 2, F, O, T, "member 0 is null")):
        assert L.hprlp_solver_ray_step_many(h, k, f, o, t) == -1, word
        assert "hprlp_solver_ray_step_many" in hprlp.last_error() and word in hprlp.last_error(), (word, hprlp.last_error())
    assert not out.any() and not tested.any()


def test_solve_many_detect_without_a_gpu_is_an_error_not_a_crash(capfd):
    """No CPU fallback exists: every member comes back with status ERROR, no arrays and a certificate of kind 0 that carries its
    m and n (hprlp_solve_detect's contract)."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    models = small_models(3)
    results, certs = hprlp.solve_many_detect(models, hprlp.Parameters(max_iter=100))
    assert [r.status for r in results] == ["ERROR"] * 3
    assert all(r.x is None and r.y is None and r.z is None for r in results)
    assert "hprlp_solve_many_detect: model 2" in hprlp.last_error()
    for k, m in zip(certs, models):
        assert k.kind == 0 and k.y is None and k.z is None and k.d is None and (k.m, k.n) == (m.m, m.n)
    err = capfd.readouterr().err
    for k in range(3):
        assert f"model {k} failed its set-up" in err
    counts = hprlp.last_run_many_detect_counts()
    assert counts["ray_served"] == 0 and counts["certs_served"] == 0
    for m in models:
        m.free()


def test_the_host_selftests_pass_with_their_new_checks():
    """group_pack: check 9, the certificate block; group_table: check 10, the stage of an evaluation with the three ray kinds."""
    L = hprlp.lib()
    assert L.hprlp_group_pack_selftest() == 0
    assert L.hprlp_group_table_selftest() == 0


def test_the_host_pieces_run_clean_under_the_host_sanitizers(tmp_path):
    """group_pack.cpp and group_table.cpp in the stand-alone program tools/group_pack_check.cpp (its own main, no GPU, no HIP) under
    AddressSanitizer and UndefinedBehaviorSanitizer: both self-tests ok, exit 0, no report.  Nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "hpr-lp-c_amd", "csrc")
    exe = tmp_path / "group_pack_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(ROOT, "tools", "group_pack_check.cpp"), os.path.join(csrc, "group_pack.cpp"),
                           os.path.join(csrc, "group_table.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert "group pack self-test: ok (0)" in r.stdout and "group table self-test: ok (0)" in r.stdout, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
