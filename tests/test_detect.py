"""CPU: the infeasibility detection's C ABI (include/hprlp_amd.h: hprlp_detection, hprlp_certificate, hprlp_solve_detect, ...)
and the generators of infeasible / unbounded LPs (hpr-lp-c_amd/lpgen.py), judged by HiGHS and by a numpy restatement of the
Farkas ratio tests -- never by the library itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import sparse
from scipy.optimize import linprog

from conftest import ROOT, hprlp, lpgen

INC = os.path.join(ROOT, "include")


# ---- the ratio tests, restated (model min c'x, AL <= Ax <= AU, l <= x <= u) -----------------------------------------------------
def primal_ray_test(lp, y):
    """(D, V) of a dual ray y: z = -A'y; D sums the finite bound terms, V is the largest multiplier of an infinite bound."""
    A = sparse.csr_matrix(lp["A"]) if "A" in lp else sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    y = np.asarray(y, float)
    z = -(A.T @ y)
    D, V = 0.0, 0.0
    for v, lo, hi in ((y, lp["AL"], lp["AU"]), (z, lp["l"], lp["u"])):
        pos, neg = v > 0, v < 0
        D += np.sum(lo[pos & np.isfinite(lo)] * v[pos & np.isfinite(lo)]) + np.sum(hi[neg & np.isfinite(hi)] * v[neg & np.isfinite(hi)])
        viol = np.concatenate([v[pos & ~np.isfinite(lo)], -v[neg & ~np.isfinite(hi)], [0.0]])
        V = max(V, float(viol.max()))
    return float(D), V


def dual_ray_test(lp, d):
    """(c'd, W) of a primal ray d: W is the largest step of q = Ad or of d out of the cone of the finite bounds."""
    A = sparse.csr_matrix(lp["A"]) if "A" in lp else sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    d = np.asarray(d, float)
    q = A @ d
    W = 0.0
    for v, lo, hi in ((q, lp["AL"], lp["AU"]), (d, lp["l"], lp["u"])):
        W = max(W, float(np.max(np.concatenate([-v[np.isfinite(lo)], v[np.isfinite(hi)], [0.0]]))))
    return float(lp["c"] @ d), W


def highs_status(lp):
    A = sparse.csr_matrix(lp["A"])
    AL, AU = lp["AL"], lp["AU"]
    fu, fl = np.isfinite(AU), np.isfinite(AL)
    bounds = [(None if not np.isfinite(a) else a, None if not np.isfinite(b) else b) for a, b in zip(lp["l"], lp["u"])]
    r = linprog(lp["c"], A_ub=sparse.vstack([A[fu], -A[fl]]), b_ub=np.concatenate([AU[fu], -AL[fl]]), bounds=bounds, method="highs")
    return r.status


INFEASIBLE = {
    "planted 300x400": lambda: lpgen.planted_infeasible_lp(300, 400, 2400, 1),
    "planted 2000x1500": lambda: lpgen.planted_infeasible_lp(2000, 1500, 12000, 2),
    "transportation 30 < 36": lambda: lpgen.transportation_lp([10, 10, 10], [12, 12, 12], 3),
    "transportation 8x12": lambda: lpgen.transportation_lp(np.full(8, 5.0), np.full(12, 3.5), 4),
    "transportation 6x8, fixed shipments": lambda: lpgen.transportation_lp(np.full(6, 5.0), np.full(8, 4.0), 3, fixed=3),
}
UNBOUNDED = {
    "planted 300x400": lambda: lpgen.planted_unbounded_lp(300, 400, 2400, 5),
    "planted 1500x2000": lambda: lpgen.planted_unbounded_lp(1500, 2000, 12000, 6),
}


@pytest.mark.parametrize("name", sorted(INFEASIBLE))
def test_generated_infeasible_lps_and_their_certificates(name):
    lp = INFEASIBLE[name]()
    assert highs_status(lp) == 2, name  # HiGHS: infeasible
    D, V = primal_ray_test(lp, lp["y_cert"])
    assert D > 0 and V <= 1e-12 * D, (D, V)
    np.testing.assert_allclose(-(sparse.csr_matrix(lp["A"]).T @ lp["y_cert"]), lp["z_cert"], atol=1e-12)


@pytest.mark.parametrize("name", sorted(UNBOUNDED))
def test_generated_unbounded_lps_and_their_certificates(name):
    lp = UNBOUNDED[name]()
    assert highs_status(lp) == 3, name  # HiGHS: unbounded
    cd, W = dual_ray_test(lp, lp["d_cert"])
    assert cd < 0 and W <= 1e-12 * -cd, (cd, W)


def test_ratio_tests_reject_a_feasible_lp_ray():
    """The restatement itself: on a feasible planted LP no y passes the primal test (Farkas) -- its planted dual optimum and
    random vectors give D <= 0 or a violation."""
    lp = lpgen.planted_lp(200, 300, 1500, 7)
    rng = np.random.default_rng(0)
    for y in [lp["y_star"]] + [rng.normal(size=200) for _ in range(20)]:
        D, V = primal_ray_test(lp, y)
        assert not (D > 0 and V <= 1e-8 * D)


def test_presolve_reduces_the_transportation_lp_with_fixed_shipments():
    """The model tests/test_gpu_detect.py uses for the presolve path: the host presolver removes its fixed columns (so a
    detection solve with presolve runs the reduced model first), and leaves the plain transportation LP alone."""
    for fixed, reduced in ((0, False), (3, True)):
        lp = lpgen.transportation_lp(np.full(6, 5.0), np.full(8, 4.0), 3, fixed=fixed)
        model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
        if reduced:
            pre = hprlp.Presolved(model)
            assert pre.stats["fixed_cols"] == 3 and (pre.stats["m"], pre.stats["n"]) == (lp["m"], lp["n"] - 3), pre.stats
            pre.free()
        else:
            with pytest.raises(RuntimeError):
                hprlp.Presolved(model)
        model.free()


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "hprlp_amd.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(hprlp_detection), offsetof(hprlp_detection, eps_primal_infeasible), offsetof(hprlp_detection, eps_dual_infeasible));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hprlp_certificate), offsetof(hprlp_certificate, kind),
           offsetof(hprlp_certificate, iter), offsetof(hprlp_certificate, m), offsetof(hprlp_certificate, n),
           offsetof(hprlp_certificate, objective), offsetof(hprlp_certificate, violation), offsetof(hprlp_certificate, y),
           offsetof(hprlp_certificate, z), offsetof(hprlp_certificate, d));
    return 0;
}
"""


@pytest.mark.parametrize("cc,std", [("gcc", "-std=c11"), ("g++", "-std=c++11")])
def test_struct_layouts_equal_the_ctypes_mirrors(cc, std, tmp_path):
    src = tmp_path / ("probe.c" if cc == "gcc" else "probe.cpp")
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, std, "-I", INC, str(src), "-o", str(exe)])
    det, cert = [list(map(int, ln.split())) for ln in subprocess.check_output([str(exe)]).decode().split("\n") if ln]
    D, K = hprlp.CDetection, hprlp.CCertificate
    assert det == [C.sizeof(D), D.eps_primal_infeasible.offset, D.eps_dual_infeasible.offset]
    assert cert == [C.sizeof(K)] + [getattr(K, f).offset for f in ("kind", "iter", "m", "n", "objective", "violation", "y", "z", "d")]


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("hprlp_solve_detect", "hprlp_free_certificate", "hprlp_solver_set_detection", "hprlp_solver_get_certificate",
              "hprlp_solver_ray_step"):
        assert s in names, s


def test_solve_detect_without_a_gpu_is_an_error_not_a_crash():
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    lp = lpgen.transportation_lp([10, 10, 10], [12, 12, 12], 3)
    model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    for presolve in (False, True):
        r = model.solve_detect(hprlp.Parameters(use_presolve=presolve, max_iter=300))
        assert r.status == "ERROR" and r.x is None
        assert hprlp.last_error()
        k = r.certificate
        assert k.kind == 0 and k.y is None and k.z is None and k.d is None and (k.m, k.n) == (lp["m"], lp["n"])
    model.free()
