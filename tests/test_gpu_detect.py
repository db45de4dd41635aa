"""Infeasibility detection on the GPU (include/hprlp_amd.h hprlp_solve_detect / hprlp_solver_set_detection, DESIGN.md
"Infeasibility and unboundedness"): verdicts on the edge cases and on planted LPs through every kernel form, certificates judged
by the numpy restatement of tests/test_detect.py in the caller's units, and no perturbation of feasible solves."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen
from test_detect import dual_ray_test, primal_ray_test

pytestmark = pytest.mark.gpu
INF = np.inf
EPS = 1e-8


def _csr_case(m, n, rp, ci, v, AL, AU, l, u, c):  # (as tests/test_gpu_edge.py)
    return (m, n, np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, float), np.array(AL, float), np.array(AU, float),
            np.array(l, float), np.array(u, float), np.array(c, float))


# the two cases of tests/test_gpu_edge.py that end in ITER_LIMIT there: x >= 2 and x <= 1; min -x with x - y <= 5, both free above
EDGE = {
    "infeasible": _csr_case(2, 1, [0, 1, 2], [0, 0], [1, 1], [2, -INF], [INF, 1], [0], [10], [1]),
    "unbounded": _csr_case(1, 2, [0, 2], [0, 1], [1, -1], [-INF], [5], [0, 0], [INF, INF], [-1, 0]),
}


def as_lp(case):
    m, n, rp, ci, v, AL, AU, l, u, c = case
    return dict(m=m, n=n, rowptr=rp, colind=ci, values=v, AL=AL, AU=AU, l=l, u=u, c=c)


def model_of(lp):
    return hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])


def check_certificate(lp, r, want, by_value=False):
    """The verdict `want` and its certificate in the caller's units and numbering, by the numpy ratio tests (10 x eps); by_value
    (solves with use_CR_scaling off): objective and violation equal D and V resp. c'd and W of the returned ray, from both sides,
    within the derived tolerance of tests/evalref.py: check_certificate_values."""
    import evalref
    k = r.certificate
    assert r.status == want and k.verdict == want, (r.status, k.kind)
    assert (k.m, k.n) == (lp["m"], lp["n"]) and k.iter == r.iter and k.iter > 0
    if want == "PRIMAL_INFEASIBLE":
        assert k.d is None and len(k.y) == lp["m"] and len(k.z) == lp["n"]
        assert abs(np.abs(k.y).max() - 1.0) <= 1e-12
        D, V = primal_ray_test(lp, k.y)
        assert D > 0 and V <= 10 * EPS * D, (D, V)
        from scipy import sparse
        A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
        np.testing.assert_allclose(k.z, -(A.T @ k.y), rtol=1e-9, atol=1e-12)
        assert abs(k.objective - D) <= 1e-6 * abs(D) and k.violation <= 10 * EPS * D
        if by_value:
            evalref.check_certificate_values(lp, 1, k.y, k.objective, k.violation, want)
    else:
        assert k.y is None and k.z is None and len(k.d) == lp["n"]
        assert abs(np.abs(k.d).max() - 1.0) <= 1e-12
        cd, W = dual_ray_test(lp, k.d)
        assert cd < 0 and W <= 10 * EPS * -cd, (cd, W)
        assert abs(k.objective - cd) <= 1e-6 * abs(cd) and k.violation <= 10 * EPS * -cd
        if by_value:
            evalref.check_certificate_values(lp, 2, k.d, k.objective, k.violation, want)
    return k


@pytest.mark.parametrize("name,want", [("infeasible", "PRIMAL_INFEASIBLE"), ("unbounded", "DUAL_INFEASIBLE")])
def test_edge_cases_end_in_a_verdict(gpu, name, want):
    lp = as_lp(EDGE[name])
    model = model_of(lp)
    r = model.solve_detect(hprlp.Parameters(stop_tol=1e-8, max_iter=3000, use_presolve=False, use_CR_scaling=False))
    check_certificate(lp, r, want, by_value=True)
    assert r.iter <= 1500, r.iter
    model.free()


def test_detection_off_through_the_new_entry_is_solve(gpu):
    """Detection off (NULL options) is solve(): an infeasible LP still ends in ITER_LIMIT at max_iter, bit for bit."""
    lp = as_lp(EDGE["infeasible"])
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=1e-8, max_iter=1200, use_presolve=False)
    a = model.solve_detect(prm, eps_primal=None, eps_dual=None)
    b = model.solve(prm)
    assert a.status == b.status == "ITER_LIMIT" and a.iter == b.iter == 1200 and a.certificate.kind == 0
    for f in ("x", "y", "z"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    model.free()


def test_presolve_on_gives_a_certificate_of_the_original_model(gpu, capfd):
    """Presolve removes the three fixed shipments; the reduced model's verdict is no certificate of the caller's model, so the
    original model is solved again with detection: the certificate has the original dimensions and passes the ratio test on
    the original model, and the reported iterations cover both solves."""
    import re
    lp = lpgen.transportation_lp(np.full(6, 5.0), np.full(8, 4.0), 3, fixed=3)   # supply 30 < demand 32
    model = model_of(lp)
    pre = hprlp.Presolved(model)   # (raises if presolve leaves the model unchanged)
    assert pre.stats["fixed_cols"] == 3 and (pre.stats["m"], pre.stats["n"]) == (lp["m"], lp["n"] - 3), pre.stats
    pre.free()
    capfd.readouterr()
    r = model.solve_detect(hprlp.Parameters(max_iter=6000, use_presolve=True, use_CR_scaling=False))
    out = capfd.readouterr().out
    hit = re.search(r"Reduced model ended PRIMAL_INFEASIBLE at iteration (\d+); solving the original model", out)
    assert hit, out[-2000:]
    it_reduced = int(hit.group(1))
    assert it_reduced > 0 and r.iter >= it_reduced + 300, (it_reduced, r.iter)   # (a verdict needs two evaluations)
    check_certificate(lp, r, "PRIMAL_INFEASIBLE", by_value=True)   # (k.iter == r.iter: offset by the reduced solve's count too)
    model.free()


def _identical(a, b):
    return a.status == b.status and a.iter == b.iter and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("x", "y", "z"))


FEASIBLE = {
    "model.mps": lambda: dict(m=2, n=2, rowptr=np.array([0, 2, 4], np.int32), colind=np.array([0, 1, 0, 1], np.int32),
                              values=np.array([1.0, 2.0, 3.0, 1.0]), AL=np.array([-INF, -INF]), AU=np.array([10.0, 12.0]),
                              l=np.zeros(2), u=np.full(2, INF), c=np.array([-3.0, -5.0])),
    "c2_like": lambda: lpgen.c2_25fv47_like(),
    "pds_like": lambda: lpgen.FAMILIES_SMALL["pds_like"](),
    "planted": lambda: lpgen.planted_lp(1500, 2000, 12000, 9),
}


@pytest.mark.parametrize("name", sorted(FEASIBLE))
def test_detection_does_not_perturb_a_feasible_solve(gpu, name):
    lp = FEASIBLE[name]()
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=1e-4, max_iter=6000, use_presolve=False)
    on = model.solve_detect(prm)
    off = model.solve(prm)
    assert on.status in ("OPTIMAL", "ITER_LIMIT") and on.certificate.kind == 0, on.status
    assert _identical(on, off), (on.status, on.iter, off.status, off.iter)
    model.free()


# ---- every kernel form: one subprocess per form (the form thresholds are read once per process) --------------------------------
FORM_SCRIPT = r'''
import os, sys
import numpy as np
from scipy import sparse
sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import hprlp, lpgen
from test_gpu_detect import check_certificate, model_of, _identical
form, kind = sys.argv[1], sys.argv[2]
gen = lpgen.planted_infeasible_lp if kind == "infeasible" else lpgen.planted_unbounded_lp
want = "PRIMAL_INFEASIBLE" if kind == "infeasible" else "DUAL_INFEASIBLE"
if form in ("small", "stream", "all-remainder"):
    m, n = (400, 600) if form == "small" else (3000, 4000)
    lp = gen(m, n, 6 * m, 21)
elif form == "reordered":   # (the shape of tests/test_gpu_reorder.py: its ordering is accepted at the default thresholds)
    m = n = 1_600_000
    rp, ci, v = lpgen.banded_csr(m, n, 10, 16000, 5)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n)); A.sum_duplicates()
    rng = np.random.default_rng(8)
    pr, pc = rng.permutation(m), rng.permutation(n)
    inv = np.empty(n, np.int64); inv[pc] = np.arange(n)
    B = A[pr]; B = sparse.csr_matrix((B.data, inv[B.indices], B.indptr), shape=(m, n)); B.sort_indices()
    lp = gen(m, n, 0, 22, A=B)
else:   # tiled forms: a banded matrix
    m, n = 8000, 10000
    rp, ci, v = lpgen.banded_csr(m, n, 8, 1500, 6)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n)); A.sum_duplicates(); A.sort_indices()
    lp = gen(m, n, 0, 23, A=A)
model = model_of(lp)
by_value = form != "reordered"   # (1.6 M rows; a reordered solver's certificate at a small shape: tests/test_gpu_reorder_small.py, bit twin)
prm = hprlp.Parameters(max_iter=50000, use_presolve=False, use_CR_scaling=not by_value)
s = hprlp.Solver(model, prm)
d, info = s.describe(), s.info()
expect = {"small": "single-workgroup kernel", "stream": "A: stream kernel", "tiled": "tiled, fused (k_tiled_fused",
          "pieces": "tiled, piece form", "all-remainder": "all-remainder form (k_pb_fused", "reordered": "locality ordering applied"}[form]
assert expect in d, d
if form == "stream":
    assert "A^T: stream kernel" in d and "single-workgroup" not in d, d
s.set_detection()
s.scale(); lam, _ = s.power_iteration(); s.init(-1.0, lam * 1.01)
rs = s.run(max_trace=1)
ks = s.certificate()
s.close()
r1 = model.solve_detect(prm); k1 = check_certificate(lp, r1, want, by_value)
assert rs.status == want and ks.kind == k1.kind and ks.iter == r1.iter, (rs.status, ks.iter, r1.iter)
if form != "reordered":  # (there the step-level run above is the second run)
    r2 = model.solve_detect(prm); k2 = check_certificate(lp, r2, want, False)
    assert r1.iter == r2.iter and np.array_equal(k1.y if k1.y is not None else k1.d, k2.y if k2.y is not None else k2.d)
print("OK", form, kind, r1.status, r1.iter, r1.time, d)
''' % ROOT

BASE_ENV = {"HPRLP_TEST_HOOKS": "1"}
FORM_ENV = {
    "small": {},
    "stream": {"HPRLP_NO_SMALL": "1"},
    "tiled": {"HPRLP_NO_SMALL": "1", "HPRLP_TILED_MIN_ROWS": "1", "HPRLP_TILED_MIN_DENSE": "0.0", "HPRLP_TILE_PIECES": "0",
              "HPRLP_NO_REORDER": "1"},
    "pieces": {"HPRLP_NO_SMALL": "1", "HPRLP_TILED_MIN_ROWS": "1", "HPRLP_TILED_MIN_DENSE": "0.0", "HPRLP_TILE_PIECES": "16",
               "HPRLP_PIECES_ANYWAY": "1", "HPRLP_NO_REORDER": "1"},
    "all-remainder": {"HPRLP_NO_SMALL": "1", "HPRLP_DEVICE_TRANSPOSE_MIN": "1000", "HPRLP_PB_MIN_COLS": "1", "HPRLP_PB_MIN_NNZ": "1",
                      "HPRLP_TILED_MIN_ROWS": "1", "HPRLP_NO_REORDER": "1", "HPRLP_TILED_MIN_DENSE": "1.01"},
    "reordered": {"HPRLP_NO_SMALL": "1"},
}


@pytest.mark.parametrize("kind", ["infeasible", "unbounded"])
@pytest.mark.parametrize("form", list(FORM_ENV))
def test_planted_verdicts_on_every_kernel_form(gpu, form, kind):
    env = dict(os.environ, **BASE_ENV, **FORM_ENV[form])
    r = subprocess.run([sys.executable, "-c", FORM_SCRIPT, form, kind], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or "OK" not in r.stdout:
        pytest.fail("form %s, %s: exit %d\n%s\n%s" % (form, kind, r.returncode, r.stdout[-800:], r.stderr[-2500:]), pytrace=False)
    print(r.stdout.strip().splitlines()[-1])


def test_sharded_solver_refuses_detection(gpu):
    lp = lpgen.planted_lp(300, 400, 2000, 3)
    model = model_of(lp)
    group = hprlp.Solver.local_group(2)
    errs = [None, None]

    def work(rank):
        s = hprlp.Solver.create_local(model, hprlp.Parameters(use_presolve=False), rank, 2, group)
        try:
            s.set_detection()
        except RuntimeError as e:
            errs[rank] = str(e)
        s.set_detection(on=False)  # (off is accepted)
        s.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    hprlp.Solver.free_local_group(group)
    assert all(e and "one GPU only" in e for e in errs), errs
    model.free()
