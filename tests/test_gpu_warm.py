"""Warm start on the GPU (include/hprlp_amd.h hprlp_solve_warm / hprlp_solve_batched_warm / hprlp_solver_set_start, DESIGN.md
"Warm start"): a start that already meets the tolerance ends OPTIMAL at iteration 0 on every kernel form, the iteration-0 trace
row is the KKT error of the projected start (a numpy restatement judges it), a zero or NULL start is the cold solve bit for bit,
and the batched members start, freeze and iterate member by member."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from scipy import sparse

from conftest import ROOT, hprlp, lpgen
from test_gpu_detect import BASE_ENV, FORM_ENV, check_certificate, model_of

pytestmark = pytest.mark.gpu


def project(lp, x, y):
    """Item 2 of the warm start: x clamped into [l, u], y onto the sign cone of its row's sides (y > 0: row at AL)."""
    xp = np.minimum(np.maximum(x, lp["l"]), lp["u"])
    yp = np.where(np.isfinite(lp["AL"]), y, np.minimum(y, 0.0))
    yp = np.where(np.isfinite(lp["AU"]), yp, np.maximum(yp, 0.0))
    return xp, yp


def start_row(lp, x, y, norm_b_org, norm_c_org):
    """The iteration-0 evaluation of a start, restated: (err_Rp, err_Rd, primal_obj, dual_obj, gap) of the projected point with z
    the dual completion of y, and the dual objective of (y, z): y_obj the row side and l / u the column bound each multiplier's
    sign pairs with."""
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    xp, yp = project(lp, x, y)
    AL, AU, l, u, c = lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"]
    w = c - A.T @ yp
    z = np.where(((w > 0) & np.isfinite(l)) | ((w < 0) & np.isfinite(u)), w, 0.0)
    Ax = A @ xp
    yobj = np.where(yp > 0, AL, np.where(yp < 0, AU, np.minimum(np.maximum(Ax, AL), AU)))
    rp = np.maximum(np.minimum(AU - Ax, 0.0), AL - Ax)
    err_rp = np.linalg.norm(rp) / norm_b_org
    err_rd = np.linalg.norm(w - z) / norm_c_org
    pobj = float(c @ xp)
    bz = np.where(z > 0, l, np.where(z < 0, u, 0.0))   # the bound each multiplier leans on (finite wherever z != 0)
    dobj = float(yobj @ yp + bz @ z)
    gap = abs(pobj - dobj) / (1 + abs(pobj) + abs(dobj))
    return dict(err_Rp=err_rp, err_Rd=err_rd, primal_obj=pobj, dual_obj=dobj, gap=gap), xp


def _identical(a, b):
    return a.status == b.status and a.iter == b.iter and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("x", "y", "z"))


# ---- every kernel form: one subprocess per form (the form thresholds are read once per process) --------------------------------
FORM_SCRIPT = r'''
import os, sys
import numpy as np
from scipy import sparse
sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import hprlp, lpgen
from test_gpu_detect import model_of
from test_gpu_warm import start_row, project
form = sys.argv[1]
def planted_on(A, seed):
    A = sparse.csr_matrix(A); A.sum_duplicates(); A.sort_indices()
    lp = lpgen._plant(np.random.default_rng(seed), A)
    lp.update(m=A.shape[0], n=A.shape[1], A=A, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy())
    return lp
if form in ("small", "stream", "all-remainder"):
    m, n = (400, 600) if form == "small" else (3000, 4000)
    lp = lpgen.planted_lp(m, n, 6 * m, 31, values="network")
elif form == "reordered":   # (the shape of tests/test_gpu_detect.py's reordered form)
    m = n = 1_600_000
    rp, ci, v = lpgen.banded_csr(m, n, 10, 16000, 5)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n)); A.sum_duplicates()
    rng = np.random.default_rng(8)
    pr, pc = rng.permutation(m), rng.permutation(n)
    inv = np.empty(n, np.int64); inv[pc] = np.arange(n)
    B = A[pr]; B = sparse.csr_matrix((B.data, inv[B.indices], B.indptr), shape=(m, n))
    lp = planted_on(B, 32)
else:   # tiled forms: a banded matrix
    m, n = 8000, 10000
    rp, ci, v = lpgen.banded_csr(m, n, 8, 1500, 6)
    lp = planted_on(sparse.csr_matrix((v, ci, rp), shape=(m, n)), 33)
model = model_of(lp)
# (1) the iteration-0 evaluation through the solver-level path: a start outside the box with multipliers of the wrong sign
s = hprlp.Solver(model, hprlp.Parameters(max_iter=0, use_presolve=False))
d = s.describe()
expect = {"small": "single-workgroup kernel", "stream": "A: stream kernel", "tiled": "tiled, fused (k_tiled_fused",
          "pieces": "tiled, piece form", "all-remainder": "all-remainder form (k_pb_fused", "reordered": "locality ordering applied"}[form]
assert expect in d, d
if form == "stream":
    assert "A^T: stream kernel" in d and "single-workgroup" not in d, d
s.scale(); lam, _ = s.power_iteration(); s.init(-1.0, lam * 1.01)
rng = np.random.default_rng(5)
x0 = lp["x_star"] + rng.normal(scale=2.0, size=lp["n"])
y0 = lp["y_star"] + rng.normal(scale=1.0, size=lp["m"])
xp, yp = project(lp, x0, y0)
assert (xp != x0).any() and (yp != y0).any()
s.set_start(x0, y0)
sc = s.scalars()
rs = s.run(max_trace=4)
s.close()
want, xp = start_row(lp, x0, y0, sc["norm_b_org"], sc["norm_c_org"])
row = rs.trace[0]
assert rs.status == "ITER_LIMIT" and rs.iter == 0 and row["iter"] == 0, (rs.status, rs.iter)
for k, v in want.items():
    assert abs(row[k] - v) <= 1e-10 * abs(v) + 1e-14, (k, row[k], v)
np.testing.assert_allclose(rs.x, xp, rtol=1e-12, atol=1e-12 * np.abs(xp).max())
# ... y in the caller's numbering (the only check of k_start_in's row permutation), and z = the dual completion of the returned y
# in the caller's units, per element within the start reference's bound plus the allowance for the roundings of scale()
np.testing.assert_allclose(rs.y, yp, rtol=1e-12, atol=1e-12 * np.abs(yp).max())
import evalref as E, startref as S
AT = sparse.csr_matrix(sparse.csr_matrix(lp["A"]).T); AT.sort_indices()
inp = E.unit_inputs(lp, (AT.indptr, AT.indices, AT.data))
zr, ez = S.evaluate_start(*inp, rs.x, rs.y)["z_bar"]
tolz = S.TOL_FACTOR * ez + S.caller_units_z_allowance(inp[1], lp["c"], rs.y, zr, curtis_reid=True)
dz = np.abs(rs.z.astype(E.LD) - zr)
assert np.isfinite(rs.z).all() and (dz <= tolz).all(), (int(np.argmax(dz - tolz)), float((dz / tolz)[tolz > 0].max()))
assert (rs.z > 0).any() and (rs.z == 0).any()
print("z: largest difference / tolerance", float((dz / tolz)[tolz > 0].max()))
# (2) a start that meets the tolerance ends OPTIMAL at iteration 0: the planted optimum, through hprlp_solve_warm
prm = hprlp.Parameters(stop_tol=1e-6, max_iter=20000, use_presolve=False)
r = model.solve_warm(lp["x_star"], lp["y_star"], prm)
assert r.status == "OPTIMAL" and r.iter == 0, (r.status, r.iter, r.residuals)
np.testing.assert_allclose(r.x, lp["x_star"], rtol=1e-12, atol=1e-12 * np.abs(lp["x_star"]).max())
# (3) cold to 1e-8, then warm from the returned point at 1e-6 (the small forms: a cold solve of the large ones takes too long)
if form in ("small", "stream"):
    c8 = model.solve(hprlp.Parameters(stop_tol=1e-8, max_iter=200000, use_presolve=False))
    assert c8.status == "OPTIMAL", c8.status
    w = model.solve_warm(c8.x, c8.y, prm)
    xq, _ = project(lp, c8.x, c8.y)
    assert w.status == "OPTIMAL" and w.iter == 0, (w.status, w.iter, w.residuals)
    np.testing.assert_allclose(w.x, xq, rtol=1e-12, atol=1e-12 * np.abs(xq).max())
print("OK", form, row["err_Rp"], row["err_Rd"], row["gap"], d.splitlines()[0] if d else "")
''' % ROOT


@pytest.mark.parametrize("form", list(FORM_ENV))
def test_start_on_every_kernel_form(gpu, form):
    env = dict(os.environ, **BASE_ENV, **FORM_ENV[form])
    r = subprocess.run([sys.executable, "-c", FORM_SCRIPT, form], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or "OK" not in r.stdout:
        pytest.fail("form %s: exit %d\n%s\n%s" % (form, r.returncode, r.stdout[-800:], r.stderr[-2500:]), pytrace=False)
    print(r.stdout.strip().splitlines()[-1])


# ---- single LP, in process ---------------------------------------------------------------------------------------------------
def test_zero_and_null_starts_are_the_cold_solve(gpu):
    lp = lpgen.planted_lp(1500, 2000, 12000, 9, values="network")
    assert (lp["l"] <= 0).all() and (lp["u"] >= 0).all()   # (zero lies in the box: the projected zero start is zero)
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=1e-6, max_iter=20000, use_presolve=False)
    cold = model.solve(prm)
    zero = model.solve_warm(np.zeros(lp["n"]), np.zeros(lp["m"]), prm)
    null = model.solve_warm(None, None, prm)
    assert cold.status in ("OPTIMAL", "ITER_LIMIT") and cold.iter > 0
    assert _identical(zero, cold), (zero.status, zero.iter, cold.iter)
    assert _identical(null, cold)
    model.free()


def test_presolve_on_warm_start_from_a_presolved_answer(gpu):
    from test_presolve import decorated_lp
    lp = decorated_lp(2)
    model = model_of(lp)
    pre = hprlp.Presolved(model)   # (raises if presolve leaves the model unchanged)
    assert pre.stats["slack_cols"] > 0 and pre.stats["parallel_cols"] > 0, pre.stats
    pre.free()
    a = model.solve(hprlp.Parameters(stop_tol=1e-8, max_iter=100000))
    assert a.status == "OPTIMAL", a.status
    tol = 1e-6
    b = model.solve_warm(a.x, a.y, hprlp.Parameters(stop_tol=tol, max_iter=100000))
    assert b.status == "OPTIMAL", b.status
    k = hprlp.original_kkt(model, b.x, b.y, b.z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 10 * tol, k
    assert b.iter <= a.iter, (b.iter, a.iter)
    print("presolved: cold to 1e-8", a.iter, "iterations; warm to 1e-6", b.iter)
    model.free()


def test_detection_with_a_start_still_gives_the_verdict(gpu):
    lp = lpgen.planted_infeasible_lp(300, 400, 2400, 1)
    model = model_of(lp)
    rng = np.random.default_rng(3)
    r = model.solve_warm(rng.normal(size=lp["n"]), rng.normal(size=lp["m"]),
                         hprlp.Parameters(stop_tol=1e-8, max_iter=50000, use_presolve=False), eps_primal=1e-8, eps_dual=1e-8)
    check_certificate(lp, r, "PRIMAL_INFEASIBLE")
    model.free()


def test_sharded_solver_refuses_a_start(gpu):
    lp = lpgen.planted_lp(300, 400, 2000, 3)
    model = model_of(lp)
    group = hprlp.Solver.local_group(2)
    errs = [None, None]

    def work(rank):
        s = hprlp.Solver.create_local(model, hprlp.Parameters(use_presolve=False), rank, 2, group)
        try:
            s.set_start(np.zeros(lp["n"]), None)
        except RuntimeError as e:
            errs[rank] = str(e)
        s.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    hprlp.Solver.free_local_group(group)
    assert all(e and "one GPU only" in e for e in errs), errs
    model.free()


@pytest.mark.parametrize("seed", [11, 12])
def test_warm_resolve_after_a_small_change_of_c_needs_fewer_iterations(gpu, seed):
    """tools/warm_ab.py probe's setting (measured on an MI355X: cold 6100 / warm 2500 iterations for seed 11, 1600 / 850 for seed
    12); the iterations are deterministic, the margin is what a regression would eat."""
    lp = lpgen.planted_lp(300, 400, 2400, seed, values="network")
    prm = hprlp.Parameters(stop_tol=1e-6, max_iter=500000, use_presolve=False)
    model = model_of(lp)
    base = model.solve(prm)
    assert base.status == "OPTIMAL"
    model.free()
    rng = np.random.default_rng(7)
    lp2 = dict(lp, c=lp["c"] * (1 + 1e-3 * rng.normal(size=lp["n"])))
    model2 = model_of(lp2)
    cold = model2.solve(prm)
    warm = model2.solve_warm(base.x, base.y, prm)
    assert cold.status == warm.status == "OPTIMAL"
    print("seed", seed, "cold", cold.iter, "warm", warm.iter)
    assert warm.iter < 0.75 * cold.iter, (warm.iter, cold.iter)
    model2.free()


# ---- batched --------------------------------------------------------------------------------------------------------------------
def make_batch(lp, B, seed):  # (tests/test_gpu_batched.py's recipe)
    rng = np.random.default_rng(seed)
    m, n = lp["m"], lp["n"]
    Cm = lp["c"][:, None] * (1 + 0.1 * rng.normal(size=(n, B)))
    AU = lp["AU"][:, None] + np.abs(rng.normal(scale=0.1, size=(m, B)))
    AL = np.repeat(lp["AL"][:, None], B, axis=1)
    AL = np.where(np.isfinite(AL), np.minimum(AL, AU), AL)
    L = np.repeat(lp["l"][:, None], B, axis=1)
    U = np.repeat(lp["u"][:, None], B, axis=1)
    U = np.where(np.isfinite(U), U, 50.0)
    return Cm, AL, AU, L, U


def _same_members(a, b, ka, kb):
    return (a["status"][ka] == b["status"][kb] and a["iter"][ka] == b["iter"][kb]
            and all(np.array_equal(a[f][:, ka], b[f][:, kb]) for f in ("x", "y", "z")))


def test_batched_null_start_and_half_warm_batch(gpu):
    lp = lpgen.planted_lp(300, 400, 2400, 7, values="network")
    B = 8
    Cm, AL, AU, L, U = make_batch(lp, B, 2)
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=1e-6, max_iter=50000, use_presolve=False)
    cold = hprlp.solve_batched(model, Cm, AL, AU, L, U, None, prm)
    null = hprlp.solve_batched_warm(model, Cm, AL, AU, L, U, None, None, None, prm)
    assert cold["status"] == ["OPTIMAL"] * B
    for k in range(B):
        assert _same_members(null, cold, k, k), k
    fine = hprlp.solve_batched(model, Cm, AL, AU, L, U, None, hprlp.Parameters(stop_tol=1e-8, max_iter=200000, use_presolve=False))
    assert fine["status"] == ["OPTIMAL"] * B
    warm_k = [0, 2, 4, 6]
    X0, Y0 = np.zeros((lp["n"], B)), np.zeros((lp["m"], B))
    X0[:, warm_k] = fine["x"][:, warm_k]
    Y0[:, warm_k] = fine["y"][:, warm_k]
    half = hprlp.solve_batched_warm(model, Cm, AL, AU, L, U, X0, Y0, None, prm)
    for k in range(B):
        if k in warm_k:
            assert half["status"][k] == "OPTIMAL" and half["iter"][k] == 0, (k, half["status"][k], half["iter"][k])
            xq = np.minimum(np.maximum(X0[:, k], L[:, k]), U[:, k])
            np.testing.assert_allclose(half["x"][:, k], xq, rtol=1e-12, atol=1e-12 * np.abs(xq).max())
        else:
            assert _same_members(half, cold, k, k), (k, half["iter"][k], cold["iter"][k])
    model.free()


def test_batched_config4_warm_resolve_after_a_change_of_c(gpu):
    lp = lpgen.c3_pds20_like()
    B, tol = 64, 1e-4
    Cm, AL, AU, L, U = make_batch(lp, B, 4)
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=tol, max_iter=60000, use_presolve=False)
    r0 = hprlp.solve_batched(model, Cm, AL, AU, L, U, None, prm)
    assert r0["status"] == ["OPTIMAL"] * B
    rng = np.random.default_rng(40)
    C2 = Cm * (1 + 1e-3 * rng.normal(size=Cm.shape))
    r1 = hprlp.solve_batched_warm(model, C2, AL, AU, L, U, r0["x"], r0["y"], None, prm)
    assert r1["status"] == ["OPTIMAL"] * B
    assert (np.asarray(r1["residuals"]) <= tol).all()
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    for k in range(0, B, 9):
        x, y, z = r1["x"][:, k], r1["y"][:, k], r1["z"][:, k]
        rd = C2[:, k] - A.T @ y - z
        assert np.linalg.norm(rd) <= 3 * tol * (1 + np.linalg.norm(C2[:, k])), k
        assert abs(r1["primal_obj"][k] - float(C2[:, k] @ x)) <= 1e-8 * (1 + abs(r1["primal_obj"][k]))
    print("config 4 re-solve: cold iterations", int(np.max(r0["iter"])), "warm", int(np.max(r1["iter"])))
    model.free()
