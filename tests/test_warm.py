"""CPU: the warm start's C ABI (include/hprlp_amd.h: hprlp_solve_warm, hprlp_solve_batched_warm, hprlp_solver_set_start,
hprlp_presolve_forward) and the presolve's forward map, judged by HiGHS and by the original-model KKT metric -- never by the
solver itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import sparse

from conftest import hprlp, lpgen
from test_presolve import decorated_lp, highs, make_model, reduced_arrays, structured_lp

NEW_SYMBOLS = ("hprlp_solve_warm", "hprlp_solve_batched_warm", "hprlp_solver_set_start", "hprlp_presolve_forward")


def small_lp():
    return lpgen.planted_lp(40, 60, 240, 3)


def completion(m, n, rp, ci, v, l, u, c, y):
    """z of the dual completion: w = c - A^T y where its sign has a finite bound to lean on, else 0."""
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))
    w = c - A.T @ y
    keep = ((w > 0) & np.isfinite(l)) | ((w < 0) & np.isfinite(u))
    return np.where(keep, w, 0.0)


def test_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in NEW_SYMBOLS:
        assert s in names, s


def test_solve_warm_without_a_gpu_is_an_error_not_a_crash():
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    lp = small_lp()
    model = make_model(lp)
    for presolve in (False, True):
        r = model.solve_warm(lp["x_star"], lp["y_star"], hprlp.Parameters(use_presolve=presolve, max_iter=100))
        assert r.status == "ERROR" and r.x is None
        assert hprlp.last_error()
        r = model.solve_warm(lp["x_star"], None, hprlp.Parameters(use_presolve=presolve, max_iter=100), eps_primal=1e-8)
        assert r.status == "ERROR" and r.certificate.kind == 0
    model.free()


def test_solve_batched_warm_without_a_gpu_is_an_error_not_a_crash():
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    lp = small_lp()
    model = make_model(lp)
    B = 3
    rep = lambda v: np.repeat(np.asarray(v)[:, None], B, axis=1)
    out = hprlp.solve_batched_warm(model, rep(lp["c"]), rep(lp["AL"]), rep(lp["AU"]), rep(lp["l"]), rep(lp["u"]),
                                   X0=rep(lp["x_star"]), Y0=rep(lp["y_star"]), param=hprlp.Parameters(max_iter=100))
    assert out["status"] == ["ERROR"] * B and out["x"] is None
    assert hprlp.last_error()
    model.free()


def test_solver_set_start_on_a_null_handle_is_an_error():
    L = hprlp.lib()
    x = np.zeros(4)
    assert L.hprlp_solver_set_start(None, x.ctypes.data_as(hprlp.c_dbl_p), None) == -1
    assert "null solver" in hprlp.last_error()


def test_non_finite_start_is_an_error():
    """Checked before any device work: the same answer with or without a GPU."""
    lp = small_lp()
    model = make_model(lp)
    for bad in (np.nan, np.inf, -np.inf):
        x = lp["x_star"].copy()
        x[7] = bad
        # the Python layer refuses it ...
        with pytest.raises(ValueError, match="non-finite"):
            model.solve_warm(x, None)
        # ... and so does the C entry on its own
        cp = hprlp.Parameters(use_presolve=False, max_iter=10).to_c()
        res = hprlp.lib().hprlp_solve_warm(model._ptr, C.byref(cp), x.ctypes.data_as(hprlp.c_dbl_p), None, None, None)
        r = hprlp.Results(res, model.m, model.n)
        assert r.status == "ERROR" and r.x is None
        assert "x0[7] is not finite" in hprlp.last_error()
    y = lp["y_star"].copy()
    y[0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        model.solve_warm(None, y)
    model.free()


def test_wrong_lengths_are_errors():
    lp = small_lp()
    model = make_model(lp)
    with pytest.raises(ValueError, match="length"):
        model.solve_warm(np.zeros(lp["n"] - 1), None)
    with pytest.raises(ValueError, match="length"):
        model.solve_warm(None, np.zeros(lp["m"] + 1))
    with pytest.raises(ValueError, match="length"):
        model.solve_warm(np.zeros((lp["n"], 1)), None)
    B = 2
    rep = lambda v: np.repeat(np.asarray(v)[:, None], B, axis=1)
    with pytest.raises(ValueError, match="shape"):
        hprlp.solve_batched_warm(model, rep(lp["c"]), rep(lp["AL"]), rep(lp["AU"]), rep(lp["l"]), rep(lp["u"]),
                                 X0=np.zeros((lp["n"], B + 1)))
    with pytest.raises(ValueError, match="shape"):
        hprlp.solve_batched_warm(model, rep(lp["c"]), rep(lp["AL"]), rep(lp["AU"]), rep(lp["l"]), rep(lp["u"]),
                                 Y0=np.zeros((lp["m"] - 1, B)))
    X0 = np.zeros((lp["n"], B))
    X0[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        hprlp.solve_batched_warm(model, rep(lp["c"]), rep(lp["AL"]), rep(lp["AU"]), rep(lp["l"]), rep(lp["u"]), X0=X0)
    model.free()


def test_forward_lengths_and_zeros():
    lp = structured_lp(3)
    model = make_model(lp)
    pre = hprlp.Presolved(model)
    xr, yr = pre.forward(np.zeros(lp["n"]), np.zeros(lp["m"]))
    assert xr.shape == (pre.reduced.n,) and yr.shape == (pre.reduced.m,)
    assert pre.reduced.n < lp["n"] and pre.reduced.m < lp["m"]
    # (no slack column of this LP that goes carries a cost: nothing moves out of a multiplier, zeros map to zeros; a costed one
    # moves c_j / a out of its row's multiplier even at y = 0 -- test_forward_map_is_more_than_a_restriction)
    assert not xr.any() and not yr.any()
    with pytest.raises(ValueError):
        pre.forward(np.zeros(lp["n"] + 1), np.zeros(lp["m"]))
    L = hprlp.lib()
    assert L.hprlp_presolve_forward(None, None, None, None, None) == -1
    pre.free(); model.free()


def forward_kkt(lp):
    """forward() of the HiGHS optimum, and the reduced model's KKT metric at its image (z: the dual completion)."""
    model = make_model(lp)
    f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    pre = hprlp.Presolved(model)
    xr, yr = pre.forward(x0, y0)
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    zr = completion(rm, rn, rp, ci, v, l, u, c, yr)
    k = hprlp.original_kkt(pre.reduced, xr, yr, zr)
    stats = dict(pre.stats)
    err = max(k["primal_feas"], k["dual_feas"], k["gap"])
    obj = k["primal_obj"]
    pre.free(); model.free()
    return err, stats, obj, f0


def slack_lp(seed):
    """tests/test_presolve.py's equality-form LP with slack columns (some with a cost), rebuilt from the same recipe."""
    rng = np.random.default_rng(seed)
    m0, n0 = 35, 60
    base = lpgen.planted_lp(m0, n0, 220, seed)
    A = sparse.csr_matrix((base["values"], base["colind"], base["rowptr"]), shape=(m0, n0))
    AL, AU = base["AL"].copy(), base["AU"].copy()
    ineq = np.where(~(np.isfinite(AL) & (AL == AU)))[0]
    cols, l_new, u_new = [], [], []
    for i in ineq:
        a = float(rng.choice([1.0, -1.0, 2.5, -0.5]))
        col = sparse.lil_matrix((m0, 1))
        col[i, 0] = a
        cols.append(col.tocsr())
        b = AU[i] if np.isfinite(AU[i]) else AL[i]
        lo, hi = sorted(((b - AU[i]) / a, (b - AL[i]) / a))
        l_new.append(lo); u_new.append(hi)
        AL[i] = AU[i] = b
    A2 = sparse.hstack([A] + cols).tocsr()
    A2.sort_indices()
    l = np.concatenate([base["l"], l_new]); u = np.concatenate([base["u"], u_new])
    c = np.concatenate([base["c"], np.zeros(len(ineq))])
    for t in range(0, len(ineq), 3):
        c[n0 + t] = 0.3 if np.isfinite(l[n0 + t]) else (-0.3 if np.isfinite(u[n0 + t]) else 0.0)
    return dict(m=m0, n=A2.shape[1], rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
                AL=AL, AU=AU, l=l, u=u, c=c)


FORWARD_LPS = {
    "structured 1": lambda: structured_lp(1),
    "structured 3": lambda: structured_lp(3),
    "slack 1": lambda: slack_lp(1),
    "slack 2": lambda: slack_lp(2),
    "decorated 1": lambda: decorated_lp(1),
    "decorated 2": lambda: decorated_lp(2),
}


@pytest.mark.parametrize("name", sorted(FORWARD_LPS))
def test_forward_map_of_the_optimum_is_optimal_for_the_reduced_model(name):
    err, stats, obj, f0 = forward_kkt(FORWARD_LPS[name]())
    assert err <= 1e-9, (name, err, stats)
    assert abs(obj - f0) <= 1e-8 * (1 + abs(f0)), (obj, f0)


def test_forward_lps_cover_folded_columns_and_slack_substitutions():
    """At least one LP above folds a parallel column and one substitutes a costed slack: the two places where the forward map is
    more than a restriction."""
    seen = {k: 0 for k in ("parallel_cols", "slack_cols", "parallel_rows")}
    for name, gen in FORWARD_LPS.items():
        pre = hprlp.Presolved(make_model(gen()))
        for k in seen:
            seen[k] += pre.stats[k]
        pre.free()
    assert all(v > 0 for v in seen.values()), seen


def test_forward_map_is_more_than_a_restriction():
    """A restriction maps ones to ones and zeros to zeros.  A folded parallel column's kept entry carries 1 + lambda, a folded
    parallel row's multiplier 1 + lambda, and a costed slack moves c_j / a out of its row's multiplier even at y = 0."""
    lp = decorated_lp(1)
    pre = hprlp.Presolved(make_model(lp))
    assert pre.stats["parallel_cols"] > 0 and pre.stats["parallel_rows"] > 0
    xr, _ = pre.forward(np.ones(lp["n"]), np.zeros(lp["m"]))
    _, yr = pre.forward(np.zeros(lp["n"]), np.ones(lp["m"]))
    assert np.sum(xr != 1.0) >= 1 and np.sum(yr != 1.0) >= 1, (xr, yr)
    pre.free()
    lp = slack_lp(1)
    pre = hprlp.Presolved(make_model(lp))
    assert pre.stats["slack_cols"] > 0
    xr, yr = pre.forward(np.zeros(lp["n"]), np.zeros(lp["m"]))
    assert not xr.any() and yr.any()
    pre.free()
