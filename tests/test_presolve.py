"""Presolve / postsolve around solve() (hpr-lp-c_amd/csrc/presolve.cpp).

CPU tests: the reduced model and the postsolve map are checked with an exact LP solver (HiGHS via scipy) --
same optimum as the original, and the postsolved primal-dual triple satisfies the KKT conditions of the
ORIGINAL model.  The presolver the reference vendors (PSLP v0.0.8) is the reference point on some of the same LPs:
what it made of them is stored in tests/golden/pslp_reference.json (tests/golden/make_pslp_golden.py).
GPU test: solve() with use_presolve on and off gives the same optimum in the original dimensions."""
import json
import os

import numpy as np
import pytest
from scipy import sparse
from scipy.optimize import linprog

from conftest import hprlp, lpgen

INF = np.inf
PSLP_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pslp_reference.json")


def pslp_record(key, lp):
    """PSLP's status, reduced size and postsolved solution for `lp` (tests/golden/make_pslp_golden.py), checked to be of this LP."""
    with open(PSLP_GOLDEN) as f:
        rec = json.load(f)[key]
    assert (rec["m"], rec["n"], rec["nnz"]) == (lp["m"], lp["n"], len(lp["values"])), key
    return rec


def highs(m, n, rp, ci, v, AL, AU, l, u, c):
    """Exact optimum and duals in our convention (z = c - A^T y, y_i > 0 <=> row at AL)."""
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))
    eq = np.isfinite(AL) & (AL == AU)
    up = np.isfinite(AU) & ~eq
    lo = np.isfinite(AL) & ~eq
    A_ub = sparse.vstack([A[up], -A[lo]]) if (up.any() or lo.any()) else None
    b_ub = np.concatenate([AU[up], -AL[lo]]) if A_ub is not None else None
    A_eq = A[eq] if eq.any() else None
    b_eq = AL[eq] if eq.any() else None
    bounds = [(None if not np.isfinite(a) else a, None if not np.isfinite(b) else b) for a, b in zip(l, u)]
    # (HiGHS' own presolve off and tight tolerances: with the defaults it calls a few of the reduced models of the sweeps
    # infeasible or "unknown" that it solves to optimality without its presolve, and its 1e-7 feasibility tolerance shows
    # up as 1e-5 differences in the optimum of degenerate LPs)
    r = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs",
                options=dict(presolve=False, primal_feasibility_tolerance=1e-9, dual_feasibility_tolerance=1e-9))
    assert r.status == 0, r.message
    y = np.zeros(m)
    if A_ub is not None:
        mu = r.ineqlin.marginals
        nu_ = int(up.sum())
        y[up] += mu[:nu_]
        y[lo] += -mu[nu_:]
    if A_eq is not None:
        y[eq] = r.eqlin.marginals
    z = r.lower.marginals + r.upper.marginals
    return r.fun, r.x, y, z


def structured_lp(seed, m0=60, n0=90):
    """A planted LP decorated with everything the presolver removes: fixed columns, singleton rows (some binding),
    empty rows, redundant rows, empty columns."""
    rng = np.random.default_rng(seed)
    base = lpgen.planted_lp(m0, n0, 6 * m0, seed)
    A = sparse.csr_matrix((base["values"], base["colind"], base["rowptr"]), shape=(m0, n0)).tolil()
    AL, AU = base["AL"].copy(), base["AU"].copy()
    l, u, c = base["l"].copy(), base["u"].copy(), base["c"].copy()
    xs = base["x_star"]
    # fixed columns at their planted value
    for j in rng.choice(n0, size=6, replace=False):
        l[j] = u[j] = xs[j]
    rows = [A]
    extra_AL, extra_AU = [], []

    def add_row(cols, vals, lo, hi):
        r = sparse.lil_matrix((1, n0))
        for cc, vv in zip(cols, vals):
            r[0, cc] = vv
        rows.append(r)
        extra_AL.append(lo)
        extra_AU.append(hi)

    # singleton rows: loose ones, ones that are active at the planted optimum, and equalities
    for j in rng.choice(n0, size=8, replace=False):
        a = rng.choice([-2.0, 0.5, 3.0])
        kind = rng.integers(0, 3)
        if kind == 0:
            add_row([j], [a], -INF if a > 0 else a * (xs[j] + 5.0), a * (xs[j] + 5.0) if a > 0 else INF)  # x_j <= xs+5
        elif kind == 1:
            t = xs[j]  # x_j >= planted value: active at the optimum, which stays optimal
            add_row([j], [a], a * t if a > 0 else -INF, INF if a > 0 else a * t)
        else:
            add_row([j], [a], a * xs[j], a * xs[j])
    add_row([], [], -1.0, 2.0)  # empty row, consistent
    add_row([], [], -INF, 0.0)
    # redundant rows: activity range inside the row bounds (boxed columns only)
    boxed = np.where(np.isfinite(l) & np.isfinite(u))[0]
    if len(boxed) >= 3:
        cols = boxed[:3]
        vals = np.array([1.0, -2.0, 0.5])
        lo_act = sum(min(a * l[j], a * u[j]) for a, j in zip(vals, cols))
        up_act = sum(max(a * l[j], a * u[j]) for a, j in zip(vals, cols))
        add_row(cols, vals, lo_act - 1.0, up_act + 1.0)
        add_row(cols, vals, -INF, up_act)
    A2 = sparse.vstack(rows).tocsr()
    # empty columns appended: positive cost at a finite lower bound, negative cost at a finite upper bound, zero cost
    extra_cols = 3
    A2 = sparse.hstack([A2, sparse.csr_matrix((A2.shape[0], extra_cols))]).tocsr()
    l = np.concatenate([l, [1.0, -INF, -INF]])
    u = np.concatenate([u, [INF, 4.0, INF]])
    c = np.concatenate([c, [2.0, -1.5, 0.0]])
    A2.sort_indices()
    AL = np.concatenate([AL, extra_AL])
    AU = np.concatenate([AU, extra_AU])
    m, n = A2.shape
    return dict(m=m, n=n, rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
                AL=AL, AU=AU, l=l, u=u, c=c)


def make_model(lp):
    return hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"],
                                lp["u"], lp["c"])


def reduced_arrays(pre):
    red = pre.reduced
    rp, ci, v = red.csr()
    vec = red.vectors()
    return red.m, red.n, rp, ci, v, vec["AL"], vec["AU"], vec["l"], vec["u"], vec["c"]


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_reduced_model_has_same_optimum_and_postsolve_satisfies_original_kkt(seed):
    lp = structured_lp(seed)
    model = make_model(lp)
    f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    pre = hprlp.Presolved(model)
    st = pre.stats
    assert st["m"] < lp["m"] and st["n"] < lp["n"]
    assert st["fixed_cols"] >= 6 and st["singleton_rows"] >= 8 and st["empty_rows"] >= 2 and st["empty_cols"] >= 3
    # (the two redundant rows turn into singleton rows when two of their three columns happen to be fixed)
    assert st["redundant_rows"] + st["singleton_rows"] >= 10 and lp["m"] - st["m"] >= 12
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0))
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert k["primal_feas"] <= 1e-9 and k["dual_feas"] <= 1e-9 and k["gap"] <= 1e-9, k
    assert abs(k["primal_obj"] - f0) <= 1e-8 * (1 + abs(f0))
    # the KKT metric itself: the exact solver's own primal-dual pair passes it on the original model
    k0 = hprlp.original_kkt(model, x0, y0, z0)
    assert max(k0["primal_feas"], k0["dual_feas"], k0["gap"]) <= 1e-9
    pre.free(); model.free()


def test_binding_singleton_row_gets_the_multiplier():
    """min 2*x0 + x1  s.t.  x0 + x1 >= 2 (row 0),  2*x0 >= 3 (row 1, singleton, binding),  x >= 0.
    Optimum x = (1.5, 0.5), y = (1, 0.5), z = 0: the reduced cost that column 0 shows at its presolved bound
    1.5 belongs to the singleton row."""
    rp = np.array([0, 2, 3], np.int32); ci = np.array([0, 1, 0], np.int32); v = np.array([1.0, 1.0, 2.0])
    model = hprlp.Model.from_csr(2, 2, rp, ci, v, [2.0, 3.0], [INF, INF], [0.0, 0.0], [INF, INF], [2.0, 1.0])
    pre = hprlp.Presolved(model)
    assert pre.stats["singleton_rows"] == 1 and pre.reduced.m == 1
    assert pre.reduced.vectors()["l"][0] == 1.5
    rm, rn, rp2, ci2, v2, AL, AU, l, u, c = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp2, ci2, v2, AL, AU, l, u, c)
    np.testing.assert_allclose(zr, [1.0, 0.0], atol=1e-12)
    x, y, z = pre.postsolve(xr, yr, zr)
    np.testing.assert_allclose(x, [1.5, 0.5], atol=1e-12)
    np.testing.assert_allclose(y, [1.0, 0.5], atol=1e-12)
    np.testing.assert_allclose(z, [0.0, 0.0], atol=1e-12)
    pre.free(); model.free()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_dual_fixing(seed):
    """Columns whose cost and rows all push them to one bound (PSLP's Simple_dual_fix): slack-like columns appended to a
    planted LP are fixed at that bound, the optimum is unchanged and the postsolved triple passes the original KKT."""
    rng = np.random.default_rng(seed)
    base = lpgen.planted_lp(40, 70, 240, seed)
    m0, n0 = 40, 70
    A = sparse.csr_matrix((base["values"], base["colind"], base["rowptr"]), shape=(m0, n0)).tolil()
    AL, AU = base["AL"].copy(), base["AU"].copy()
    only_up = np.where(~np.isfinite(AL) & np.isfinite(AU))[0]
    only_lo = np.where(np.isfinite(AL) & ~np.isfinite(AU))[0]
    if len(only_lo) < 2:  # the generator makes equalities and <= rows: turn two <= rows around (sign flip keeps them valid)
        for i in only_up[:2]:
            A[i, :] = -A[i, :]
            AL[i], AU[i] = -AU[i], INF
        only_up = only_up[2:]
        only_lo = np.where(np.isfinite(AL) & ~np.isfinite(AU))[0]
    assert len(only_up) >= 2 and len(only_lo) >= 2
    new_cols = sparse.lil_matrix((m0, 3))
    # column n0: cost > 0, +entries in <= rows and a -entry in a >= row: lowering it can only help  -> lower bound 0.3
    new_cols[only_up[0], 0] = 1.5; new_cols[only_up[1], 0] = 0.25; new_cols[only_lo[0], 0] = -2.0
    # column n0+1: cost < 0, +entry in a >= row and -entry in a <= row: raising it can only help   -> upper bound 2.5
    new_cols[only_lo[1], 1] = 1.0; new_cols[only_up[0], 1] = -0.5
    # column n0+2: zero cost, +entry in a <= row, lower bound only                                 -> lower bound -1
    new_cols[only_up[1], 2] = 3.0
    A2 = sparse.hstack([A.tocsr(), new_cols.tocsr()]).tocsr()
    A2.sort_indices()
    l = np.concatenate([base["l"], [0.3, -INF, -1.0]])
    u = np.concatenate([base["u"], [INF, 2.5, INF]])
    c = np.concatenate([base["c"], [0.7, -0.4, 0.0]])
    # keep the planted point feasible: shift the row sides by the new columns at their dual-fixed values
    shift = A2[:, n0:] @ np.array([0.3, 2.5, -1.0])
    AL, AU = AL + shift, AU + shift
    lp = dict(m=m0, n=n0 + 3, rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
              AL=AL, AU=AU, l=l, u=u, c=c)
    model = make_model(lp)
    f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], AL, AU, l, u, c)
    pre = hprlp.Presolved(model)
    assert pre.stats["dual_fixed_cols"] >= 3 and pre.stats["n"] <= n0
    rm, rn, rp, ci, v, rAL, rAU, rl, ru, rc = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, rAL, rAU, rl, ru, rc)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0))
    x, y, z = pre.postsolve(xr, yr, zr)
    np.testing.assert_allclose(x[n0:], [0.3, 2.5, -1.0], atol=0)
    k = hprlp.original_kkt(model, x, y, z)
    assert k["primal_feas"] <= 1e-9 and k["dual_feas"] <= 1e-9 and k["gap"] <= 1e-9, k
    pre.free(); model.free()


@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_slack_columns_of_equality_rows(seed):
    """An LP in equality form with explicit slack / surplus / free columns (some of them with a cost, some boxed): every
    such column appears in one equality row only and is substituted out (PSLP's StonCols, equality case); the row turns
    into a ranged row, the optimum is unchanged and the postsolved triple passes the original KKT."""
    rng = np.random.default_rng(seed)
    m0, n0 = 35, 60
    base = lpgen.planted_lp(m0, n0, 220, seed)
    A = sparse.csr_matrix((base["values"], base["colind"], base["rowptr"]), shape=(m0, n0))
    AL, AU = base["AL"].copy(), base["AU"].copy()
    ineq = np.where(~(np.isfinite(AL) & (AL == AU)))[0]
    assert len(ineq) >= 6
    cols, l_new, u_new, c_new = [], [], [], []
    for t, i in enumerate(ineq):
        a = float(rng.choice([1.0, -1.0, 2.5, -0.5]))
        col = sparse.lil_matrix((m0, 1))
        col[i, 0] = a
        cols.append(col.tocsr())
        # row i:  AL <= r.x <= AU   becomes   r.x + a s = b  with  s in [ (b - AU)/a , (b - AL)/a ]  (sorted)
        b = AU[i] if np.isfinite(AU[i]) else AL[i]
        lo, hi = (b - AU[i]) / a, (b - AL[i]) / a
        lo, hi = min(lo, hi), max(lo, hi)
        l_new.append(lo); u_new.append(hi)
        c_new.append(0.0)  # costs on a third of them are set below
        AL[i] = AU[i] = b
    A2 = sparse.hstack([A] + cols).tocsr()
    A2.sort_indices()
    l = np.concatenate([base["l"], l_new]); u = np.concatenate([base["u"], u_new]); c = np.concatenate([base["c"], c_new])
    # slack columns WITH a cost: add cost c_s to slack s and subtract c_s/a * (row) from nothing -- instead perturb directly
    # and let the exact solver be the judge (the LP stays feasible and bounded: boxed or one-sided slacks with the cost
    # pointing at the finite side)
    k = n0
    for t in range(len(ineq)):
        if t % 3 == 0:
            if np.isfinite(l[k + t]):
                c[k + t] = 0.3
            elif np.isfinite(u[k + t]):
                c[k + t] = -0.3
    lp = dict(m=m0, n=A2.shape[1], rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
              AL=AL, AU=AU, l=l, u=u, c=c)
    model = make_model(lp)
    f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], AL, AU, l, u, c)
    pre = hprlp.Presolved(model)
    # zero-cost slacks always go; costed ones only behind a pivot that is not small for its row (presolve.cpp kSlackPivot)
    assert pre.stats["slack_cols"] >= int(np.sum(c[n0:] == 0.0)) - 1 and pre.stats["slack_cols"] > len(ineq) // 2, pre.stats
    rm, rn, rp, ci, v, rAL, rAU, rl, ru, rc = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, rAL, rAU, rl, ru, rc)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0))
    x, y, z = pre.postsolve(xr, yr, zr)
    kk = hprlp.original_kkt(model, x, y, z)
    assert kk["primal_feas"] <= 1e-9 and kk["dual_feas"] <= 1e-9 and kk["gap"] <= 1e-9, kk
    assert abs(kk["primal_obj"] - f0) <= 1e-8 * (1 + abs(f0))
    pre.free(); model.free()


def decorated_lp(seed):
    """structured_lp() plus slack columns on some inequality rows (turned into equalities, a third of the slacks with a
    cost) and slack-like columns that dual fixing removes -- every reduction of the presolver in one model, so that the
    undo sequence mixes them."""
    rng = np.random.default_rng(1000 + seed)
    lp = structured_lp(seed, m0=30 + seed % 7, n0=45 + seed % 11)
    m, n = lp["m"], lp["n"]
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(m, n)).tolil()
    AL, AU, l, u, c = lp["AL"].copy(), lp["AU"].copy(), lp["l"].copy(), lp["u"].copy(), lp["c"].copy()
    nnz_row = np.diff(lp["rowptr"])
    ineq = [i for i in range(m) if not (np.isfinite(AL[i]) and AL[i] == AU[i]) and nnz_row[i] >= 2
            and (np.isfinite(AL[i]) or np.isfinite(AU[i]))]
    rng.shuffle(ineq)
    new_cols, nl, nu, nc = [], [], [], []
    for t, i in enumerate(ineq[:6]):  # slack columns
        a = float(rng.choice([1.0, -1.0, 2.0, -0.5]))
        b = AU[i] if np.isfinite(AU[i]) else AL[i]
        lo, hi = sorted(((b - AU[i]) / a, (b - AL[i]) / a))
        col = sparse.lil_matrix((m, 1)); col[i, 0] = a
        new_cols.append(col.tocsr()); nl.append(lo); nu.append(hi)
        cost = 0.0
        if t % 3 == 0:
            cost = 0.25 if np.isfinite(lo) else (-0.25 if np.isfinite(hi) else 0.0)
        nc.append(cost)
        AL[i] = AU[i] = b
    one_sided = [i for i in ineq[6:] if np.isfinite(AL[i]) != np.isfinite(AU[i])]
    for i in one_sided[:3]:  # dual-fix columns: cost and the row both push them to the finite bound
        only_up = np.isfinite(AU[i])
        a = float(rng.choice([0.5, 1.5]))
        col = sparse.lil_matrix((m, 1)); col[i, 0] = a if only_up else -a
        new_cols.append(col.tocsr()); nl.append(0.4); nu.append(INF); nc.append(0.6)
        shift = (a if only_up else -a) * 0.4
        AL[i] += shift; AU[i] += shift
    for i in one_sided[3:6] + ineq[:2]:  # zero-cost columns that live in one row only (inequality, ranged or equality)
        a = float(rng.choice([1.0, -2.0]))
        col = sparse.lil_matrix((m, 1)); col[i, 0] = a
        new_cols.append(col.tocsr()); nl.append(0.0); nu.append(float(rng.choice([1.5, INF]))); nc.append(0.0)
    for t, i in enumerate(one_sided[6:8]):  # free columns with a cost that pushes them against the row's finite side
        only_up = np.isfinite(AU[i])
        a = float(rng.choice([1.0, 2.0]))
        col = sparse.lil_matrix((m, 1)); col[i, 0] = a
        # row <= AU: raising x_j is blocked by the row, so a negative cost is bounded; row >= AL: positive cost
        new_cols.append(col.tocsr()); nl.append(-INF); nu.append(INF); nc.append(-0.35 if only_up else 0.35)
    Acsc = A.tocsc()
    for t, j in enumerate([j for j in range(n) if Acsc.indptr[j + 1] - Acsc.indptr[j] >= 2][: 3 + seed % 2]):
        lam = float(rng.choice([2.0, -1.0, 0.5]))  # parallel columns: lam x column j, cost lam c_j, a finite box around 0
        new_cols.append((Acsc[:, j] * lam).tocsr()); nl.append(-0.5 if t % 2 else 0.0); nu.append(1.2); nc.append(lam * c[j])
    A2 = sparse.hstack([A.tocsr()] + new_cols).tocsr() if new_cols else A.tocsr()
    # parallel rows: multiples of existing rows, looser on both sides or with one side only
    picks = [i for i in range(m) if A2.indptr[i + 1] - A2.indptr[i] >= 3][: 4 + seed % 3]
    extra_rows, eAL, eAU = [], [], []
    for t, i in enumerate(picks):
        lam = float(rng.choice([2.0, -0.5, 1.0, -3.0]))
        lo_i, up_i = AL[i], AU[i]
        if t % 2 == 0:   # looser copy of the row (the original stays the binding one)
            lo_n, up_n = (lo_i - 0.4 if np.isfinite(lo_i) else -INF), (up_i + 0.7 if np.isfinite(up_i) else INF)
        else:            # one side tighter by nothing, the other missing: the sides get split between the two rows
            lo_n, up_n = lo_i, INF
        a, b = lam * lo_n, lam * up_n
        extra_rows.append(A2[i] * lam); eAL.append(min(a, b)); eAU.append(max(a, b))
    # forcing rows: over columns that sit at their lower bound in the planted point (so the LP stays feasible), the least
    # (or, with negative coefficients, the largest) activity the box allows is made the row's only feasible value
    m0, n0 = 30 + seed % 7, 45 + seed % 11
    xs = lpgen.planted_lp(m0, n0, 6 * m0, seed)["x_star"]
    at_low = [j for j in range(n0) if np.isfinite(l[j]) and xs[j] == l[j] and u[j] > l[j]]
    for t in range(min(2, len(at_low) // 3)):
        cols = at_low[3 * t: 3 * t + 3]
        sign = 1.0 if (seed + t) % 2 == 0 else -1.0
        vals = sign * np.array([1.0, 2.0, 0.5])
        act = float(sum(a * l[j] for a, j in zip(vals, cols)))
        r = sparse.lil_matrix((1, A2.shape[1]))
        for a, j in zip(vals, cols):
            r[0, j] = a
        extra_rows.append(r.tocsr())
        if sign > 0:
            eAL.append(-INF); eAU.append(act)   # activity <= its own minimum
        else:
            eAL.append(act); eAU.append(INF)    # activity >= its own maximum
    if extra_rows:
        A2 = sparse.vstack([A2] + extra_rows).tocsr()
        AL, AU = np.concatenate([AL, eAL]), np.concatenate([AU, eAU])
    A2.sort_indices()
    return dict(m=A2.shape[0], n=A2.shape[1], rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
                AL=AL, AU=AU, l=np.concatenate([l, nl]), u=np.concatenate([u, nu]), c=np.concatenate([c, nc]))


def test_randomised_sweep_of_all_reductions():
    """40 decorated LPs: the reduced model has the original optimum and the postsolved triple satisfies the KKT conditions
    of the original model -- the undo sequence is exercised with every mix of reductions the generator produces."""
    seen = dict(fixed_cols=0, empty_cols=0, singleton_rows=0, empty_rows=0, redundant_rows=0, dual_fixed_cols=0, slack_cols=0,
                parallel_rows=0, parallel_cols=0, forcing_rows=0)
    for seed in range(40):
        lp = decorated_lp(seed)
        try:
            f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
        except AssertionError:
            continue  # (a decoration made this one unbounded or infeasible: not what the sweep is about)
        model = make_model(lp)
        pre = hprlp.Presolved(model)
        for k in seen:
            seen[k] += pre.stats[k]
        rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
        fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
        assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0)), seed
        x, y, z = pre.postsolve(xr, yr, zr)
        k = hprlp.original_kkt(model, x, y, z)
        assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-8, (seed, k, pre.stats)
        pre.free(); model.free()
    assert all(v > 0 for v in seen.values()), seen


def doubleton_lp(seed, m0=50, n0=80, pairs=10, free_share=0.0):
    """A planted LP plus `pairs` equality rows a x_j + b x_k = a xs_j + b xs_k over columns that also sit in other rows
    (some chained: the kept column of one pair is a member of the next); with free_share > 0 some columns lose their
    finite bounds, so that rows imply them."""
    rng = np.random.default_rng(seed)
    base = lpgen.planted_lp(m0, n0, 6 * m0, seed)
    A = sparse.csr_matrix((base["values"], base["colind"], base["rowptr"]), shape=(m0, n0)).tolil()
    AL, AU = list(base["AL"]), list(base["AU"])
    l, u, c = base["l"].copy(), base["u"].copy(), base["c"].copy()
    xs = base["x_star"]
    # columns strictly inside their box at the planted optimum first (a pair of columns on their bounds is a forcing row)
    inside = np.flatnonzero((xs > l + 1e-3) & (xs < u - 1e-3))
    others = np.setdiff1d(np.arange(n0), inside)
    cols = np.concatenate([rng.permutation(inside), rng.permutation(others)])[:pairs + 1]
    rows = [A]
    for q in range(pairs):
        j, k = int(cols[q]), int(cols[q + 1])  # chained: k of this pair is j of the next
        a, b = rng.choice([1.0, -2.0, 0.5, 3.0]), rng.choice([1.0, -1.0, 4.0, -0.25])
        r = sparse.lil_matrix((1, n0))
        r[0, j], r[0, k] = a, b
        rows.append(r)
        rhs = a * xs[j] + b * xs[k]
        AL.append(rhs); AU.append(rhs)
    if free_share > 0:
        pick = rng.random(n0) < free_share
        u[pick & (xs < u)] = INF          # planted value is not on that bound: the optimum stays an optimum
        l[pick & (xs > l) & (rng.random(n0) < 0.5)] = -INF
    A2 = sparse.vstack(rows).tocsr()
    A2.sort_indices()
    return dict(m=A2.shape[0], n=n0, rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), values=A2.data.copy(),
                AL=np.array(AL), AU=np.array(AU), l=l, u=u, c=c)


@pytest.mark.parametrize("seed", [31, 32, 33, 34, 35, 36])
def test_doubleton_equations(seed):
    """Doubleton equality rows are substituted out (the matrix entries change: PSLP DtonsEq): the reduced model keeps the
    optimum, and the postsolved triple -- x_j from the row, the row's multiplier from the reduced costs -- satisfies the
    KKT conditions of the original model."""
    lp = doubleton_lp(seed)
    f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    model = make_model(lp)
    pre = hprlp.Presolved(model)
    # (a pair whose column another reduction fixed first is gone as a singleton row instead)
    assert pre.stats["doubleton_rows"] >= 8, pre.stats
    assert pre.reduced.m <= lp["m"] - 8 and pre.reduced.n <= lp["n"] - 8
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0))
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-8, (k, pre.stats)
    assert abs(k["primal_obj"] - f0) <= 1e-8 * (1 + abs(f0))
    pre.free(); model.free()


@pytest.mark.parametrize("seed,free_share", [(45, 0.5), (44, 0.5), (7, 0.3)])
def test_doubleton_chain_at_gpu_test_size(seed, free_share):
    """Regression: at 230 x 320 with 30 chained pairs a substitution left a merged coefficient of 1.8e-10 in an equality row; the
    forcing-row test (a tolerance test) then pinned that column to a bound 11 away from its value and the reduced model lost
    the optimum by 1e4.  Such near-cancelling substitutions are refused now, and forcing rows with entries below 1e-6 of their
    largest one are left alone."""
    lp = doubleton_lp(seed, m0=200, n0=320, pairs=30, free_share=free_share)
    f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    model = make_model(lp)
    pre = hprlp.Presolved(model)
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-7 * (1 + abs(f0)), pre.stats
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-7, (k, pre.stats)
    pre.free(); model.free()


def test_doubleton_bound_transfer_moves_the_multiplier():
    """min x0 + x1  s.t.  x0 - 2 x1 = 0 (doubleton),  x0 + x1 + x2 >= 1,  0 <= x0 <= 0.3,  0 <= x1 <= 10,  0 <= x2 <= 10, cost
    of x2 = 5.  x0 = 2 x1 and x0 <= 0.3 cap x1 at 0.15: optimum x = (0.3, 0.15, 0.55).  Whichever column is substituted, the
    bound that stops the pair is x0's: after postsolve x0 carries the reduced cost and x1 none."""
    rp = np.array([0, 2, 5], np.int32); ci = np.array([0, 1, 0, 1, 2], np.int32); v = np.array([1.0, -2.0, 1.0, 1.0, 1.0])
    AL, AU = np.array([0.0, 1.0]), np.array([0.0, INF])
    l, u, c = np.zeros(3), np.array([0.3, 10.0, 10.0]), np.array([1.0, 1.0, 5.0])
    f0, x0, y0, z0 = highs(2, 3, rp, ci, v, AL, AU, l, u, c)
    np.testing.assert_allclose(x0, [0.3, 0.15, 0.55], atol=1e-12)
    model = hprlp.Model.from_csr(2, 3, rp, ci, v, AL, AU, l, u, c)
    pre = hprlp.Presolved(model)
    assert pre.stats["doubleton_rows"] == 1
    rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc)
    x, y, z = pre.postsolve(xr, yr, zr)
    np.testing.assert_allclose(x, x0, atol=1e-12)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-10, k
    assert z[1] == 0.0 and z[0] < 0.0   # x0 sits on its upper bound, x1 is strictly inside its box
    np.testing.assert_allclose(z, c - sparse.csr_matrix((v, ci, rp), shape=(2, 3)).T @ y, atol=1e-12)
    pre.free(); model.free()


@pytest.mark.parametrize("seed", [41, 42, 43, 44])
def test_bound_propagation_feeds_the_reductions(seed):
    """Columns without finite bounds get the bounds their rows imply (PSLP Primal_propagation, infinite bounds only); the box is
    kept only when the next round removes something with it.  Optimum and original KKT as everywhere."""
    lp = doubleton_lp(seed, pairs=4, free_share=0.5)
    try:
        f0, x0, y0, z0 = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    except AssertionError:
        pytest.skip("unbounded after freeing columns")
    model = make_model(lp)
    pre = hprlp.Presolved(model)
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-7 * (1 + abs(f0))
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-7, (k, pre.stats)
    pre.free(); model.free()


def test_bound_propagation_alone_is_not_a_reduction():
    """x0 + 2 x1 <= 10, 3 x0 + x1 <= 12, x >= 0 without upper bounds: the rows imply them, nothing can be removed with them,
    and the caller keeps its own model (Presolve::run: the bound stage is dropped)."""
    rp = np.array([0, 2, 4], np.int32); ci = np.array([0, 1, 0, 1], np.int32); v = np.array([1.0, 2.0, 3.0, 1.0])
    model = hprlp.Model.from_csr(2, 2, rp, ci, v, [-INF, -INF], [10.0, 12.0], [0.0, 0.0], [INF, INF], [-3.0, -5.0])
    with pytest.raises(RuntimeError):
        hprlp.Presolved(model)
    model.free()


def test_randomised_sweep_of_the_chain():
    """90 LPs of three families (decorated, structured with freed columns, doubleton chains with freed columns) through the
    whole chain -- reductions, doubleton substitution, bound propagation, several rounds: optimum kept and original-model KKT
    of the postsolved exact solution at 1e-8."""
    def gen(seed):
        kind = seed % 3
        if kind == 0:
            return decorated_lp(seed)
        if kind == 1:
            lp = structured_lp(seed, m0=40 + seed % 50, n0=60 + seed % 70)
            pick = np.random.default_rng(seed).random(lp["n"]) < 0.3
            lp["u"] = np.where(pick & (lp["l"] < lp["u"]), np.inf, lp["u"])
            return lp
        return doubleton_lp(seed, m0=30 + seed % 40, n0=50 + seed % 60, pairs=3 + seed % 9, free_share=[0.0, 0.3, 0.6][(seed // 3) % 3])
    ran = dt = tb = 0
    for seed in range(200, 290):
        lp = gen(seed)
        try:
            f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
        except AssertionError:
            continue
        model = make_model(lp)
        try:
            pre = hprlp.Presolved(model)
        except RuntimeError:
            model.free()
            continue
        ran += 1
        dt += pre.stats["doubleton_rows"]
        tb += pre.stats["tightened_bounds"]
        rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
        fr, xr, yr, zr = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
        assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0)), (seed, pre.stats)
        x, y, z = pre.postsolve(xr, yr, zr)
        k = hprlp.original_kkt(model, x, y, z)
        assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-8, (seed, k, pre.stats)
        pre.free(); model.free()
    assert ran >= 60 and dt >= 100 and tb >= 300, (ran, dt, tb)


def test_free_singleton_column_with_a_cost():
    """min 0.5 f + x1 + 2 x2  s.t.  f + x1 + x2 >= 2 (row 0),  1 <= x1 + 3 x2 <= 4 (row 1),  0 <= x1, x2 <= 5,  f free.
    f appears in row 0 only and is free, so z_f = 0 forces y_0 = 0.5 > 0: row 0 is active at 2 in every optimum and f is
    substituted out as in an equality row; row 0 disappears with it."""
    rp = np.array([0, 3, 5], np.int32); ci = np.array([0, 1, 2, 1, 2], np.int32); v = np.array([1.0, 1.0, 1.0, 1.0, 3.0])
    AL, AU = np.array([2.0, 1.0]), np.array([INF, 4.0])
    l, u, c = np.array([-INF, 0.0, 0.0]), np.array([INF, 5.0, 5.0]), np.array([0.5, 1.0, 2.0])
    model = hprlp.Model.from_csr(2, 3, rp, ci, v, AL, AU, l, u, c)
    f0, x0, y0, z0 = highs(2, 3, rp, ci, v, AL, AU, l, u, c)
    pre = hprlp.Presolved(model)
    assert pre.stats["slack_cols"] == 1 and pre.reduced.m == 1 and pre.reduced.n == 2
    rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc = reduced_arrays(pre)
    np.testing.assert_allclose(rc, [0.5, 1.5])  # c_k - (c_f / a) a_0k
    fr, xr, yr, zr = highs(rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-12
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-12, k
    assert y[0] == 0.5 and z[0] == 0.0 and abs(x[0] + x[1] + x[2] - 2.0) <= 1e-12
    pre.free(); model.free()


def test_implied_free_singleton_column():
    """min f + 3 x1 + 0.5 x2  s.t.  f + x1 + x2 = 4 (row 0),  x1 + 2 x2 <= 2.5 (row 1),  -0.5 <= x1 - x2 <= 0.8 (row 2),
    0 <= x1, x2 <= 1,  0 <= f <= 10.  Row 0 and the boxes of x1, x2 keep f in [2, 4]: its own bounds never bind, so it
    counts as free, is substituted out and takes row 0 with it (the row would otherwise stay behind as a ranged row)."""
    rp = np.array([0, 3, 5, 7], np.int32); ci = np.array([0, 1, 2, 1, 2, 1, 2], np.int32)
    v = np.array([1.0, 1.0, 1.0, 1.0, 2.0, 1.0, -1.0])
    AL, AU = np.array([4.0, -INF, -0.5]), np.array([4.0, 2.5, 0.8])
    l, u, c = np.array([0.0, 0.0, 0.0]), np.array([10.0, 1.0, 1.0]), np.array([1.0, 3.0, 0.5])
    model = hprlp.Model.from_csr(3, 3, rp, ci, v, AL, AU, l, u, c)
    f0, x0, y0, z0 = highs(3, 3, rp, ci, v, AL, AU, l, u, c)
    pre = hprlp.Presolved(model)
    assert pre.stats["slack_cols"] == 1 and pre.reduced.m == 2 and pre.reduced.n == 2, pre.stats
    rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc = reduced_arrays(pre)
    np.testing.assert_allclose(rc, [2.0, -0.5])
    fr, xr, yr, zr = highs(rm, rn, rp2, ci2, v2, rAL, rAU, rl, ru, rc)
    assert abs(fr + pre.reduced.obj_constant - f0) <= 1e-12
    x, y, z = pre.postsolve(xr, yr, zr)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-12, k
    assert 2.0 <= x[0] <= 4.0 and z[0] == 0.0 and y[0] == 1.0
    pre.free(); model.free()


def test_model_solved_by_presolve_alone():
    """min f + 3 x1 + 0.5 x2  s.t.  f + x1 + x2 = 4,  x1 + 2 x2 <= 2.5,  0 <= x1, x2 <= 1,  0 <= f <= 10: the reductions
    remove every row and column (implied-free column, dual fixing, singleton row, empty column); solve() then returns
    the postsolved optimum without a single iteration -- and without touching a GPU, so this runs on the CPU box."""
    rp = np.array([0, 3, 5], np.int32); ci = np.array([0, 1, 2, 1, 2], np.int32); v = np.array([1.0, 1.0, 1.0, 1.0, 2.0])
    AL, AU = np.array([4.0, -INF]), np.array([4.0, 2.5])
    l, u, c = np.array([0.0, 0.0, 0.0]), np.array([10.0, 1.0, 1.0]), np.array([1.0, 3.0, 0.5])
    model = hprlp.Model.from_csr(2, 3, rp, ci, v, AL, AU, l, u, c)
    f0, x0, y0, z0 = highs(2, 3, rp, ci, v, AL, AU, l, u, c)
    r = model.solve(hprlp.Parameters(stop_tol=1e-8, use_presolve=True))
    assert r.status == "OPTIMAL" and r.iter == 0
    assert abs(r.primal_obj - f0) <= 1e-12
    np.testing.assert_allclose(r.x, x0, atol=1e-12)
    k = hprlp.original_kkt(model, r.x, r.y, r.z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-12, k
    model.free()


def test_presolve_declines(model_mps_arrays):
    """Nothing to remove (the reference's model.mps) and infeasible input: the caller keeps the original model."""
    a = model_mps_arrays
    model = hprlp.Model.from_csr(a["m"], a["n"], a["rowptr"], a["colind"], a["values"], a["AL"], a["AU"], a["l"], a["u"], a["c"])
    with pytest.raises(RuntimeError):
        hprlp.Presolved(model)
    model.free()
    rp = np.array([0, 1, 2], np.int32); ci = np.array([0, 0], np.int32); v = np.array([1.0, 1.0])
    bad = hprlp.Model.from_csr(2, 1, rp, ci, v, [2.0, -INF], [INF, 1.0], [0.0], [INF], [1.0])  # x >= 2 and x <= 1
    with pytest.raises(RuntimeError):
        hprlp.Presolved(bad)
    bad.free()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_the_reference_presolver(seed):
    """PSLP (the reference's presolver) and ours on the same LP: both reduced models have the original optimum and
    both postsolves give a KKT point of the original model.  (Sizes differ either way: PSLP has more reductions, ours
    eliminates zero-cost singleton columns of inequality rows that PSLP v0.0.8 keeps.)"""
    lp = structured_lp(seed)
    model = make_model(lp)
    f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    ref = pslp_record("structured_%d" % seed, lp)
    pre = hprlp.Presolved(model)
    assert ref["status"] == 1  # REDUCED
    assert ref["rm"] < lp["m"] and ref["rn"] < lp["n"] and pre.reduced.m < lp["m"] and pre.reduced.n < lp["n"]
    # PSLP's postsolve of the exact optimum of its reduced model
    kp = hprlp.original_kkt(model, ref["x"], ref["y"], ref["z"])
    # PSLP's obj_offset counts columns given with l == u twice (v0.0.8), so the comparison goes through c.x
    assert abs(kp["primal_obj"] - f0) <= 1e-7 * (1 + abs(f0))
    assert kp["primal_feas"] <= 1e-8
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fo, xo, yo, zo = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    x, y, z = pre.postsolve(xo, yo, zo)
    k = hprlp.original_kkt(model, x, y, z)
    assert abs(k["primal_obj"] - kp["primal_obj"]) <= 1e-7 * (1 + abs(f0))
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-9
    pre.free(); model.free()


@pytest.mark.parametrize("seed,free_share", [(31, 0.0), (34, 0.0), (42, 0.5), (43, 0.5)])
def test_doubletons_and_bounds_against_the_reference_presolver(seed, free_share):
    """The LPs of the doubleton / bound-propagation tests through PSLP as well: its DtonsEq and Primal_propagation are the
    counterparts of our two stages.  Both reduced models keep the optimum; ours is not larger than PSLP's by more than the
    rows PSLP's extra machinery (dual propagation) removes -- checked loosely: within 25 % of its row and column counts."""
    lp = doubleton_lp(seed, free_share=free_share)
    try:
        f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    except AssertionError:
        pytest.skip("unbounded after freeing columns")
    model = make_model(lp)
    ref = pslp_record("doubleton_%d_%g" % (seed, free_share), lp)
    pre = hprlp.Presolved(model)
    assert ref["status"] == 1
    if ref["rm"] > 0 and ref["rn"] > 0:
        kp = hprlp.original_kkt(model, ref["x"], ref["y"], ref["z"])
        assert abs(kp["primal_obj"] - f0) <= 1e-7 * (1 + abs(f0)) and kp["primal_feas"] <= 1e-8
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    fo, xo, yo, zo = highs(rm, rn, rp, ci, v, AL, AU, l, u, c)
    assert abs(fo + pre.reduced.obj_constant - f0) <= 1e-8 * (1 + abs(f0))
    x, y, z = pre.postsolve(xo, yo, zo)
    k = hprlp.original_kkt(model, x, y, z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-8
    print(f"seed {seed}: original {lp['m']} x {lp['n']}, PSLP {ref['rm']} x {ref['rn']}, ours {rm} x {rn}")
    assert rm <= 1.25 * ref["rm"] + 5 and rn <= 1.25 * ref["rn"] + 5
    pre.free(); model.free()


@pytest.mark.gpu
def test_solve_with_presolve_matches_solve_without(gpu):
    lp = structured_lp(11, m0=300, n0=500)
    model = make_model(lp)
    f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    on = model.solve(hprlp.Parameters(stop_tol=1e-8, use_presolve=True))
    off = model.solve(hprlp.Parameters(stop_tol=1e-8, use_presolve=False))
    assert on.status == "OPTIMAL" and off.status == "OPTIMAL"
    assert len(on.x) == lp["n"] and len(on.y) == lp["m"] and len(on.z) == lp["n"]
    assert abs(on.primal_obj - f0) <= 1e-6 * (1 + abs(f0))
    assert abs(off.primal_obj - f0) <= 1e-6 * (1 + abs(f0))
    k = hprlp.original_kkt(model, on.x, on.y, on.z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-6, k
    model.free()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 3, 8, 12, 22, 30])
def test_gpu_solve_of_decorated_lps_with_presolve(gpu, seed):
    """End to end on the GPU: solve() with the presolver on, for LPs that trigger every reduction; the returned triple (in
    the ORIGINAL dimensions) has the exact solver's optimum and passes the original-model KKT evaluation."""
    lp = decorated_lp(seed)
    try:
        f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    except AssertionError:
        pytest.skip("this decoration is infeasible or unbounded")
    model = make_model(lp)
    r = model.solve(hprlp.Parameters(stop_tol=1e-7, use_presolve=True, max_iter=400000))
    assert r.status == "OPTIMAL"
    assert abs(r.primal_obj - f0) <= 1e-5 * (1 + abs(f0))
    k = hprlp.original_kkt(model, r.x, r.y, r.z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-5, k
    assert len(r.x) == lp["n"] and len(r.y) == lp["m"]
    model.free()


@pytest.mark.parametrize("seed,free_share", [(33, 0.0), (45, 0.5)])
def test_doubleton_chain_keeps_the_reduced_model_well_conditioned(seed, free_share):
    """Regression (CPU, oracle as the solver): the reduced model must not be harder for the first-order method than the model as
    given.  A chain of substitutions with |a_k / a_j| < 1 used to leave fill-in entries of 1e-9 / 1e-10 (no cancellation
    involved); the solver's column scaling blows such columns up and the reduced models of these two seeds took 221 850 / 294 300
    iterations where the originals took 34 650 (1e-6) / 1 500 (1e-4)."""
    from oracle import oracle as O
    lp = doubleton_lp(seed, m0=200, n0=320, pairs=30, free_share=free_share)
    model = make_model(lp)
    pre = hprlp.Presolved(model)
    rm, rn, rp, ci, v, AL, AU, l, u, c = reduced_arrays(pre)
    av = np.abs(v[v != 0.0])
    assert av.min() >= 1e-6 * av.max() / 30, (av.min(), av.max())  # dynamic range of the entries stays bounded
    tol = 1e-4
    r0 = O.solve(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                 params=O.Params.default(stop_tol=tol, max_iter=400000))
    r1 = O.solve(rm, rn, rp, ci, v, AL, AU, l, u, c, params=O.Params.default(stop_tol=tol, max_iter=400000))
    assert r0["status"] == r1["status"] == "OPTIMAL"
    assert r1["iter"] <= 4 * r0["iter"] + 3000, (r1["iter"], r0["iter"])
    pre.free(); model.free()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,free_share", [(31, 0.0), (33, 0.0), (42, 0.5), (45, 0.5), (46, 0.5)])
def test_gpu_solve_with_doubletons_and_implied_bounds(gpu, seed, free_share):
    """solve() through the whole chain (reductions, doubleton substitution, bound propagation) on the GPU: an approximate
    solution of the reduced model, postsolved, has the exact optimum and passes the original-model KKT evaluation."""
    lp = doubleton_lp(seed, m0=200, n0=320, pairs=30, free_share=free_share)
    try:
        f0, *_ = highs(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    except AssertionError:
        pytest.skip("unbounded after freeing columns")
    model = make_model(lp)
    r = model.solve(hprlp.Parameters(stop_tol=1e-6, use_presolve=True, max_iter=400000))
    assert r.status == "OPTIMAL"
    # (round 3: the reduced models of seeds 33 and 45 held fill-in entries of 1e-9 / 1e-10 -- products of chained substitution
    # factors below one -- and took 220 000 / 385 000 iterations at 1e-6, on the edge of the limit; DoubletonStage now refuses a
    # substitution that would leave an entry below 1e-6 of its row's largest one: 17 100 / 16 350 iterations, oracle on both)
    assert r.iter <= 150000, r.iter
    assert abs(r.primal_obj - f0) <= 1e-4 * (1 + abs(f0))
    k = hprlp.original_kkt(model, r.x, r.y, r.z)
    assert max(k["primal_feas"], k["dual_feas"], k["gap"]) <= 1e-5, k  # (stop_tol on the reduced model, slack for the norms)
    model.free()
