"""The ray-test evaluator of tests/evalref.py (evaluate_rays) on the CPU, on the oracle's scaled data: it agrees with the independent
numpy restatement of the ratio tests (tests/test_detect.py) on the UNSCALED model, an FP64 evaluation in other summation orders
is within its bounds, and the deliberately wrong evaluations are NOT: one matrix entry left out of the arg-max line, the arg-max
element left out of each of the six maxima, a sum paired with the wrong bound side.  Every (sign, bound kind) branch is
populated by the rays used, and a NaN never passes."""
import numpy as np
import pytest
from scipy import sparse

import evalcases as C
import evalref as E
from conftest import lpgen
from oracle import oracle as O
from test_detect import dual_ray_test, primal_ray_test
from test_evalref import _ReadBack, inputs_of

CASES = ("small", "stream-rows", "tiled-aside")
_cache = {}


def scaled(case):
    """(lp, ScaledLP with use_CR_scaling=0, evaluator inputs): built once per process and left unchanged"""
    if case not in _cache:
        lp = C.case_lp(case, lpgen)
        ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                         O.Params.default(use_CR_scaling=0))
        _cache[case] = (lp, ref, inputs_of(ref))
    return _cache[case]


def col_kinds(n):
    return np.arange(n) % C.COL_KINDS


def row_kinds(m):
    return np.arange(m) % C.ROW_KINDS


def targeted(case, lp, inp, slot):
    """Rays whose maximum `slot` is dominated by one line: (ds, ys, the line, a stored entry of it in A (WQ) or A^T (VZ) or None)."""
    A, AT, data, sc = inp
    m, n = lp["m"], lp["n"]
    ds, ys = E.random_rays(m, n, 11)
    fin = np.isfinite
    if slot == "VZ":      # a column without a lower bound (kinds 2, 3: z_j > 0 is a violation), the longest of them
        lens = np.diff(AT[0])
        j = int(np.argmax(np.where(~fin(data["l"]), lens, -1)))
        return ds, E.line_of(AT, j, m, -1.0), j, E.largest_entry(AT, j)
    if slot == "WQ":      # a row with a finite upper side (q_i > 0 steps out of it), the longest of them
        lens = np.diff(A[0])
        i = int(np.argmax(np.where(fin(data["AU"]), lens, -1)))
        return E.line_of(A, i, n, 1.0), ys, i, E.largest_entry(A, i)
    if slot in ("YN", "VY"):   # y_i > 0 on a row without a lower side: it enters both
        i = int(np.flatnonzero(~fin(data["AL"]))[-1])
        return ds, E.boosted(ys, data["row_norm"], i, 1.0), i, None
    j = int(np.flatnonzero(fin(data["l"]))[-1])   # DN, WD: d_j < 0 on a column with a finite lower bound
    return E.boosted(ds, data["col_norm"], j, -1.0), ys, j, None


@pytest.mark.parametrize("case", CASES)
def test_against_the_independent_restatement_on_the_unscaled_model(case):
    """D, V, c'd, W of the evaluator (scaled data, scaled rays) against primal_ray_test / dual_ray_test on the model as the
    caller gave it and the rays mapped to its units in FP64.  Tolerance: TOL_FACTOR x the evaluator's bound (the restatement's own
    FP64 sums are an evaluation in one more order) plus the allowance for scale()'s roundings, counted beside evalref.K_ENTRY:
    22 on a matrix entry + 11 on each of its two norms + 2 on the ray entry = 46 u per product with an entry, 13 on a side, bound
    or cost + 11 on its norm + 2 = 26 u per product with one."""
    lp, ref, inp = scaled(case)
    assert (E.K_ENTRY, E.K_SIDE) == (46, 26)
    A, AT, data, sc = inp
    AT0 = sparse.csr_matrix(lp["A"].T)
    AT0.sort_indices()
    for seed in (1, 2):
        ds, ys = E.random_rays(lp["m"], lp["n"], seed)
        want = E.evaluate_rays(A, AT, data, sc, ds, ys)
        d = (ds / data["col_norm"]) * sc["b_scale"]
        y = (ys / data["row_norm"]) * sc["c_scale"]
        allow = E.caller_units_allowance((lp["rowptr"], lp["colind"], lp["values"]), (AT0.indptr, AT0.indices, AT0.data), lp, d, y)
        D, V = primal_ray_test(lp, y)
        cd, W = dual_ray_test(lp, d)
        for name, got in (("D", D), ("V", V), ("cd", cd), ("W", W)):
            v, b = want[name]
            diff, tol = abs(E.LD(got) - v), E.TOL_FACTOR * b + allow[name]
            print(case, seed, name, "value %.6g difference %.3g tolerance %.3g (bound %.3g, allowance %.3g)" % (float(v), float(diff), float(tol), float(b), float(allow[name])))
            assert np.isfinite(got) and diff <= tol and tol <= 1e-9 * max(abs(float(v)), 1.0), (name, got, v, tol)
            assert abs(float(v)) > 0


def _sequential(p):
    return np.cumsum(p)[-1] if len(p) else 0.0      # (np.cumsum adds one term after the other in FP64)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("order", ["csr", "reversed"])
def test_fp64_in_other_summation_orders_is_within_bounds(case, order):
    lp, ref, inp = scaled(case)
    ds, ys = E.random_rays(lp["m"], lp["n"], 3)
    want = E.evaluate_rays(*inp, ds, ys)
    total = _sequential if order == "csr" else (lambda p: _sequential(p[::-1]))

    def row_sums(csr, v, drop):
        rp, ci, val = csr
        p = np.asarray(val, np.float64) * np.asarray(v, np.float64)[ci]
        return np.array([total(p[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])

    got = E.evaluate_rays_f64(*inp, ds, ys, row_sums=row_sums, total=total)
    r = E.ratios(got, want, E.RAY_NAMES)
    print(case, order, {k: round(v, 4) for k, v in r.items()})
    assert E.all_within(r), r
    assert all(abs(got[k]) > 0 for k in E.RAY_NAMES), got
    # numpy's own (pairwise) order too
    assert E.all_within(E.ratios(E.evaluate_rays_f64(*inp, ds, ys), want, E.RAY_NAMES))


@pytest.mark.parametrize("case", CASES)
def test_a_sum_with_the_wrong_bound_side_is_out_of_bounds(case):
    lp, ref, inp = scaled(case)
    ds, ys = E.random_rays(lp["m"], lp["n"], 3)
    want = E.evaluate_rays(*inp, ds, ys)
    bad = E.ratios(E.evaluate_rays_f64(*inp, ds, ys, swap_sides=True), want, E.RAY_NAMES)
    print(case, {k: "%.3g" % v for k, v in bad.items()})
    assert min(bad["DY"], bad["DZ"], bad["D"]) > E.TOL_FACTOR, bad
    assert max(bad["CD"], bad["WD"], bad["WQ"], bad["YN"], bad["DN"]) <= E.TOL_FACTOR, bad    # (the primal ray's side has no such pairing)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("slot", E.RAY_MAXIMA)
def test_a_left_out_arg_max_and_a_left_out_entry_are_out_of_bounds(case, slot):
    lp, ref, inp = scaled(case)
    ds, ys, line, entry = targeted(case, lp, inp, slot)
    want = E.evaluate_rays(*inp, ds, ys)
    k, top, second = E.top_two(want["elements"][slot])
    print(case, slot, "line", line, "maximum %.6g runner-up %.6g" % (top, second))
    assert k == line and top > 0 and second <= 0.5 * top, (k, line, top, second)      # asserted on the reference
    assert E.ratio(E.evaluate_rays_f64(*inp, ds, ys)[slot], want[slot]) <= E.TOL_FACTOR
    bad = E.evaluate_rays_f64(*inp, ds, ys, leave_out={slot: line})
    assert E.ratio(bad[slot], want[slot]) > E.TOL_FACTOR, (bad[slot], want[slot])
    if slot in ("VZ", "WQ"):
        drop = dict(drop_AT=entry) if slot == "VZ" else dict(drop_A=entry)
        bad = E.evaluate_rays_f64(*inp, ds, ys, **drop)
        assert E.ratio(bad[slot], want[slot]) > E.TOL_FACTOR, (bad[slot], want[slot])
        # ... and the evaluator itself with the entry left out is as far from the complete FP64 evaluation
        assert E.ratio(E.evaluate_rays_f64(*inp, ds, ys)[slot], E.evaluate_rays(*inp, ds, ys, **drop)[slot]) > E.TOL_FACTOR


@pytest.mark.parametrize("case", CASES)
def test_every_branch_is_populated(case):
    """Over the random rays used above every (sign, bound kind) pair occurs at least n / 32 resp. m / 20 times: each of the 8
    column kinds with z > 0, z < 0, d > 0, d < 0 and each of the 5 row kinds with y > 0, y < 0, q > 0, q < 0; about one entry in
    eight of ds and ys is exactly 0."""
    lp, ref, inp = scaled(case)
    A, AT, data, sc = inp
    m, n = lp["m"], lp["n"]
    jk, ik = col_kinds(n), row_kinds(m)
    l, u, AL, AU = data["l"], data["u"], data["AL"], data["AU"]
    fin = np.isfinite
    # (the cycled kinds are what evalcases.all_bounds_lp says: the finite sides survive the scaling)
    assert (fin(l) == np.isin(jk, (0, 1, 4, 5, 6, 7))).all() and (fin(u) == np.isin(jk, (3, 5, 6, 7))).all()
    assert (fin(AL) == np.isin(ik, (0, 2, 3))).all() and (fin(AU) == np.isin(ik, (0, 1, 3))).all()
    for seed in (1, 2, 3):
        ds, ys = E.random_rays(m, n, seed)
        for v in (ds, ys):      # (a binomial count with p = 1 / 8: within four standard deviations)
            assert abs((v == 0).sum() - len(v) / 8) <= 4 * np.sqrt(len(v) * 7 / 64), (case, seed, int((v == 0).sum()), len(v))
        s = E._row_sums(AT, ys, None, np.float64)[0]
        q = E._row_sums(A, ds, None, np.float64)[0]
        z = -s
        for kind in range(C.COL_KINDS):
            for v in (z, ds):
                assert ((v > 0) & (jk == kind)).sum() >= n / 32 and ((v < 0) & (jk == kind)).sum() >= n / 32, (case, seed, kind)
        for kind in range(C.ROW_KINDS):
            for v in (ys, q):
                assert ((v > 0) & (ik == kind)).sum() >= m / 20 and ((v < 0) & (ik == kind)).sum() >= m / 20, (case, seed, kind)


def test_a_nan_in_any_slot_fails():
    lp, ref, inp = scaled("small")
    ds, ys = E.random_rays(lp["m"], lp["n"], 3)
    s = _ReadBack(inp, dict(ray_d=ds, ray_y=ys))
    patterns = (ref.Arp, ref.Aci, ref.ATrp, ref.ATci)
    got = E.evaluate_rays_f64(*inp, ds, ys)
    _, _, want, r = E.check_rays(s, patterns, got)
    assert set(r) == set(E.RAY_NAMES) and len(r) == 15
    for name in E.RAY_NAMES:
        for value in (np.nan, np.inf):
            assert E.ratio(value, want[name]) == np.inf
            with pytest.raises(AssertionError):
                E.check_rays(s, patterns, dict(got, **{name: value}))
    # a NaN in the rays themselves (the reference is not finite) fails too
    bad = ys.copy()
    bad[5] = np.nan
    with pytest.raises(AssertionError):
        E.check_rays(_ReadBack(inp, dict(ray_d=ds, ray_y=bad)), patterns, got)


@pytest.mark.parametrize("kind", [1, 2])
def test_certificate_values_from_both_sides(kind):
    """check_certificate_values (the GPU certificate tests' two-sided check) on a planted certificate in the caller's units: the
    restatement's numbers pass; an objective off by 1e-9 of itself, or a violation off by 1e-9 of the objective to EITHER side,
    does not."""
    if kind == 1:
        lp = lpgen.planted_infeasible_lp(300, 400, 2400, 1)
        ray = lp["y_cert"] / np.abs(lp["y_cert"]).max()
    else:
        lp = lpgen.planted_unbounded_lp(300, 400, 2400, 5)
        ray = lp["d_cert"] / np.abs(lp["d_cert"]).max()
    rng = np.random.default_rng(kind)
    ray = ray + 1e-9 * rng.normal(size=len(ray))      # (as a verdict's ray: the violation is small, not zero)
    ray /= np.abs(ray).max()
    obj, viol = primal_ray_test(lp, ray) if kind == 1 else dual_ray_test(lp, ray)
    assert viol > 0
    E.check_certificate_values(lp, kind, ray, obj, viol)
    for bad in ((obj * (1 + 1e-9), viol), (obj, viol + 1e-9 * abs(obj)), (obj, viol - 1e-9 * abs(obj)), (np.nan, viol), (obj, np.nan)):
        with pytest.raises(AssertionError):
            E.check_certificate_values(lp, kind, ray, *bad)
