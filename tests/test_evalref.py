"""The high-precision evaluator of tests/evalref.py on the CPU: it agrees with the project's FP64 numpy formulas within its own
bound on every LP of tests/test_gpu_evaluation.py, an FP64 evaluation that leaves one matrix entry out does NOT, and its pieces
(empty rows, any summation order, the iteration-0 bound term) behave as its docstring derives, and a NaN never passes."""
import numpy as np
import pytest

import evalcases as C
import evalref as E
from conftest import lpgen
from oracle import oracle as O


def oracle_state(lp, normal=17, sigma=0.6):
    """The oracle stepped `normal` iterations and one check step from zero: (ScaledLP, state, sigma, lambda)."""
    ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                     O.Params.default(use_CR_scaling=0))
    lam = 1.01 * ref.power_iteration()[0]
    st = ref.new_state()
    for k in range(normal + 1):
        ref.x_half(st, sigma, k, int(k == normal))
        ref.y_half(st, sigma, lam, k, int(k == normal))
    return ref, st, sigma, lam


def inputs_of(ref):
    sc = ref.sc
    return ((ref.Arp, ref.Aci, ref.Av), (ref.ATrp, ref.ATci, ref.ATv),
            dict(c=ref.c, AL=ref.AL, AU=ref.AU, l=ref.l, u=ref.u, row_norm=ref.row_norm, col_norm=ref.col_norm),
            dict(b_scale=sc.b_scale, c_scale=sc.c_scale, norm_b_org=sc.norm_b_org, norm_c_org=sc.norm_c_org))


def test_longdouble_has_a_64_bit_mantissa():
    """(otherwise evalref forms its row sums with math.fsum; the machines this suite runs on are x86-64)"""
    assert np.finfo(np.longdouble).nmant >= 63


def test_every_bound_kind_is_in_every_lp():
    lp = C.case_lp("small", lpgen)
    l, u, AL, AU = lp["l"], lp["u"], lp["AL"], lp["AU"]
    fin = np.isfinite
    kinds = [(l == 0) & ~np.signbit(l) & ~fin(u), (l == 0) & np.signbit(l) & ~fin(u), ~fin(l) & ~fin(u), ~fin(l) & fin(u),
             fin(l) & (l != 0) & ~fin(u), fin(l) & (l != 0) & fin(u) & (l < u), fin(l) & (l == u), (l == 0) & ~np.signbit(l) & fin(u)]
    assert all(k.sum() >= lp["n"] // 8 for k in kinds) and sum(k.sum() for k in kinds) == lp["n"]
    rows = [fin(AL) & (AL == AU), ~fin(AL) & fin(AU), fin(AL) & ~fin(AU), fin(AL) & fin(AU) & (AL < AU), ~fin(AL) & ~fin(AU)]
    assert all(k.sum() >= lp["m"] // 5 for k in rows) and sum(k.sum() for k in rows) == lp["m"]
    x, Ax = lp["x_star"], lp["A"] @ lp["x_star"]
    assert (x >= l).all() and (x <= u).all() and (Ax >= AL - 1e-9).all() and (Ax <= AU + 1e-9).all()   # the planted point is feasible


def test_row_sums_with_empty_rows():
    rp = np.array([0, 0, 2, 2, 2, 3, 3])
    ci = np.array([0, 1, 1])
    val = np.array([2.0, 3.0, 5.0])
    s, a, lens = E._row_sums((rp, ci, val), np.array([1.0, -1.0]))
    assert list(s) == [0, -1, 0, 0, -5, 0] and list(a) == [0, 5, 0, 0, 5, 0] and list(lens) == [0, 2, 0, 0, 1, 0]
    s, _, _ = E._row_sums((rp, ci, val), np.array([1.0, -1.0]), drop=1)
    assert list(s) == [0, 2, 0, 0, -5, 0]


@pytest.mark.parametrize("case", list(C.CASES))
def test_evaluator_agrees_with_the_fp64_formulas_and_sees_a_dropped_entry(case):
    lp = C.case_lp(case, lpgen)
    ref, st, sigma, lam = oracle_state(lp)
    A, AT, data, sc = inputs_of(ref)
    want = E.evaluate(A, AT, data, sc, st, sigma, lam)
    got = E.evaluate_f64(A, AT, data, sc, st, sigma, lam)
    r = E.ratios(got, want)
    print(case, {k: round(v, 4) for k, v in r.items()})
    assert all(np.isfinite(float(want[k][0])) and want[k][0] > 0 for k in ("err_Rp", "err_Rd", "weighted_norm")), want
    assert E.all_within(r), r
    # one entry left out of the FP64 evaluation: the pass that owns it, and the weighted norm, are out of bounds
    drop_A, drop_AT = E.sensitivity_drops(A, AT, data, st)
    bad = E.ratios(E.evaluate_f64(A, AT, data, sc, st, sigma, lam, drop_A=drop_A), want)
    assert bad["err_Rp"] > E.TOL_FACTOR and bad["weighted_norm"] > E.TOL_FACTOR and bad["err_Rd"] <= E.TOL_FACTOR, bad
    bad = E.ratios(E.evaluate_f64(A, AT, data, sc, st, sigma, lam, drop_AT=drop_AT), want)
    assert bad["err_Rd"] > E.TOL_FACTOR and bad["err_Rp"] <= E.TOL_FACTOR, bad
    assert not E.within(E.evaluate_f64(A, AT, data, sc, st, sigma, lam, drop_A=drop_A, drop_AT=drop_AT), want)


def _sequential(p):
    return np.cumsum(p)[-1] if len(p) else 0.0      # (np.cumsum adds one term after the other in FP64)


def _chunked_tree(p, chunk):
    """Sequential FP64 partial sums of `chunk` terms each, combined pairwise: what tiles, pieces and wavefront reductions do."""
    parts = np.array([_sequential(p[k:k + chunk]) for k in range(0, len(p), chunk)])
    while len(parts) > 1:
        if len(parts) % 2:
            parts = np.append(parts, 0.0)
        parts = parts[0::2] + parts[1::2]
    return parts[0] if len(parts) else 0.0


def _orders():
    rng = np.random.default_rng(3)
    return {"backwards": lambda p: _sequential(p[::-1]),
            "a tree of partial sums of 64": lambda p: _chunked_tree(p, 64),
            "a tree of partial sums of 7": lambda p: _chunked_tree(p, 7),
            "a permutation": lambda p: _sequential(p[rng.permutation(len(p))])}


@pytest.mark.parametrize("order", list(_orders()))
def test_bound_holds_for_other_summation_orders(order):
    """Every row sum and every reduction of the FP64 evaluation taken in another order (backwards, sequential partial sums combined
    as a tree, a random permutation) on the LP with rows of 64 to 5000 entries: all inside the bound."""
    lp = C.case_lp("stream-rows", lpgen)
    ref, st, sigma, lam = oracle_state(lp)
    A, AT, data, sc = inputs_of(ref)
    want = E.evaluate(A, AT, data, sc, st, sigma, lam)
    total = _orders()[order]

    def row_sums(csr, v, drop):
        rp, ci, val = csr
        p = np.asarray(val, np.float64) * np.asarray(v, np.float64)[ci]
        return np.array([total(p[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])

    got = E.evaluate_f64(A, AT, data, sc, st, sigma, lam, row_sums=row_sums, dot=lambda a, b: total(a * b))
    r = E.ratios(got, want)
    print(order, {k: round(v, 4) for k, v in r.items()})
    assert E.all_within(r), r


class _ReadBack:
    """What evalref.check_solver reads from a solver, served from the oracle's arrays."""
    def __init__(self, inputs, st):
        A, AT, data, self._scalars = inputs
        self._v = dict(data, A_val=A[2], AT_val=AT[2], **st)

    def get(self, name):
        return self._v[name]

    def scalars(self):
        return self._scalars


@pytest.mark.parametrize("broken", E.QUANTITIES)
def test_a_nan_in_any_one_quantity_fails_the_solver_check(broken):
    """check_solver on correct FP64 values passes; with a NaN (or an infinity) in any single quantity it fails, whichever key
    the NaN sits under (a max() over the ratios would skip a NaN that does not come first)."""
    lp = C.case_lp("small", lpgen)
    ref, st, sigma, lam = oracle_state(lp)
    inputs = inputs_of(ref)
    s = _ReadBack(inputs, st)
    patterns = (ref.Arp, ref.Aci, ref.ATrp, ref.ATci)
    got = E.evaluate_f64(*inputs, st, sigma, lam)
    E.check_solver(s, patterns, got, sigma, lam)
    want = E.evaluate(*inputs, st, sigma, lam)
    for value in (np.nan, np.inf):
        bad = dict(got, **{broken: value})
        assert E.ratio(value, want[broken]) == np.inf and not E.within(bad, want) and not E.all_within(E.ratios(bad, want))
        with pytest.raises(AssertionError):
            E.check_solver(s, patterns, bad, sigma, lam)
    # ... also where only that quantity is asked for
    with pytest.raises(AssertionError):
        E.check_solver(s, patterns, dict(got, **{broken: np.nan}), sigma, lam, names=(broken,))


def test_iteration_zero_bound_term():
    lp = C.case_lp("small", lpgen)
    ref, st, sigma, lam = oracle_state(lp, normal=3)
    A, AT, data, sc = inputs_of(ref)
    rng = np.random.default_rng(5)
    x = st["x_bar"].copy()
    fin = np.flatnonzero(np.isfinite(ref.l) & np.isfinite(ref.u))
    pick = rng.integers(0, 3, size=len(fin))
    below, above = fin[pick == 0], fin[pick == 1]
    x[below] = ref.l[below] - rng.uniform(0.5, 1.5, size=len(below))
    x[above] = ref.u[above] + rng.uniform(0.5, 1.5, size=len(above))
    st0 = dict(st, x_bar=x)
    want = E.evaluate(A, AT, data, sc, st0, sigma, lam)
    t = np.where(x < ref.l, ref.l - x, np.where(x > ref.u, x - ref.u, 0.0))
    term = sc["b_scale"] * np.sqrt(np.sum((t / ref.col_norm) ** 2))
    assert term > 0 and E.ratio(term, want["lu_term"]) <= E.TOL_FACTOR
    assert np.array_equal(want["lu_vector"], t / ref.col_norm)
    assert want["err_Rp0"][0] == max(want["err_Rp"][0], want["lu_term"][0])
    # inside the box the term vanishes and err_Rp0 is err_Rp
    inside = E.evaluate(A, AT, data, sc, st, sigma, lam)
    assert inside["lu_term"][0] == 0 and inside["err_Rp0"][0] == inside["err_Rp"][0]
    # a bound violation the FP64 side forgets (one column) is seen
    t2 = t.copy()
    t2[below[0]] = 0.0
    assert E.ratio(sc["b_scale"] * np.sqrt(np.sum((t2 / ref.col_norm) ** 2)), want["lu_term"]) > E.TOL_FACTOR


def test_movement_norms():
    lp = C.case_lp("small", lpgen)
    ref, st, sigma, lam = oracle_state(lp)
    A, AT, data, sc = inputs_of(ref)
    want = E.evaluate(A, AT, data, sc, st, sigma, lam)
    assert E.ratio(np.linalg.norm(st["x_bar"] - st["last_x"]), want["move_x"]) <= E.TOL_FACTOR
    assert E.ratio(np.linalg.norm(st["y_bar"] - st["last_y"]), want["move_y"]) <= E.TOL_FACTOR
    assert E.ratio(np.linalg.norm(st["x_bar"] - st["last_x"]) * (1 + 1e-12), want["move_x"]) > E.TOL_FACTOR
