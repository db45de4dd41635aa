"""The warm start's reference of tests/startref.py on the CPU, on the scaled LPs of tests/test_gpu_start_values.py (the oracle's
scaling, Curtis-Reid off): its FP64 restatement stays within 1 x its own bound in three summation orders, every deliberately wrong
start of startref.MUTANTS (and one with a matrix entry left out) lies FARTHER than the 2 x tolerance in a named quantity, and the
starts reach every branch of the map, the projection, the dual completion and y_obj."""
import numpy as np
import pytest

import evalcases as C
import evalref as E
import startref as S
from conftest import lpgen
from oracle import oracle as O
from test_evalref import inputs_of

pytestmark = pytest.mark.skipif(not E.HAVE_LD, reason="np.longdouble is no wider than float64 here")

_cache = {}


def scaled_case(case):
    """(lp, inputs of the scaled LP, x0, y0, the reference) of a case, built once per process and left unchanged"""
    if case not in _cache:
        lp = C.case_lp(case, lpgen)
        ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                         O.Params.default(use_CR_scaling=0))
        inp = inputs_of(ref)
        x0, y0 = S.case_start(lp, S.case_seed(list(C.CASES).index(case)))
        _cache[case] = (lp, inp, x0, y0, S.reference(*inp, x0, y0))
    return _cache[case]


def _tree(p):
    p = np.asarray(p, np.float64)
    while len(p) > 1:
        if len(p) % 2:
            p = np.append(p, 0.0)
        p = p[0::2] + p[1::2]
    return p[0] if len(p) else 0.0


def _sequential(p):
    return np.cumsum(p)[-1] if len(p) else 0.0      # (np.cumsum adds one term after the other in FP64)


ORDERS = {"sequential": _sequential, "reversed": lambda p: _sequential(p[::-1]), "pairwise": _tree}


def _row_sums_in(total):
    def row_sums(csr, v, drop):
        rp, ci, val = csr
        p = np.asarray(val, np.float64) * np.asarray(v, np.float64)[np.asarray(ci, dtype=np.int64)]
        if drop is not None:
            p[drop] = 0.0
        return np.array([total(p[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])
    return row_sums


@pytest.mark.parametrize("case", list(C.CASES))
def test_restatement_stays_within_one_bound_in_every_order(case):
    lp, inp, x0, y0, want = scaled_case(case)
    for name, total in ORDERS.items():
        got = S.restatement(*inp, x0, y0, row_sums=_row_sums_in(total), total=total)
        r = S.ratios(got, want)
        print(case, name, {k: round(v, 4) for k, v in r.items()})
        assert all(v <= 1.0 for v in r.values()), (case, name, r)
    got = S.restatement(*inp, x0, y0)       # numpy's own orders
    r = S.ratios(got, want)
    assert all(v <= 1.0 for v in r.values()), (case, "numpy", r)
    assert all(np.isfinite(float(want[k][0])) for k in S.SCALARS) and abs(want["S_XZ"][0]) > 0 and abs(want["S_YOBJ_Y"][0]) > 0


# mutant -> the quantities of which AT LEAST ONE must be out of tolerance (all of them are asserted: each is named for a reason)
NAMED = {
    "wrong-side": ("z_bar", "S_XZ", "dual_obj"),
    "ignores-finiteness": ("z_bar",),
    "AL-AU-swapped": ("y_obj", "S_YOBJ_Y", "dual_obj"),
    "no-clamp": ("y_obj",),
    "x-dot-z": ("S_XZ", "dual_obj", "gap"),
    "free-rows-unprojected": ("y",),
    "clamp-before-scaling": ("x",),
}


@pytest.mark.parametrize("case", list(C.CASES))
def test_every_mutant_is_outside_the_tolerance(case):
    lp, inp, x0, y0, want = scaled_case(case)
    assert set(NAMED) == set(S.MUTANTS)
    for mutant, names in NAMED.items():
        bad = S.ratios(S.restatement(*inp, x0, y0, mutant=mutant), want)
        print(case, mutant, {k: bad[k] for k in names})
        assert all(bad[k] > S.TOL_FACTOR for k in names), (case, mutant, {k: bad[k] for k in names})
    # one stored entry left out of a row of A (a row whose y_obj is its activity) resp. of A^T (a column whose z_bar is w)
    xs, ys = S.start_map(inp[2], inp[3], x0, y0)
    drop_A, drop_AT = S.sensitivity_drops(inp[0], inp[1], inp[2], xs, ys)
    bad = S.ratios(S.evaluate_start_f64(*inp, xs, ys, drop_A=drop_A), want)
    assert bad["y_obj"] > S.TOL_FACTOR and bad["z_bar"] <= 1.0, (case, "A", bad)
    bad = S.ratios(S.evaluate_start_f64(*inp, xs, ys, drop_AT=drop_AT), want)
    assert bad["z_bar"] > S.TOL_FACTOR and bad["S_XZ"] > S.TOL_FACTOR and bad["y_obj"] <= 1.0, (case, "A^T", bad)


@pytest.mark.parametrize("case", list(C.CASES))
def test_the_starts_reach_every_branch(case):
    lp, (A, AT, data, sc), x0, y0, want = scaled_case(case)
    n, m = lp["n"], lp["m"]
    fin = np.isfinite
    l, u, AL, AU = data["l"], data["u"], data["AL"], data["AU"]
    jk, ik = np.arange(n) % C.COL_KINDS, np.arange(m) % C.ROW_KINDS
    # the scaled bounds keep the caller's kinds (positive scaling)
    assert np.array_equal(fin(l), fin(lp["l"])) and np.array_equal(fin(u), fin(lp["u"]))
    assert np.array_equal(fin(AL), fin(lp["AL"])) and np.array_equal(fin(AU), fin(lp["AU"]))
    # every column kind with w > 0 and with w < 0, clear of its bound (so the device takes the same branch)
    w, e_w = (np.asarray(a, np.float64) for a in want["w"])
    for kind in range(C.COL_KINDS):
        k = jk == kind
        assert ((w > 4 * e_w) & k).any() and ((w < -4 * e_w) & k).any(), (case, "column kind", kind)
    z = np.asarray(want["z_bar"][0], np.float64)
    assert ((z == 0) & (w != 0)).any() and (z > 0).any() and (z < 0).any()
    # every row kind with a projected y of each sign its cone allows, and with y = 0
    ys = np.asarray(want["y"][0], np.float64)
    allowed = {0: (1, 1), 1: (0, 1), 2: (1, 0), 3: (1, 1), 4: (0, 0)}       # kind -> (y > 0 allowed, y < 0 allowed)
    for kind, (pos, neg) in allowed.items():
        k = ik == kind
        assert ((ys == 0) & k).any(), (case, "row kind", kind, "y = 0")
        assert ((ys > 0) & k).any() == bool(pos) and ((ys < 0) & k).any() == bool(neg), (case, "row kind", kind)
    # y_obj's clamp acts from both sides and not at all where y = 0
    q = E._row_sums(A, want["x"][0], None, np.float64)[0]
    at0 = ys == 0
    assert (at0 & (q < AL)).any() and (at0 & (q > AU)).any() and (at0 & (q > AL) & (q < AU)).any(), case
    # x0 below l, inside, above u and exactly on a finite bound -- zero and not zero -- in SCALED units, before the clamp
    raw = (x0 * data["col_norm"]) / sc["b_scale"]
    assert (raw < l).any() and (raw > u).any() and ((raw > l) & (raw < u)).any(), case
    on = ((raw == l) & fin(l)) | ((raw == u) & fin(u))
    assert (on & (raw == 0)).any() and (on & (raw != 0)).any(), (case, int(on.sum()))
    assert (np.signbit(raw) & (raw == 0)).any()        # a -0.0 start against l = +-0.0
    # y0 = -0.0
    assert ((y0 == 0) & np.signbit(y0)).sum() >= m // 10
    # a start the projection changes, in x and in y
    rawy = (y0 * data["row_norm"]) / sc["c_scale"]
    assert (np.asarray(want["x"][0], np.float64) != raw).any() and (ys != rawy).any(), case
    assert ((ys == 0) & (rawy != 0)).any()


def test_null_starts_project_zero():
    lp, inp, x0, y0, want = scaled_case("small")
    xs, ys = S.start_map(inp[2], inp[3], None, None)
    l, u = inp[2]["l"], inp[2]["u"]
    assert np.array_equal(xs, np.minimum(np.maximum(0.0, l), u)) and (xs[l > 0] == l[l > 0]).all() and (l > 0).any() and (u < 0).any()
    assert (xs[u < 0] == u[u < 0]).all() and not ys.any()
    x_only, _ = S.start_map(inp[2], inp[3], x0, None)
    assert np.array_equal(x_only, np.asarray(want["x"][0], np.float64))


def test_a_nan_or_a_wrong_side_never_passes():
    lp, inp, x0, y0, want = scaled_case("small")
    got = S.restatement(*inp, x0, y0)
    for name in S.VECTORS:
        bad = np.array(got[name], dtype=np.float64)
        bad[3] = np.nan
        assert S.ratio(bad, want[name]) == np.inf
    for name in S.SCALARS:
        assert S.ratio(np.nan, want[name]) == np.inf and S.ratio(np.inf, want[name]) == np.inf
    # check_vectors: the row side's bits where y != 0
    S.check_vectors(got, want)
    ys = np.asarray(want["y"][0], np.float64)
    i = int(np.flatnonzero(ys != 0)[0])
    yo = got["y_obj"].copy()
    yo[i] = np.nextafter(yo[i], np.inf)
    with pytest.raises(AssertionError):
        S.check_vectors(dict(got, y_obj=yo), want)
