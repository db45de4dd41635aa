"""The WARM START of the single solver BY VALUE on every kernel form (GPU): k_start_in, then StartColEpi and StartRowEpi through
launch_fused (kernels.hip) behind hprlp_solver_set_start -- the seeded vectors against the float64 map and projection of
tests/startref.py bit for bit, z_bar / y_obj and the iteration-0 objectives and gap against its high-precision reference ON THE
SOLVER'S OWN READ-BACK DATA within 2 x the derived bound of that module and nothing wider, err_Rp / err_Rd through
tests/evalref.py's evaluator on the read-back state.  (kkt is the larger of those two and the START's gap: the evaluator's own gap
is x_bar . z_bar, which the start replaces by the bound terms.)

Forms and LPs: the eight entries of evalcases.CASES -- every column and row bound kind, -0.0, l = u, ranged and free rows -- at the
smallest shapes at which each form is selected.  The starts are startref.case_start (tests/test_startref.py shows on the CPU that
they reach every branch, and that the deliberately wrong starts lie outside the tolerance).  The reordered form adds only the gather
of the caller's x0 / y0 through the ordering's permutation: tests/test_gpu_reorder_small.py holds a warm start of a solver with a
locality ordering to one on the explicitly permuted LP, bit for bit.

Per case: the start with x0 and y0, with either missing and with neither (a null x0 still projects 0 into [l, u]); the same start
after seven iterations and a check step gives every vector and number the bits of the first time (invalidate_far on the tiled
forms); then 1, 2 more normal iterations and a check step from the start against a second solver under the stream hooks with the
same history, at the case's tolerance (the kXRebuild path from x_hat = x; the small kernel reading x, last_x, y, last_y).

Largest observed-difference / bound ratio per quantity and case, MI355X (the tolerance is 2; the module prints the rows,
"LARGEST RATIOS"):

| case | z_bar | y_obj | primal_obj | dual_obj | gap | err_Rp | err_Rd | kkt |
|---|---|---|---|---|---|---|---|---|
| small | 0.407 | 0.303 | 0.000258 | 0.000356 | 3.08e-05 | 0.00326 | 0.00225 | 6.55e-05 |
| stream-short | 0.413 | 0.407 | 2.83e-05 | 5.48e-05 | 8.18e-06 | 0.000694 | 0.000227 | 8.18e-06 |
| stream-rows | 0.429 | 0.451 | 2.1e-05 | 9.36e-05 | 7.2e-06 | 6.25e-05 | 0.000419 | 7.2e-06 |
| tiled | 0.408 | 0.277 | 5.23e-06 | 1.48e-05 | 3.14e-06 | 0.000187 | 0.000201 | 3.14e-06 |
| tiled-rounds | 0.379 | 0.209 | 5.37e-07 | 4.54e-06 | 8.46e-07 | 4.18e-05 | 5.23e-05 | 8.46e-07 |
| pieces | 0.431 | 0.334 | 1.32e-05 | 4.07e-05 | 3.57e-06 | 0.000474 | 0.000536 | 3.57e-06 |
| all-remainder | 0.415 | 0.474 | 5.63e-05 | 1.3e-05 | 8.62e-06 | 0.000539 | 0.00019 | 8.62e-06 |
| tiled-aside | 0.42 | 0.238 | 1.15e-05 | 2.49e-05 | 3.78e-06 | 9.16e-06 | 0.000177 | 3.78e-06 |
| worst | 0.431 | 0.474 | 0.000258 | 0.000356 | 3.08e-05 | 0.00326 | 0.00225 | 6.55e-05 |
"""
import numpy as np
import pytest

import evalcases as C
import evalref as E
import startref as S
from conftest import hprlp, lpgen
from test_gpu_epilogue_batches import set_env
from test_gpu_evaluation import EXPECT, NAMES, assert_form, make, set_form

pytestmark = pytest.mark.gpu

SEEDED_N = ("x", "x_hat", "x_bar", "last_x")
SEEDED_M = ("y", "y_bar", "last_y")
READ = SEEDED_N + SEEDED_M + ("z_bar", "y_obj")
NUMBERS = ("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt")
SIGMA = 0.6


def read_start(s):
    return {k: s.get(k) for k in READ}


def check_start(s, patterns, x0, y0, lam, label):
    """The state set_start(x0, y0) left and residuals(0, True) of it against the reference.  Returns (vectors, numbers, ratios)."""
    inp = E.solver_inputs(s, *patterns)
    got = read_start(s)
    xs, ys = S.start_map(inp[2], inp[3], x0, y0)
    for k in SEEDED_N:
        assert np.array_equal(got[k], xs), (label, k, int((got[k] != xs).sum()))
    for k in SEEDED_M:
        assert np.array_equal(got[k], ys), (label, k, int((got[k] != ys).sum()))
    want = S.evaluate_start(*inp, xs, ys)
    r = S.check_vectors(got, want, label)
    res = s.residuals(0, True)
    assert all(np.isfinite(res[k]) for k in NUMBERS), (label, res)
    r.update(S.ratios(res, want, S.RESULTS))
    _, st, ev, r2 = E.check_solver(s, patterns, res, SIGMA, lam, ("err_Rp", "err_Rd"), label)
    r.update(r2)
    # the projected start lies in the box: the iteration-0 bound term is exactly 0
    assert ev["lu_term"][0] == 0 and not st["x_temp"].any() and not ev["lu_vector"].any(), label
    kkt = (max(ev["err_Rd"][0], ev["err_Rp"][0], want["gap"][0]), max(ev["err_Rd"][1], ev["err_Rp"][1], want["gap"][1]))
    r["kkt"] = E.ratio(res["kkt"], kkt)
    print("start", label, " ".join("%s %.3g" % kv for kv in r.items()))
    assert S.all_within(r), (label, r, res)
    # the comparison can see the dual completion leaning on the wrong side
    bad = S.evaluate_start(*inp, xs, ys, mutant="wrong-side")
    assert S.ratio(got["z_bar"], bad["z_bar"]) > S.TOL_FACTOR and E.ratio(res["dual_obj"], bad["dual_obj"]) > S.TOL_FACTOR, label
    return got, {k: res[k] for k in NUMBERS}, r


@pytest.mark.parametrize("case", list(C.CASES))
def test_start_by_value_on_every_kernel_form(gpu, case, monkeypatch):
    form, tol = set_form(monkeypatch, case)
    lp = C.case_lp(case, lpgen)
    model, s, ref = make(lp)
    assert_form(s, case, form)
    patterns = (lp["rowptr"], lp["colind"], ref.ATrp, ref.ATci)
    x0, y0 = S.case_start(lp, S.case_seed(list(C.CASES).index(case)))
    worst = {}

    def note(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)

    s.scale()
    lam = 1.01 * s.power_iteration()[0]
    s.init(SIGMA, lam)
    # 1. the start with both vectors
    s.set_start(x0, y0)
    sc = s.scalars()
    assert sc["kx"] == 0 and sc["ky"] == 0
    first, numbers, r = check_start(s, patterns, x0, y0, lam, case)
    note(r)
    assert (first["z_bar"] != 0).any() and (first["y_obj"] != 0).any() and numbers["primal_obj"] != 0 and numbers["dual_obj"] != 0
    # 2. null starts: a null x0 projects 0 into [l, u]
    l, u = s.get("l"), s.get("u")
    for label, a, b in (("no x0", None, y0), ("no y0", x0, None), ("neither", None, None)):
        s.set_start(a, b)
        got, _, r = check_start(s, patterns, a, b, lam, case + " " + label)
        note(r)
        if a is None:
            assert np.array_equal(got["x"], np.minimum(np.maximum(0.0, l), u)) and (got["x"][l > 0] == l[l > 0]).all() and (l > 0).any()
        if b is None:
            assert not got["y"].any()
    sc = s.scalars()
    assert sc["kx"] == 0 and sc["ky"] == 0
    # 3. independence of history: the same start after seven iterations and a check step
    s.set_start(x0, y0)
    s.iterate(7, True)
    assert (s.get("x") != first["x"]).any() and (s.get("y") != first["y"]).any()
    s.set_start(x0, y0)
    again = read_start(s)
    for k in READ:
        assert np.array_equal(again[k], first[k]), (case, "after a history", k, int((again[k] != first[k]).sum()))
    res = s.residuals(0, True)
    assert {k: res[k] for k in NUMBERS} == numbers, (case, "after a history", res, numbers)
    # 4. the first iterations read the start: against the stream kernel with the same history
    if form != "stream":
        states = []
        for normal, check in ((1, False), (2, False), (0, True)):
            s.iterate(normal, check)
            states.append({name: s.get(name) for name in NAMES})
        assert (states[0]["x"] != first["x"]).any() and (states[0]["y"] != first["y"]).any()
        set_env(monkeypatch, "stream")
        s2 = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
        d = s2.describe()
        assert EXPECT["stream"] in d and "A^T: stream kernel" in d and "single-workgroup" not in d, d
        s2.scale()
        s2.init(SIGMA, lam)
        s2.set_start(x0, y0)
        s2.iterate(7, True)
        s2.set_start(x0, y0)
        for k in SEEDED_N + SEEDED_M:       # (the same scaled data on both: the seeded vectors are the same bits)
            assert np.array_equal(s2.get(k), first[k]), (case, "stream", k)
        s2.residuals(0, True)               # (as above: the iteration-0 evaluation leaves its bound-term vector in x_temp)
        for t, (normal, check) in enumerate(((1, False), (2, False), (0, True))):
            s2.iterate(normal, check)
            for name in NAMES:
                a, b = states[t][name], s2.get(name)
                where = "%s after %d more (%s)" % (case, (1, 3, 4)[t], name)
                if tol is None:
                    assert np.array_equal(a, b), (where, int((a != b).sum()), float(np.abs(a - b).max()))
                else:
                    np.testing.assert_allclose(a, b, rtol=tol[0], atol=tol[1], err_msg=where)
        s2.close()
    print("start", case, "LARGEST RATIOS", " | ".join("%s %.3g" % (k, worst[k]) for k in ("z_bar", "y_obj") + S.RESULTS + ("err_Rp", "err_Rd", "kkt")))
    s.close(); model.free()
