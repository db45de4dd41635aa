"""The infeasibility detection's ray test BY VALUE on every kernel form (GPU): the nine device scalars of Solver::ray_test --
k_ray_form's six, RayColEpi's two and RayRowEpi's one, with the max accumulators of block_store_partials and the max items of
k_finalize that only they use -- behind hprlp_solver_ray_step, against tests/evalref.py's evaluate_rays ON THE SOLVER'S OWN
READ-BACK scaled data and rays, within 2 x the derived bound of that module and nothing wider.

Per form (evalcases.CASES: the smallest shapes at which existing tests show each form selected; the hook sets of
tests/test_gpu_detect.py: FORM_ENV) one step with random rays, then TARGETED rays that put the maximum of a slot on one chosen
line -- the first, the last, one inside the last block, every line the case was built around (rows of 64 to 5000 entries, rows
and columns kept aside from a tiled copy), a neighbour of an empty line -- with the runner-up below half of it on the reference,
so an epilogue that skips that line, or a reduction that drops its block, is out of bounds.  (A targeted line gets the bound
kind its slot needs through set(), and the few lines that share entries with a short targeted line and would come within 0.4 of
it get, for that step, the kind that keeps them out of the maximum: no iterates are compared here.)  For every targeted slot the
evaluator with that line (or one entry of it) left out, and for the sums the evaluator with the wrong bound side, is shown to be
farther than the tolerance from the GPU's number: the comparison can see the fault it is there for.  No vector here is
kThreads * kReduceBlocks = 131072 long, so k_ray_form's grid-stride loops take one trip; their targets are index 0 and the last.
The REORDERED form: tests/test_gpu_reorder_small.py holds the nine scalars and the four ray vectors of a solver with a locality
ordering (HPRLP_REORDER_ANYWAY, 20 011 x 26 003) to a solver on the explicitly permuted LP, bit for bit; tests/test_gpu_reorder.py
checks the permutation of the four vector names at 1.6 M rows.

A step writes nothing but its own buffers (the eleven state vectors keep their bits, later iterations are those of a solver that
never stepped), and a later run() with detection starts clean.

Largest observed-difference / bound ratio per slot and form, MI355X (the tolerance is 2):

| form | DY | CD | VY | WD | YN | DN | DZ | VZ | WQ | D | V | cd | W | yn | dn |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|
| small | 0.0052 | 0.008 | 0.63 | 0.38 | 0.54 | 0.38 | 0.0051 | 0.14 | 0.17 | 0.0039 | 0.14 | 0.008 | 0.17 | 0.54 | 0.38 |
| stream-short | 0.00036 | 0.00026 | 0.31 | 0.46 | 0.42 | 0.44 | 0.00053 | 0.19 | 0.093 | 0.00046 | 0.19 | 0.00026 | 0.46 | 0.42 | 0.44 |
| stream-rows | 0.00053 | 0.00013 | 0.66 | 0.49 | 0.64 | 0.49 | 0.0002 | 0.014 | 0.001 | 0.00018 | 0.37 | 0.00013 | 0.001 | 0.64 | 0.49 |
| tiled | 9.3e-05 | 6.3e-05 | 0.56 | 0.41 | 0.46 | 0.41 | 0.00013 | 0.16 | 0.15 | 0.00012 | 0.16 | 6.3e-05 | 0.12 | 0.46 | 0.41 |
| tiled-rounds | 2.2e-05 | 4.3e-05 | 0.27 | 0.36 | 0.35 | 0.66 | 1.2e-05 | 0.14 | 0.076 | 9.9e-06 | 0.14 | 4.3e-05 | 0.076 | 0.35 | 0.66 |
| pieces | 5.5e-05 | 7.9e-05 | 0.31 | 0.49 | 0.26 | 0.49 | 7.7e-05 | 0.16 | 0.092 | 7.8e-05 | 0.16 | 7.9e-05 | 0.48 | 0.26 | 0.49 |
| all-remainder | 0.00027 | 0.0002 | 0.51 | 0.5 | 0.51 | 0.51 | 0.00043 | 0.14 | 0.17 | 0.00041 | 0.14 | 0.0002 | 0.17 | 0.51 | 0.51 |
| tiled-aside | 7.5e-05 | 4.6e-05 | 0.63 | 0.61 | 0.36 | 0.61 | 0.00011 | 0.0011 | 0.00058 | 0.00015 | 0.0011 | 4.6e-05 | 0.00058 | 0.36 | 0.61 |
| worst | 0.0052 | 0.008 | 0.66 | 0.61 | 0.64 | 0.66 | 0.0051 | 0.19 | 0.17 | 0.0039 | 0.37 | 0.008 | 0.48 | 0.64 | 0.66 |
"""
import numpy as np
import pytest

import evalcases as C
import evalref as E
from conftest import hprlp, lpgen
from test_gpu_detect import model_of
from test_gpu_evaluation import NAMES, assert_form, make, set_form

pytestmark = pytest.mark.gpu


def _nonempty_near(lens, k):
    """the line nearest to k (k itself first, then k + 1, k - 1, ...) that stores an entry"""
    for step in range(len(lens)):
        for cand in (k + step, k - step):
            if 0 <= cand < len(lens) and lens[cand] > 0:
                return int(cand)
    raise AssertionError("no stored entry")


def target_lines(lens, built_around, empty):
    """The lines the SpMV epilogues are targeted at: first, last, one inside the last (ragged) block, the lines the case was built
    around, the neighbours of an empty line; each moved to the nearest line that stores an entry."""
    last = len(lens) - 1
    want = [0, last, last - 7] + sorted(built_around)
    for e in empty[:1]:
        want += [e - 1, e + 1]
    out = []
    for k in want:
        k = _nonempty_near(lens, min(max(k, 0), last))
        if k not in out:
            out.append(k)
    return out


def ray_value_steps(s, lp, patterns, case, note):
    """Steps 1 to 3 of a case on the solver s (after its check step).  Returns the bound arrays as they were before the targeted
    steps changed them."""
    m, n = lp["m"], lp["n"]
    fin = np.isfinite
    # 1. the start: before the first begin the four vectors are unknown names; the first step only stores the iterate
    with pytest.raises(RuntimeError):
        s.get("ray_prev_x")
    with pytest.raises(RuntimeError):
        s.ray_step()                       # (no stored iterate and none asked for)
    assert s.ray_step(restart=True) is None
    px, py = s.get("ray_prev_x"), s.get("ray_prev_y")
    assert np.array_equal(px, s.get("x_bar")) and np.array_equal(py, s.get("y_bar")) and len(px) == n and len(py) == m

    def step(ds_t, ys_t, label):
        """x_bar = prev_x + ds_t, y_bar = prev_y + ys_t, one ray_step: the rays and the stored iterate by bits, the fifteen numbers
        by value, and the eleven state vectors untouched"""
        px, py = s.get("ray_prev_x"), s.get("ray_prev_y")
        s.set("x_bar", px + ds_t)
        s.set("y_bar", py + ys_t)
        before = {k: s.get(k) for k in NAMES}
        got = s.ray_step()
        assert got is not None
        after = {k: s.get(k) for k in NAMES}
        for k in NAMES:
            assert np.array_equal(before[k], after[k]), (label, k)
        # one subtraction is the same bits anywhere
        assert np.array_equal(s.get("ray_d"), after["x_bar"] - px) and np.array_equal(s.get("ray_y"), after["y_bar"] - py), label
        assert np.array_equal(s.get("ray_prev_x"), after["x_bar"]) and np.array_equal(s.get("ray_prev_y"), after["y_bar"]), label
        for a, b in (("D", got["DY"] + got["DZ"]), ("V", max(got["VY"], got["VZ"])), ("cd", got["CD"]), ("W", max(got["WD"], got["WQ"])),
                     ("yn", got["YN"]), ("dn", got["DN"])):
            assert got[a] == b, (label, a)
        inp, (ds, ys), want, r = E.check_rays(s, patterns, got, case + " " + label)
        note(r)
        return got, inp, ds, ys, want

    def dominated(want, got, inp, ds, ys, slot, line, label, **drop):
        """the reference shows `line` as the arg-max of `slot` with the runner-up below half of it, and the evaluator without that
        line (and without one entry of it) is farther than the tolerance from the GPU's number"""
        k, top, second = E.top_two(want["elements"][slot])
        assert k == line and top > 0 and second <= 0.5 * top, (label, slot, line, k, top, second)
        bad = E.evaluate_rays(*inp, ds, ys, leave_out={slot: line})
        assert E.ratio(got[slot], bad[slot]) > E.TOL_FACTOR, (label, slot, got[slot], bad[slot])
        if drop:
            bad = E.evaluate_rays(*inp, ds, ys, **drop)
            assert E.ratio(got[slot], bad[slot]) > E.TOL_FACTOR, (label, slot, drop, got[slot], bad[slot])

    # 2. random rays, every bound kind on both signs; a sum with the wrong bound side is seen
    ds0, ys0 = E.random_rays(m, n, 5)
    got, inp, ds, ys, want = step(ds0, ys0, "random rays")
    assert (ds == 0).sum() >= n // 16 and (ys == 0).sum() >= m // 16
    assert all(abs(got[k]) > 0 for k in E.RAY_NAMES), got
    bad = E.ratios(got, E.evaluate_rays(*inp, ds, ys, swap_sides=True), ("DY", "DZ", "D"))
    assert min(bad.values()) > E.TOL_FACTOR, bad

    # 3. targeted rays.  The bound kinds the targeted slots need, on the targeted lines only: a column whose z_j > 0 is to count
    # as a violation has no lower bound, a row whose q_i > 0 is to count has an upper side; for k_ray_form's maxima at index 0 and
    # the last index y_i > 0 needs a row without a lower side and d_j > 0 a column with an upper bound.
    A, AT, data, sc = inp
    orig = {k: data[k].copy() for k in ("l", "u", "AL", "AU")}
    facts = lp["facts"] or {}
    cols = target_lines(np.diff(AT[0]), facts.get("cols", ()), facts.get("empty_cols", []))
    rows = target_lines(np.diff(A[0]), facts.get("rows", ()), facts.get("empty_rows", []))
    assert set(facts.get("cols", ())) <= set(cols) and set(facts.get("rows", ())) <= set(rows)
    ends_n, ends_m = [0, n - 1], [0, m - 1]
    l, u, AL, AU = (orig[k].copy() for k in ("l", "u", "AL", "AU"))
    l[cols] = -np.inf
    u[ends_n] = np.where(fin(u[ends_n]), u[ends_n], 1.0)
    AU[rows] = np.where(fin(AU[rows]), AU[rows], 1.0)
    AL[ends_m] = -np.inf
    AU[ends_m] = np.where(fin(AU[ends_m]), AU[ends_m], 1.0)
    for name, v in (("l", l), ("u", u), ("AL", AL), ("AU", AU)):
        s.set(name, v)
    cn, rn = data["col_norm"], data["row_norm"]
    for which, (j, i) in (("index 0", (0, 0)), ("the last index", (n - 1, m - 1))):
        label = "k_ray_form's maxima at " + which
        got, inp, ds, ys, want = step(E.boosted(ds0, cn, j, 1.0), E.boosted(ys0, rn, i, 1.0), label)
        for slot, line in (("WD", j), ("DN", j), ("VY", i), ("YN", i)):
            dominated(want, got, inp, ds, ys, slot, line, label)
    # ys = -(column j of the scaled A) gives z_j = cn_j c_scale sum a^2, ds = +(row i) gives q_i = rn_i b_scale sum a^2.  A line that
    # shares an entry's row or column with a short targeted line can come close to it (its norm may be much the larger): such
    # rivals, the elements above 0.4 of the target's on the reference, get the kind that keeps them out of the maximum for this
    # step (both column bounds finite, a free row), again through set().
    for k in range(max(len(cols), len(rows))):
        j, i = cols[min(k, len(cols) - 1)], rows[min(k, len(rows) - 1)]
        label = "column %d (%d entries), row %d (%d entries)" % (j, AT[0][j + 1] - AT[0][j], i, A[0][i + 1] - A[0][i])
        ds_t, ys_t = E.line_of(A, i, n, 1.0), E.line_of(AT, j, m, -1.0)
        pre = E.evaluate_rays(A, AT, dict(data, l=l, u=u, AL=AL, AU=AU), sc, ds_t, ys_t)["elements"]
        rc, rr = np.flatnonzero(pre["VZ"] > 0.4 * pre["VZ"][j]), np.flatnonzero(pre["WQ"] > 0.4 * pre["WQ"][i])
        rc, rr = rc[rc != j], rr[rr != i]
        assert pre["VZ"][j] > 0 and pre["WQ"][i] > 0 and len(rc) <= 16 and len(rr) <= 16, (label, len(rc), len(rr))
        l2, u2, AL2, AU2 = l.copy(), u.copy(), AL.copy(), AU.copy()
        l2[rc], u2[rc] = np.where(fin(l[rc]), l[rc], -1.0), np.where(fin(u[rc]), u[rc], 1.0)
        AL2[rr], AU2[rr] = -np.inf, np.inf
        for name, v in (("l", l2), ("u", u2), ("AL", AL2), ("AU", AU2)):
            s.set(name, v)
        label += ", %d + %d rivals" % (len(rc), len(rr))
        got, inp, ds, ys, want = step(ds_t, ys_t, label)
        dominated(want, got, inp, ds, ys, "VZ", j, label, drop_AT=E.largest_entry(AT, j))
        dominated(want, got, inp, ds, ys, "WQ", i, label, drop_A=E.largest_entry(A, i))
    return orig


def prepared(lp, case, form, sigma=0.6, oracle=True):
    """a solver after scale(), the real lambda_max, init and 17 normal iterations with a check step (the oracle's ScaledLP serves
    for the pattern of the transpose only)"""
    if oracle:
        model, s, ref = make(lp)
    else:
        model, ref = model_of(lp), None
        s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    assert_form(s, case, form)
    s.scale()
    lam = 1.01 * s.power_iteration()[0]
    s.init(sigma, lam)
    s.iterate(17, True)
    return model, s, ref


@pytest.mark.parametrize("case", list(C.CASES))
def test_ray_slots_by_value_on_every_kernel_form(gpu, case, monkeypatch):
    form, _ = set_form(monkeypatch, case)
    lp = C.case_lp(case, lpgen)
    model, s, ref = prepared(lp, case, form)
    patterns = (lp["rowptr"], lp["colind"], ref.ATrp, ref.ATci)
    at_check = {k: s.get(k) for k in NAMES}
    worst = {}

    def note(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)

    orig = ray_value_steps(s, lp, patterns, case, note)
    print("rays", case, "LARGEST RATIOS", " | ".join("%s %.3g" % (k, worst[k]) for k in E.RAY_NAMES))
    # 4. with the bounds and the check step's x_bar / y_bar put back, the eleven state vectors are the check step's bits, and nine
    # iterations and a check step on are the bits of a solver that never stepped (the tiled forms' remainder buffers were
    # invalidated before the ray SpMVs refilled them)
    for name, v in orig.items():
        s.set(name, v)
    s.set("x_bar", at_check["x_bar"])
    s.set("y_bar", at_check["y_bar"])
    for k in NAMES:
        assert np.array_equal(s.get(k), at_check[k]), k
    s.iterate(9, True)
    model2, s2, _ = prepared(lp, case, form, oracle=False)
    for k in NAMES:
        assert np.array_equal(s2.get(k), at_check[k]), k
    s2.iterate(9, True)
    for k in NAMES:
        a, b = s.get(k), s2.get(k)
        assert np.array_equal(a, b), (k, int((a != b).sum()), float(np.abs(a - b).max()))
    assert np.abs(s.get("x")).max() > 0 and s.scalars()["kx"] == s2.scalars()["kx"] == 28
    s.close(); model.free()
    s2.close(); model2.free()


def _planted_infeasible(case):
    """the planted infeasible LPs of tests/test_gpu_detect.py: FORM_SCRIPT"""
    from scipy import sparse
    if case == "small":
        return lpgen.planted_infeasible_lp(400, 600, 2400, 21)
    rp, ci, v = lpgen.banded_csr(8000, 10000, 8, 1500, 6)
    A = sparse.csr_matrix((v, ci, rp), shape=(8000, 10000))
    A.sum_duplicates()
    A.sort_indices()
    return lpgen.planted_infeasible_lp(8000, 10000, 0, 23, A=A)


@pytest.mark.parametrize("case", ["small", "tiled"])
def test_a_later_run_starts_clean(gpu, case, monkeypatch):
    """set_detection() + run() on a fresh init after ray steps: the status, iteration and certificate bits of a solver that never
    stepped (the steps leave no stored iterate behind, and the detection setting is the caller's)."""
    form, _ = set_form(monkeypatch, case)
    lp = _planted_infeasible(case)
    outs = []
    for stepped in (False, True):
        model = model_of(lp)
        s = hprlp.Solver(model, hprlp.Parameters(max_iter=50000, use_presolve=False))
        assert_form(s, case, form)
        s.scale()
        lam = 1.01 * s.power_iteration()[0]
        if stepped:
            s.init(-1.0, lam)
            s.iterate(17, True)
            assert s.ray_step(restart=True) is None
            ds, ys = E.random_rays(lp["m"], lp["n"], 6)
            s.set("x_bar", s.get("x_bar") + ds)
            s.set("y_bar", s.get("y_bar") + ys)
            assert s.ray_step() is not None
            s.reset()
        s.init(-1.0, lam)
        s.set_detection()
        r = s.run(max_trace=1)
        k = s.certificate()
        outs.append((r.status, r.iter, k.kind, k.iter, k.objective, k.violation, k.y.copy(), k.z.copy()))
        s.close(); model.free()
    a, b = outs
    assert a[0] == "PRIMAL_INFEASIBLE" and a[2] == 1 and a[:6] == b[:6], (a[:6], b[:6])
    assert np.array_equal(a[6], b[6]) and np.array_equal(a[7], b[7])
