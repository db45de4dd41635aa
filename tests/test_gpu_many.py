"""Many small LPs at once on the GPU (hpr-lp-c_amd/csrc/many.cpp, k_small_iterations_many / k_small_power_many in small.hip;
DESIGN.md "Many small LPs").  The criterion throughout is equality of BITS with the single-LP path: a workgroup of a group kernel
runs the single kernel's arithmetic on the same inputs, and every check step, evaluation and host rule is the member's own.  So
everything below is np.array_equal or ==; nothing has a tolerance."""
import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_detect import EDGE, as_lp
from test_gpu_small import CHECK_VECS, VECS, make
from test_resolve import base_lp, changed

pytestmark = pytest.mark.gpu

# (m, n, nnz, seed) -> kernel class <KMAX, R>: the shapes of tests/test_gpu_small.py, the smallest that reach every instance
CLASS_SHAPES = [(300, 500, 2500, 5),      # <4, 1>
                (600, 1500, 3500, 5),     # <4, 2>
                (500, 1000, 7500, 5),     # <8, 1>
                (821, 1571, 10700, 5)]    # <12, 2>
SECOND = (400, 650, 4000, 8)              # <4, 1> again: a launch with grid 2
SIX = CLASS_SHAPES + [SECOND, (821, 1571, 7000, 5)]  # ... and <8, 2>
FIELDS = ("status", "iter", "iter4", "iter6", "primal_obj", "residuals", "gap")


def planted(shape):
    m, n, nnz, seed = shape
    return lpgen.planted_lp(m, n, nnz, seed, dense_col_frac=0.01 if m != 300 else 0.0)


def long_row_lp():
    """The LP of tests/test_gpu_small.py::test_rows_too_long_for_the_small_path_fall_back: a 300-entry row, off the small path."""
    from scipy import sparse
    rng = np.random.default_rng(3)
    lp = lpgen.planted_lp(200, 600, 1500, 6)
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(200, 600)).tolil()
    for j in rng.choice(600, size=300, replace=False):
        A[0, j] = 1.0
    A = A.tocsr(); A.sort_indices()
    b = A @ (np.abs(lp["x_star"]) + 0.1)
    return dict(m=200, n=600, rowptr=A.indptr, colind=A.indices, values=A.data, AL=b - 1.0, AU=b + 1.0, l=np.zeros(600),
                u=np.full(600, 10.0), c=lp["c"])


def assert_same_result(a, b, what):
    for f in FIELDS:
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))
    for f in ("x", "y", "z"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


def close_all(solvers, models=()):
    for s in solvers:
        s.close()
    for m in models:
        m.free()


@pytest.fixture(scope="module")
def five():
    """The four classes and the 25fv47-like LP: models, and each one's own solve at 1e-6 (computed once, never changed)."""
    lps = [planted(s) for s in CLASS_SHAPES] + [lpgen.c2_25fv47_like()]
    models = [make(lp) for lp in lps]
    singles = [m.solve(hprlp.Parameters(use_presolve=False, stop_tol=1e-6)) for m in models]
    yield models, singles
    for m in models:
        m.free()


def prepared(models, prms=None, scale_only=False):
    out = []
    for k, m in enumerate(models):
        s = hprlp.Solver(m, prms[k] if prms else hprlp.Parameters(use_presolve=False))
        s.scale() if scale_only else s.prepare()
        out.append(s)
    return out


def test_iterates_equal_the_single_launches_bit_for_bit(gpu):
    """Six solvers against six controls through the plan of tests/test_gpu_small.py; one round gives the two members of one class
    7 and 6 iterations, one round gives a member none."""
    models = [make(planted(s)) for s in SIX]
    group, ctrl = prepared(models, scale_only=True), prepared(models, scale_only=True)
    assert all(s.info()["tiled"] & 4 for s in group)
    for g, c in zip(group, ctrl):
        lam, _ = c.power_iteration()
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    plan = [(1, False), (7, True), (64, False), (149, True), (3, False)]
    for step, (normal, check) in enumerate(plan):
        counts = [normal] * 6
        if step == 1:
            counts[4] = 6          # members 0 and 4 share <4, 1>: different counts inside one launch
        if step == 2:
            counts[2] = 0          # no task at all for this member
            before = {k: group[2].get(k) for k in VECS}
            k_before = (group[2].scalars()["kx"], group[2].scalars()["ky"])
        hprlp.Solver.iterate_many(group, counts, check)
        for c, cnt in zip(ctrl, counts):
            c.iterate(cnt, check)
        for i, (g, c) in enumerate(zip(group, ctrl)):
            for k in VECS + (CHECK_VECS if check else ()):
                assert np.array_equal(g.get(k), c.get(k)), (step, i, k)
            sg, sc = g.scalars(), c.scalars()
            assert (sg["kx"], sg["ky"]) == (sc["kx"], sc["ky"]), (step, i)
        if step == 2:
            assert all(np.array_equal(group[2].get(k), before[k]) for k in VECS)
            assert (group[2].scalars()["kx"], group[2].scalars()["ky"]) == k_before
    assert group[0].scalars()["kx"] != group[4].scalars()["kx"]  # (the 7 / 6 round left them apart)
    close_all(group + ctrl, models)


def test_power_iterations_equal_the_single_launches(gpu):
    models = [make(planted(s)) for s in SIX]
    group = prepared(models, scale_only=True)
    many = hprlp.Solver.power_iteration_many(group)
    alone = [s.power_iteration() for s in group]
    print("power iterations", many)
    assert many == alone, (many, alone)
    assert len({it for _, it in many}) > 1       # (not one count for all: every workgroup stopped on its own test)
    capped = hprlp.Solver.power_iteration_many(group, max_iter=25)
    assert [it for _, it in capped] == [25] * 6
    assert capped == [s.power_iteration(max_iter=25) for s in group]
    close_all(group, models)


def test_solve_many_equals_each_models_own_solve(gpu, five):
    models, singles = five
    out = hprlp.solve_many(models, hprlp.Parameters(use_presolve=False, stop_tol=1e-6))
    print("iterations", [r.iter for r in singles], hprlp.last_solve_many_phases())
    assert [r.status for r in singles] == ["OPTIMAL"] * 5
    assert len({r.iter for r in singles}) == 5   # they finish at different iterations: the group is seen to shrink
    for k in range(5):
        assert_same_result(out[k], singles[k], k)
    # one wait per evaluation round (+ two per restart of a member), one launch per class present: neither grows with the count
    ph = hprlp.last_solve_many_phases()
    assert ph["launches"] <= 5 * ph["rounds"]


def test_iteration_limit_between_the_fastest_and_the_slowest(gpu, five):
    models, singles = five
    iters = sorted(r.iter for r in singles)
    cap = (iters[0] + iters[-1]) // 2
    assert iters[0] < cap < iters[-1]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-6, max_iter=cap)
    out = hprlp.solve_many(models, prm)
    for k in range(5):
        if singles[k].iter <= cap:
            assert out[k].status == "OPTIMAL" and out[k].iter == singles[k].iter, k
            assert_same_result(out[k], singles[k], k)
        else:
            assert out[k].status == "ITER_LIMIT" and out[k].iter == cap, (k, out[k].status, out[k].iter)
            assert_same_result(out[k], models[k].solve(prm), k)
    assert {r.status for r in out} == {"OPTIMAL", "ITER_LIMIT"}


def test_a_member_off_the_small_path_rides_along(gpu):
    lps = [long_row_lp(), planted(CLASS_SHAPES[0]), planted(SECOND)]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-6)
    s = hprlp.Solver(models[0], prm)
    assert not (s.info()["tiled"] & 4)
    s.close()
    out = hprlp.solve_many(models, prm)
    for k, m in enumerate(models):
        assert_same_result(out[k], m.solve(prm), k)
    assert out[1].status == out[2].status == "OPTIMAL"
    close_all((), models)


def test_detection_rides_along(gpu):
    """Member 0: the smallest infeasible LP of tests/test_gpu_detect.py with detection on -- the same verdict, iteration and
    certificate as hprlp_solver_run alone, while the other members end OPTIMAL."""
    lps = [as_lp(EDGE["infeasible"]), planted(CLASS_SHAPES[0]), planted(SECOND)]
    models = [make(lp) for lp in lps]
    prms = [hprlp.Parameters(use_presolve=False, stop_tol=1e-8, max_iter=3000)] + [hprlp.Parameters(use_presolve=False, stop_tol=1e-6)] * 2
    group, ctrl = prepared(models, prms), prepared(models, prms)
    group[0].set_detection()
    ctrl[0].set_detection()
    out = hprlp.Solver.run_many(group)
    alone = [c.run() for c in ctrl]
    assert [r.status for r in out] == ["PRIMAL_INFEASIBLE", "OPTIMAL", "OPTIMAL"]
    for k in range(3):
        assert_same_result(out[k], alone[k], k)
    kg, kc = group[0].certificate(), ctrl[0].certificate()
    assert kg.kind == kc.kind == 1 and kg.iter == kc.iter == out[0].iter
    assert (kg.objective, kg.violation) == (kc.objective, kc.violation)
    assert np.array_equal(kg.y, kc.y) and np.array_equal(kg.z, kc.z)
    assert group[1].certificate().kind == 0
    close_all(group + ctrl, models)


def test_a_start_rides_along(gpu):
    lps = [planted(CLASS_SHAPES[0]), planted(SECOND)]
    models = [make(lp) for lp in lps]
    prms = [hprlp.Parameters(use_presolve=False, stop_tol=1e-6)] * 2
    group, ctrl = prepared(models, prms), prepared(models, prms)
    x0 = 0.9 * lps[1]["x_star"]
    group[1].set_start(x0, None)
    ctrl[1].set_start(x0, None)
    out = hprlp.Solver.run_many(group)
    alone = [c.run() for c in ctrl]
    for k in range(2):
        assert_same_result(out[k], alone[k], k)
    cold = models[1].solve(prms[1])
    assert out[1].iter != cold.iter or not np.array_equal(out[1].x, cold.x)  # (the start was not ignored)
    close_all(group + ctrl, models)


def test_changed_data_then_a_second_run_equals_resolve(gpu):
    """set_data (a new c on one member, new row sides on the other), reset, init: the second run_many on the same handles equals
    resolve() on control solvers that went the same way alone."""
    lps = [base_lp(11), base_lp(12)]
    models = [make(lp) for lp in lps]
    prms = [hprlp.Parameters(use_presolve=False, stop_tol=1e-6)] * 2
    group, ctrl = prepared(models, prms), prepared(models, prms)
    first = hprlp.Solver.run_many(group)
    for k, c in enumerate(ctrl):
        assert_same_result(first[k], c.run(), k)
    new = [changed(lps[0], "c1e-3"), changed(lps[1], "rows1e-3")]
    for s in (group, ctrl):
        s[0].set_data(c=new[0]["c"])
        s[1].set_data(AL=new[1]["AL"], AU=new[1]["AU"], l=new[1]["l"], u=new[1]["u"])
    for g in group:
        lam = g.scalars()["lambda_max"]
        g.reset()
        g.init(-1.0, lam)
    second = hprlp.Solver.run_many(group)
    for k, c in enumerate(ctrl):
        r = c.resolve()
        assert_same_result(second[k], r, k)
        assert second[k].status == "OPTIMAL" and not np.array_equal(second[k].x, first[k].x)
    close_all(group + ctrl, models)


def test_refusals_leave_the_members_untouched(gpu):
    """A sharded handle, the same handle twice, a solver never scaled, a negative count: -1 with a message, and the members'
    vectors are the same before and after."""
    lps = [planted(CLASS_SHAPES[0]), planted(SECOND)]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False)
    good = prepared(models)
    hprlp.Solver.iterate_many(good, [5, 5], True)
    before = [{k: s.get(k) for k in VECS + CHECK_VECS} for s in good]
    local = hprlp.Solver.local_group(1)
    sharded = hprlp.Solver.create_local(models[0], prm, 0, 1, local)
    sharded.scale()
    unscaled = hprlp.Solver(models[1], prm)
    cases = [([good[0], sharded, good[1]], [3, 3, 3], "sharded"), ([good[0], good[1], good[0]], [3, 3, 3], "same solver"),
             ([good[0], unscaled], [3, 3], "never scaled"), ([good[0], good[1]], [3, -1], "negative")]
    for members, counts, word in cases:
        calls = [lambda: hprlp.Solver.iterate_many(members, counts, True)]
        if word != "negative":
            calls += [lambda: hprlp.Solver.run_many(members), lambda: hprlp.Solver.power_iteration_many(members)]
        for call in calls:
            with pytest.raises(RuntimeError, match=word):
                call()
    for s, b in zip(good, before):
        for k in b:
            assert np.array_equal(s.get(k), b[k]), k
    sharded.close()
    unscaled.close()
    hprlp.Solver.free_local_group(local)
    close_all(good, models)
