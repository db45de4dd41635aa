"""Group set-up, scaling and teardown of many small LPs (hprlp_solver_create_many / _scale_many / _destroy_many; csrc/many.cpp:
scale_many, csrc/alloc.cpp: the arena, the group forms of the scaling kernels in csrc/kernels.hip; DESIGN.md "Many small LPs").
The group path changes neither arithmetic nor order: every member must be bit for bit the solver that Solver(model, param) +
scale() give it alone.  So everything below is == or np.array_equal; nothing has a tolerance.  (Of scalars() the three wall times are left out:
they are clock readings, not results.)"""
import numpy as np
import pytest

import evalcases
from conftest import hprlp, lpgen
from test_gpu_many import SIX, assert_same_result, five, long_row_lp, make, planted, prepared  # noqa: F401  (five: a fixture)
from test_gpu_setup import with_env
from test_gpu_small import CHECK_VECS, VECS

pytestmark = pytest.mark.gpu

SCALED = ("A_val", "AT_val", "AL", "AU", "l", "u", "c", "row_norm", "col_norm")
TIMES = ("setup_time", "scaling_time", "power_time")
SWITCHES = {
    "default": {},
    "no-cr": dict(use_CR_scaling=False),
    "ruiz-only": dict(use_CR_scaling=False, use_Pock_Chambolle_scaling=False, use_bc_scaling=False),
    "pc-only": dict(use_CR_scaling=False, use_Ruiz_scaling=False, use_bc_scaling=False),
    "no-bc": dict(use_bc_scaling=False),
    "none": dict(use_CR_scaling=False, use_Ruiz_scaling=False, use_Pock_Chambolle_scaling=False, use_bc_scaling=False),
}
PLAN = [(1, False), (7, True)]
_lps = {}


def prm(name="default", **kw):
    return hprlp.Parameters(use_presolve=False, **SWITCHES[name], **kw)


def odd_rows_lp():
    """120 x 200: one 150-entry row and one 90-entry column (both matrices take the vector-mode branch of the matrix passes, above
    kLongRow = 64, and the model stays on the small path), one empty row and one empty column (the norms' < 1e-15 -> 1 rule and
    Curtis-Reid's cnt == 0)."""
    if "odd" not in _lps:
        A0 = lpgen.planted_lp(120, 200, 700, 17, dense_col_frac=0.0)["A"]
        A, facts = evalcases._with_lines(A0, (150,), (90,), 18, empty_rows=(0,), empty_cols=(0,))
        lr, lc = np.diff(A.indptr), np.diff(A.tocsc().indptr)
        assert lr.max() == 150 and lc.max() == 90 and (lr == 0).sum() >= 1 and (lc == 0).sum() >= 1, facts
        _lps["odd"] = evalcases.all_bounds_lp(A, 19)
    return _lps["odd"]


def eight_lps():
    """The six class shapes, the odd-rows LP and the LP with every bound kind (tests/evalcases.py: the small 400 x 600 case)."""
    if "eight" not in _lps:
        _lps["eight"] = [planted(s) for s in SIX] + [odd_rows_lp(), evalcases.case_lp("small", lpgen)]
    return _lps["eight"]


def same_scaled_solver(g, c, what):
    for k in SCALED:
        assert np.array_equal(g.get(k), c.get(k)), (what, k)
    sg, sc = g.scalars(), c.scalars()
    for k in sg:
        if k not in TIMES:
            assert sg[k] == sc[k], (what, k, sg[k], sc[k])
    assert g.info() == c.info(), (what, g.info(), c.info())


def same_first_iterations(group, ctrl, what):
    """power_iteration_many, init, the plan: iterates and check vectors equal the controls' (which go the same way alone)."""
    many = hprlp.Solver.power_iteration_many(group)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        lam, it = c.power_iteration()
        assert many[k] == (lam, it), (what, k, many[k], lam, it)
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    for normal, check in PLAN:
        hprlp.Solver.iterate_many(group, [normal] * len(group), check)
        for c in ctrl:
            c.iterate(normal, check)
        for k, (g, c) in enumerate(zip(group, ctrl)):
            for v in VECS + (CHECK_VECS if check else ()):
                assert np.array_equal(g.get(v), c.get(v)), (what, k, v)


def controls(models, prms):
    out = []
    for mod, p in zip(models, prms):
        s = hprlp.Solver(mod, p)
        s.scale()
        out.append(s)
    return out


def close(solvers, models=()):
    hprlp.Solver.close_many(solvers)
    for m in models:
        m.free()


@pytest.mark.parametrize("switches", list(SWITCHES))
def test_scaled_members_equal_their_own_create_and_scale(gpu, switches):
    """1 and 2: the bits of the scaled solver on eight LPs for one switch set, then the first iterations."""
    models = [make(lp) for lp in eight_lps()]
    p = prm(switches)
    group = hprlp.Solver.create_many(models, p)
    assert all(s is not None for s in group)
    hprlp.Solver.scale_many(group)
    cnt = hprlp.last_setup_many_counts()
    print(switches, cnt)
    assert cnt["members served by group scaling launches"] == 8 and cnt["members that scaled on their own"] == 0
    assert all(s.info()["tiled"] & 4 for s in group)  # (all on the small path)
    ctrl = controls(models, [p] * 8)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_scaled_solver(g, c, (switches, k))
    same_first_iterations(group, ctrl, switches)
    close(group + ctrl, models)


def test_members_with_different_switches_in_one_group(gpu):
    lps = eight_lps()[:6]
    models = [make(lp) for lp in lps]
    prms = [prm(name) for name in SWITCHES]
    # (create_many takes one parameter set: the members come from Solver(), which scale_many welcomes as well)
    group = [hprlp.Solver(mod, p) for mod, p in zip(models, prms)]
    hprlp.Solver.scale_many(group)
    assert hprlp.last_setup_many_counts()["members served by group scaling launches"] == 6
    ctrl = controls(models, prms)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_scaled_solver(g, c, list(SWITCHES)[k])
    same_first_iterations(group, ctrl, "mixed")
    close(group + ctrl, models)


def tiny_lps():
    """The smallest shapes that take every path of the group scaling: 40 x 70 and 70 x 40 (m > n) with 300 entries each, and
    5 x 130 with one row of 100 entries (the vector-mode branch of the matrix passes: more than kLongRow = 64) and one empty
    row.  No size is a multiple of 256."""
    if "tiny" not in _lps:
        from scipy import sparse
        rng = np.random.default_rng(23)

        def values(k):
            return rng.normal(size=k) * 0.3 + np.sign(rng.normal(size=k))

        def scattered(m, n, nnz):
            at = rng.choice(m * n, size=nnz, replace=False)
            return sparse.csr_matrix((values(nnz), (at // n, at % n)), shape=(m, n))

        wide = sparse.lil_matrix((5, 130))
        wide[0, np.sort(rng.choice(130, size=100, replace=False))] = values(100)
        for i in (2, 3, 4):  # (row 1 stays empty)
            wide[i, np.sort(rng.choice(130, size=12, replace=False))] = values(12)
        wide = sparse.csr_matrix(wide)
        assert np.diff(wide.indptr).tolist() == [100, 0, 12, 12, 12]
        _lps["tiny"] = [evalcases.all_bounds_lp(scattered(40, 70, 300), 24), evalcases.all_bounds_lp(wide, 25),
                        evalcases.all_bounds_lp(scattered(70, 40, 300), 26)]
    return _lps["tiny"]


def test_one_curtis_reid_member_among_three_tiny_ones(gpu):
    """A kind that holds ONE task inside a repeated stage (only the 5 x 130 member has Curtis-Reid on: its forty sweeps, exp / clamp
    and the Curtis-Reid scaling pass are tables of one task), a member with Ruiz off and Pock-Chambolle on (one sum-norm pass, no
    fused norms, the <*, *, false> matrix instances only) and without b / c scaling, a member with m > n.  Bits as everywhere in
    this file; the launches are one per kind present and stage, counted from Solver::scale()'s walk for these three switch sets:
    4 (fills, the two reductions, finalize) + 40 (sweeps) + 1 (exp / clamp) + 3 (vectors, two matrix instances) + 7 (pass 0: max
    norms of the first member, sum norms of the third, vectors, four matrix instances) + 8 x 3 (passes 1-8) + 3 (pass 9) + 4
    (pass 10: sum norms, vectors, two instances) + 3 (b / c reductions, finalize) + 1 (b / c passes) + 5 (reductions, finalize, two
    codes kernels) + 1 (zeroing) = 96, with three host waits."""
    lps = tiny_lps()
    models = [make(lp) for lp in lps]
    prms = [prm("no-cr"), prm("default"), prm("pc-only")]
    group = [hprlp.Solver(mod, p) for mod, p in zip(models, prms)]
    assert all(s.info()["tiled"] & 4 for s in group)  # (all on the small path)
    hprlp.Solver.scale_many(group)
    cnt = hprlp.last_setup_many_counts()
    print(cnt)
    assert cnt["members served by group scaling launches"] == 3 and cnt["members that scaled on their own"] == 0
    assert (cnt["scaling launches"], cnt["scaling host waits"]) == (96, 3), cnt
    ctrl = controls(models, prms)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_scaled_solver(g, c, ("tiny", k))
    same_first_iterations(group, ctrl, "tiny")
    close(group + ctrl, models)


def test_a_member_behaves_as_its_own_afterwards(gpu):
    """2, second half: buffers a member allocates after the arena's scope (value maps, staging, set_data's) work, and set_matrix /
    set_data / resolve leave it bit for bit where a handle created alone ends."""
    lps = [planted(SIX[0]), planted(SIX[4])]
    models = [make(lp) for lp in lps]
    p = prm(stop_tol=1e-6, max_iter=3000)  # (every solve below ends, whatever the changed values do to the LP)
    group = hprlp.Solver.create_many(models, p)
    hprlp.Solver.scale_many(group)
    g, c = group[0], hprlp.Solver(models[0], p)
    c.scale()
    lp = lps[0]
    rng = np.random.default_rng(5)
    vals = np.asarray(lp["values"]) * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, size=len(lp["values"])))
    for s in (g, c):
        lam, _ = s.power_iteration()
        s.init(-1.0, 1.01 * lam)
    first = (g.run(), c.run())
    assert_same_result(first[0], first[1], "first run")
    out = [s.set_matrix(vals, lp["c"], lp["AL"], lp["AU"], lp["l"], lp["u"]) for s in (g, c)]
    assert out[0] == out[1], out
    same_scaled_solver(g, c, "after set_matrix")
    res = [s.resolve() for s in (g, c)]
    assert_same_result(res[0], res[1], "resolve after set_matrix")
    for s in (g, c):
        s.set_data(c=1.001 * np.asarray(lp["c"]))
    res2 = [s.resolve() for s in (g, c)]
    assert_same_result(res2[0], res2[1], "resolve after set_data")
    assert {first[0].status, res[0].status, res2[0].status} <= {"OPTIMAL", "ITER_LIMIT"} and not np.array_equal(res2[0].x, res[0].x)
    c.close()
    close(group, models)


def test_a_member_off_the_small_path_scales_on_its_own(gpu):
    """3: long_row_lp() (a 300-entry row) in a group of four."""
    lps = [planted(SIX[0]), long_row_lp(), planted(SIX[4]), planted(SIX[2])]
    models = [make(lp) for lp in lps]
    p = prm()
    group = hprlp.Solver.create_many(models, p)
    assert not (group[1].info()["tiled"] & 4)
    hprlp.Solver.scale_many(group)
    cnt = hprlp.last_setup_many_counts()
    print(cnt)
    assert cnt["members that scaled on their own"] == 1 and cnt["members served by group scaling launches"] == 3
    ctrl = controls(models, [p] * 4)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_scaled_solver(g, c, k)
    same_first_iterations(group, ctrl, "with a long row")
    close(group + ctrl, models)


def test_counts_do_not_grow_with_the_group(gpu):
    """4: the 300 x 500 planted LP taken 5 and 20 times."""
    model = make(planted(SIX[0]))
    p = prm()
    seen = {}
    for K in (5, 20):
        group = hprlp.Solver.create_many([model] * K, p)
        hprlp.Solver.scale_many(group)
        cnt = hprlp.last_setup_many_counts()
        hprlp.Solver.close_many(group)
        cnt["device frees"] = hprlp.last_setup_many_counts()["device frees"]
        print(K, cnt)
        seen[K] = cnt
    one = hprlp.Solver.create_many([model], p)
    hprlp.Solver.scale_many(one)
    own = hprlp.last_setup_many_counts()
    hprlp.Solver.close_many(one)
    print("a group of one", own)
    assert own["members that scaled on their own"] == 1 and own["members served by group scaling launches"] == 0
    for k in ("scaling launches", "scaling host waits", "device allocations", "pinned allocations", "host-to-device copies", "device frees"):
        assert seen[5][k] == seen[20][k], (k, seen[5][k], seen[20][k])
    assert seen[5]["scaling host waits"] <= 4
    assert (seen[5]["members served by group scaling launches"], seen[20]["members served by group scaling launches"]) == (5, 20)
    # against a silent member-by-member fall-back: twenty members together take fewer launches than two members' own scale()
    assert 0 < seen[20]["scaling launches"] < 2 * own["scaling launches"], (seen[20]["scaling launches"], own["scaling launches"])
    model.free()


@pytest.mark.parametrize("together", [False, True])
def test_members_of_one_arena_go_in_any_order(gpu, together):
    """5: six created together; 0, 2 and 4 closed first; the other three run and equal their models' own solves; they go in
    reverse order; a new group comes up afterwards."""
    lps = [planted(s) for s in SIX]
    models = [make(lp) for lp in lps]
    p = prm(stop_tol=1e-6, max_iter=20000)
    group = hprlp.Solver.create_many(models, p)
    hprlp.Solver.scale_many(group)
    gone = [group[0], group[2], group[4]]
    if together:
        hprlp.Solver.close_many(gone)
    else:
        for s in gone:
            s.close()
    rest = [group[1], group[3], group[5]]
    for s in rest:
        lam, _ = s.power_iteration()
        s.init(-1.0, 1.01 * lam)
    out = hprlp.Solver.run_many(rest)
    for r, k in zip(out, (1, 3, 5)):
        assert_same_result(r, models[k].solve(p), k)
    if together:
        hprlp.Solver.close_many(rest[::-1])
    else:
        for s in rest[::-1]:
            s.close()
    again = hprlp.Solver.create_many(models[:2], p)
    hprlp.Solver.scale_many(again)
    ctrl = controls(models[:2], [p] * 2)
    for k in range(2):
        same_scaled_solver(again[k], ctrl[k], ("second group", k))
    close(again + ctrl, models)


def test_a_bad_model_among_good_ones(gpu):
    """6: a non-monotone row pointer array in position 1 of 3."""
    lps = [planted(SIX[0]), planted(SIX[4]), planted(SIX[2])]
    models = [make(lp) for lp in lps]
    rp = models[1]._ptr.contents.A.contents.rowPtr
    keep = rp[4]
    assert rp[3] > 0
    rp[4] = rp[3] - 1
    p = prm(stop_tol=1e-6, max_iter=20000)
    try:
        group = hprlp.Solver.create_many(models, p)
        assert group[1] is None and sum(s is not None for s in group) == 2
        assert "model 1" in hprlp.last_error() and "monotone" in hprlp.last_error()
        good = [group[0], group[2]]
        hprlp.Solver.scale_many(good)
        ctrl = controls([models[0], models[2]], [p] * 2)
        for k in range(2):
            same_scaled_solver(good[k], ctrl[k], k)
        out = hprlp.solve_many(models, p)
        assert out[1].status == "ERROR" and out[1].x is None
        for k in (0, 2):
            assert_same_result(out[k], models[k].solve(p), k)
        close(good + ctrl)
    finally:
        rp[4] = keep
    for m in models:
        m.free()


def test_solve_many_takes_the_group_path(gpu, five):
    """7: solve_many equals the singles, its five members were served by the group's scaling launches, and under the hook
    HPRLP_NO_GROUP_SETUP=1 the same bits come from the member-by-member set-up."""
    models, singles = five
    p = hprlp.Parameters(use_presolve=False, stop_tol=1e-6)
    out = hprlp.solve_many(models, p)
    cnt = hprlp.last_setup_many_counts()
    print(cnt, hprlp.last_solve_many_phases())
    for k in range(5):
        assert_same_result(out[k], singles[k], k)
    assert cnt["members served by group scaling launches"] == 5 and cnt["members that scaled on their own"] == 0
    off = with_env({"HPRLP_TEST_HOOKS": "1", "HPRLP_NO_GROUP_SETUP": "1"}, lambda: (hprlp.solve_many(models, p), hprlp.last_setup_many_counts()))
    print(off[1])
    for k in range(5):
        assert_same_result(off[0][k], singles[k], k)
    assert off[1]["members served by group scaling launches"] == 0 and off[1]["members that scaled on their own"] == 5
    assert off[1]["device allocations"] > cnt["device allocations"]


def test_refusals_leave_everything_untouched(gpu):
    """8: a NULL list, a zero count, a duplicate handle: -1 / RuntimeError with a message, zeroed counts, and a scaled member's
    vectors as they were."""
    import ctypes as C
    models = [make(planted(SIX[0])), make(planted(SIX[4]))]
    p = prm()
    good = hprlp.Solver.create_many(models, p)
    hprlp.Solver.scale_many(good)
    before = [{k: s.get(k) for k in SCALED} for s in good]
    L = hprlp.lib()
    hs = (C.c_void_p * 2)(good[0].h, good[1].h)
    out = (C.c_void_p * 2)()
    ptrs = (C.POINTER(hprlp.CLPInfo) * 2)(models[0]._ptr, models[1]._ptr)
    cp = p.to_c()
    calls = [(lambda: L.hprlp_solver_scale_many(None, 2), "null solver list"),
             (lambda: L.hprlp_solver_scale_many(hs, 0), "count must be positive"),
             (lambda: L.hprlp_solver_create_many(None, 2, C.byref(cp), out), "null model list"),
             (lambda: L.hprlp_solver_create_many(ptrs, 0, C.byref(cp), out), "count must be positive")]
    for call, word in calls:
        assert call() == -1
        assert word in hprlp.last_error(), (word, hprlp.last_error())
    with pytest.raises(RuntimeError, match="same solver"):
        hprlp.Solver.scale_many([good[0], good[1], good[0]])
    cnt = hprlp.last_setup_many_counts()
    assert all(cnt[k] == 0 for k in hprlp.SETUP_MANY_KEYS[:7]), cnt
    L.hprlp_solver_destroy_many(None, 2)       # (void: a NULL list and a zero count are no-ops)
    L.hprlp_solver_destroy_many(hs, 0)
    for s, b in zip(good, before):
        for k in b:
            assert np.array_equal(s.get(k), b[k]), k
    close(good, models)
