"""Check step, evaluation and restart of many small LPs in one launch per kernel (kernels.hip: k_spmv_fused_many and the group forms
of k_finalize / k_movement / k_restart_copy / k_set_ctrl; many.cpp; DESIGN.md "Many small LPs").  A workgroup of a group kernel
runs the single kernel's body as workgroup lb of lg of its member, so the criterion is the one of tests/test_gpu_many.py: equality
of BITS with the member's own launches.  Everything below is == or np.array_equal; nothing has a tolerance."""
import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_detect import EDGE, as_lp
from test_gpu_many import CLASS_SHAPES, FIELDS, SECOND, SIX, assert_same_result, close_all, five, long_row_lp, planted, prepared  # noqa: F401
from test_gpu_small import CHECK_VECS, VECS, make

pytestmark = pytest.mark.gpu

TINY = (30, 50, 200, 3)   # one workgroup per launch on either matrix
ALL_VECS = VECS + CHECK_VECS
KEYS = ("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt", "weighted_norm", "lambda_max")


def seven_lps():
    return [planted(s) for s in SIX] + [lpgen.planted_lp(*TINY)]


def two_groups():
    """Seven models, a group and its controls, scaled and initialised with each control's own lambda."""
    models = [make(lp) for lp in seven_lps()]
    group, ctrl = prepared(models, scale_only=True), prepared(models, scale_only=True)
    for g, c in zip(group, ctrl):
        lam, _ = c.power_iteration()
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    return models, group, ctrl


def assert_same_state(group, ctrl, vecs, what):
    for i, (g, c) in enumerate(zip(group, ctrl)):
        for k in vecs:
            assert np.array_equal(g.get(k), c.get(k)), (what, i, k)
        sg, sc = g.scalars(), c.scalars()
        assert (sg["kx"], sg["ky"], sg["sigma"], sg["lambda_max"]) == (sc["kx"], sc["ky"], sc["sigma"], sc["lambda_max"]), (what, i)


def assert_same_residuals(many, alone, what):
    for i, (a, b) in enumerate(zip(many, alone)):
        for k in KEYS:
            assert a[k] == b[k], (what, i, k, a[k], b[k])


def test_the_group_holds_the_grid_shapes_that_matter(gpu):
    """From hprlp_solver_info: every member is on the small path without a tiled copy; the group holds a y-half grid that is no
    multiple of 8 (the remainder branch of the XCD remap), a grid of 1 (TINY) and different grids inside one launch."""
    models = [make(lp) for lp in seven_lps()]
    group = prepared(models, scale_only=True)
    info = [s.info() for s in group]
    print("grids (y, x)", [(d["grid_y"], d["grid_x"]) for d in info])
    assert all(d["tiled"] == 4 for d in info)
    assert any(d["grid_y"] % 8 != 0 and d["grid_y"] > 1 for d in info)
    assert any(d["grid_y"] > 8 and d["grid_y"] % 8 != 0 for d in info) or any(d["grid_x"] > 8 and d["grid_x"] % 8 != 0 for d in info)
    assert info[-1]["grid_y"] == 1 and info[-1]["grid_x"] == 1
    assert len({d["grid_y"] for d in info}) > 1 and len({d["grid_x"] for d in info}) > 1
    close_all(group, models)


def test_check_steps_and_evaluations_equal_the_members_own(gpu):
    """The plan of tests/test_gpu_many.py on seven members; after every step -- with and without a check -- the vectors and
    counters are the controls', and residuals_many with mixed compute_gap flags (both RpEpi classes in one call) gives the eight
    values of residuals() on the controls.  One call gives a member iter = 0: its own path, the same values."""
    models, group, ctrl = two_groups()
    plan = [(1, False), (7, True), (64, False), (149, True), (3, True)]
    it = 0
    for step, (normal, check) in enumerate(plan):
        counts = [normal] * 7
        if step == 1:
            counts[4] = 6
        if step == 2:
            counts[2] = 0
        hprlp.Solver.iterate_many(group, counts, check)
        for c, cnt in zip(ctrl, counts):
            c.iterate(cnt, check)
        assert_same_state(group, ctrl, VECS + (CHECK_VECS if check else ()), step)
        it += normal + (1 if check else 0)
        gaps = [(k + step) % 2 == 1 for k in range(7)]
        iters = [it] * 7
        if step == 3:
            iters[1] = 0      # (the iteration-0 evaluation, bound violation included: the member's own launches)
            gaps[1] = False
        many = hprlp.Solver.residuals_many(group, iters, gaps)
        alone = [c.residuals(i, g) for c, i, g in zip(ctrl, iters, gaps)]
        assert_same_residuals(many, alone, step)
        assert all(np.isfinite(r["kkt"]) for r in many)
        assert_same_state(group, ctrl, ALL_VECS, (step, "after the evaluation"))
    close_all(group + ctrl, models)


def test_restarts_equal_the_members_own(gpu):
    models, group, ctrl = two_groups()
    hprlp.Solver.iterate_many(group, [149] * 7, True)
    for c in ctrl:
        c.iterate(149, True)
    many = hprlp.Solver.residuals_many(group, [150] * 7, [True] * 7)
    alone = [c.residuals(150, True) for c in ctrl]
    assert_same_residuals(many, alone, "before")
    inputs = [(r["weighted_norm"], 2.0 * r["weighted_norm"] + 1.0, c.scalars()["sigma"], r["err_Rd"], r["err_Rp"], r["gap"])
              for r, c in zip(alone, ctrl)]
    sig_many = hprlp.Solver.restart_many(group, inputs)
    sig_alone = [c.restart(*v) for c, v in zip(ctrl, inputs)]
    print("sigmas", sig_many)
    assert sig_many == sig_alone
    assert_same_state(group, ctrl, ALL_VECS, "restart")
    assert all(g.scalars()["kx"] == 0 and g.scalars()["ky"] == 0 for g in group)
    assert all(np.array_equal(g.get("x"), g.get("x_bar")) and np.array_equal(g.get("last_y"), g.get("y_bar")) for g in group)
    hprlp.Solver.iterate_many(group, [0] * 7, True)     # (a restart's check step)
    for c in ctrl:
        c.iterate(0, True)
    assert [g.weighted_norm() for g in group] == [c.weighted_norm() for c in ctrl]
    hprlp.Solver.iterate_many(group, [37] * 7, True)
    for c in ctrl:
        c.iterate(37, True)
    assert_same_state(group, ctrl, ALL_VECS, "after the restart")
    assert_same_residuals(hprlp.Solver.residuals_many(group, [189] * 7, [True] * 7), [c.residuals(189, True) for c in ctrl], "after")
    close_all(group + ctrl, models)


def test_whole_solves_and_the_count_does_not_enter(gpu, five):
    """solve_many of the five LPs equals their own solves (the criterion of tests/test_gpu_many.py), and the same five LPs four
    times each (K = 20: equal members walk equal trajectories) take EQUAL rounds, waits, group launches and scalar copies: the
    count enters none of them.  The only operations issued for one member are the K iteration-0 evaluations."""
    models, singles = five
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-6)
    out = hprlp.solve_many(models, prm)
    c5 = hprlp.last_run_many_counts()
    for k in range(5):
        assert_same_result(out[k], singles[k], k)
    out20 = hprlp.solve_many(models * 4, prm)
    c20 = hprlp.last_run_many_counts()
    print("counts K = 5", c5, "K = 20", c20, "phases", hprlp.last_solve_many_phases())
    for k in range(20):
        assert_same_result(out20[k], singles[k % 5], k)
    for f in ("rounds", "waits", "group_launches", "copies"):
        assert c5[f] == c20[f] and c5[f] > 0, (f, c5, c20)
    assert c5["own"] == 5 and c20["own"] == 20
    assert c20["served"] == 4 * c5["served"] and c5["served"] > c5["rounds"]
    assert c5["waits"] <= 3 * c5["rounds"] and c5["waits"] > c5["rounds"]   # (some round restarted)
    assert c5["copies"] == c5["waits"]
    assert hprlp.last_solve_many_phases()["rounds"] == c20["rounds"]


def test_riders_get_what_they_get_alone(gpu):
    """A member off the small path, a detection member, a started member and two plain ones in one group: everybody's result, and
    the certificate, equal run() alone.  The off-path member's evaluations and check steps are counted as its own."""
    lps = [long_row_lp(), as_lp(EDGE["infeasible"]), planted(SECOND), planted(CLASS_SHAPES[0]), planted(CLASS_SHAPES[2])]
    models = [make(lp) for lp in lps]
    plain = hprlp.Parameters(use_presolve=False, stop_tol=1e-6)
    prms = [plain, hprlp.Parameters(use_presolve=False, stop_tol=1e-8, max_iter=3000), plain, plain, plain]
    group, ctrl = prepared(models, prms), prepared(models, prms)
    assert not (group[0].info()["tiled"] & 4)
    x0 = 0.9 * lps[2]["x_star"]
    for s in (group, ctrl):
        s[1].set_detection()
        s[2].set_start(x0, None)
    out = hprlp.Solver.run_many(group)
    counts = hprlp.last_run_many_counts()
    alone = [c.run() for c in ctrl]
    print("statuses", [r.status for r in out], "iterations", [r.iter for r in out], counts)
    assert [r.status for r in out] == ["OPTIMAL", "PRIMAL_INFEASIBLE", "OPTIMAL", "OPTIMAL", "OPTIMAL"]
    for k in range(5):
        assert_same_result(out[k], alone[k], k)
    kg, kc = group[1].certificate(), ctrl[1].certificate()
    assert kg.kind == kc.kind == 1 and kg.iter == kc.iter == out[1].iter
    assert (kg.objective, kg.violation) == (kc.objective, kc.violation)
    assert np.array_equal(kg.y, kc.y) and np.array_equal(kg.z, kc.z)
    assert group[3].certificate().kind == 0
    # own operations: five iteration-0 evaluations, and an evaluation + a check step of the off-path member per 150 iterations
    assert counts["own"] >= 5 + 2 * (out[0].iter // 150), counts
    assert counts["served"] > 0 and counts["waits"] <= 3 * counts["rounds"]
    close_all(group + ctrl, models)


def test_refusals_leave_the_members_untouched(gpu):
    """The same handle twice, a sharded solver, a solver never scaled: -1 with a message, and the members' vectors are the same
    before and after."""
    lps = [planted(CLASS_SHAPES[0]), planted(SECOND)]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False)
    good = prepared(models)
    hprlp.Solver.iterate_many(good, [5, 5], True)
    before = [{k: s.get(k) for k in ALL_VECS} for s in good]
    local = hprlp.Solver.local_group(1)
    sharded = hprlp.Solver.create_local(models[0], prm, 0, 1, local)
    sharded.scale()
    unscaled = hprlp.Solver(models[1], prm)
    cases = [([good[0], sharded, good[1]], "sharded"), ([good[0], good[1], good[0]], "same solver"), ([good[0], unscaled], "never scaled")]
    for members, word in cases:
        n = len(members)
        with pytest.raises(RuntimeError, match=word) as e:
            hprlp.Solver.residuals_many(members, [5] * n, [True] * n)
        assert "hprlp_solver_residuals_many" in str(e.value)
        with pytest.raises(RuntimeError, match=word) as e:
            hprlp.Solver.restart_many(members, [[1.0, 2.0, 1.0, 1e-3, 1e-3, 1e-3]] * n)
        assert "hprlp_solver_restart_many" in str(e.value)
    with pytest.raises(RuntimeError, match="negative"):
        hprlp.Solver.residuals_many(good, [5, -1], [True, False])
    for s, b in zip(good, before):
        for k in b:
            assert np.array_equal(s.get(k), b[k]), k
    sharded.close()
    unscaled.close()
    hprlp.Solver.free_local_group(local)
    close_all(good, models)
