"""Group detection of many small LPs on the GPU (kernels.hip: k_reduce_many<RayFormTask>, k_spmv_fused_many<RayColEpi / RayRowEpi /
PlainEpi<false>>, k_mapped_many<CopyTask>; many.cpp: loop_many, ray_step_many; DESIGN.md "Many small LPs", group detection).  A
workgroup of a group kernel runs the single kernel's body as workgroup lb of its member's own grid, so the criterion is the one of
tests/test_gpu_many_group.py: equality of BITS with the member's own launches.  Every result assertion below is == or
np.array_equal; the values of the ray kernels themselves are held by tests/test_gpu_ray_values.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_detect import EDGE, as_lp, check_certificate
from test_gpu_many import CLASS_SHAPES, SECOND, assert_same_result, close_all, long_row_lp, planted, prepared
from test_gpu_many_group import ALL_VECS, KEYS, TINY, seven_lps
from test_gpu_small import make

pytestmark = pytest.mark.gpu

RAY_VECS = ("ray_d", "ray_y", "ray_prev_x", "ray_prev_y")
VERDICT = {"PRIMAL_INFEASIBLE": 1, "DUAL_INFEASIBLE": 2}


def assert_same_certificate(a, b, what):
    assert (a.kind, a.iter, a.m, a.n) == (b.kind, b.iter, b.m, b.n), (what, a.kind, a.iter, b.kind, b.iter)
    assert (a.objective, a.violation) == (b.objective, b.violation), (what, a.objective, b.objective, a.violation, b.violation)
    for f in ("y", "z", "d"):
        va, vb = getattr(a, f), getattr(b, f)
        assert (va is None) == (vb is None) and (va is None or np.array_equal(va, vb)), (what, f)


# ---- 1: the step level ---------------------------------------------------------------------------------------------------------
def test_ray_steps_equal_the_members_own(gpu):
    """The seven LPs of tests/test_gpu_many_group.py (a grid of 1, grids that are no multiple of 8, different grids in one launch)
    and the two edge cases (2 x 1 and 1 x 2: vectors shorter than one wave).  restart everywhere (nobody tested), a step of all
    nine items, mixed flags (form-only members and full members in the same launches), and the complement of those flags through
    the C entry itself with a sentinel in `out`.  After every step: tested, the nine scalars and the four ray vectors are the
    controls' (hprlp_solver_ray_step), x_bar / y_bar and every other vector are what they were, and the eight residual values are
    the controls'."""
    lps = seven_lps() + [as_lp(EDGE["infeasible"]), as_lp(EDGE["unbounded"])]
    K = len(lps)
    models = [make(lp) for lp in lps]
    group, ctrl = prepared(models, scale_only=True), prepared(models, scale_only=True)
    for g, c in zip(group, ctrl):
        lam, _ = c.power_iteration()
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    assert all(s.info()["tiled"] & 4 for s in group)   # (everybody on the small path: everybody joins)
    it = 0

    def advance(normal):
        nonlocal it
        hprlp.Solver.iterate_many(group, [normal] * K, True)
        for c in ctrl:
            c.iterate(normal, True)
        it += normal + 1

    def compare(many, flags, what):
        alone = [c.ray_step(bool(f)) for c, f in zip(ctrl, flags)]
        for k, (a, b) in enumerate(zip(many, alone)):
            assert (a is None) == (b is None), (what, k)
            assert a == b, (what, k, a, b)
        for k, (g, c) in enumerate(zip(group, ctrl)):
            for v in RAY_VECS + ALL_VECS:
                assert np.array_equal(g.get(v), c.get(v)), (what, k, v)
        res_many = hprlp.Solver.residuals_many(group, [it] * K, [True] * K)
        res_alone = [c.residuals(it, True) for c in ctrl]
        for k, (a, b) in enumerate(zip(res_many, res_alone)):
            for f in KEYS:
                assert a[f] == b[f], (what, k, f)
        return alone

    def step(flags, what):
        before = [{v: g.get(v) for v in ALL_VECS} for g in group]
        many = hprlp.Solver.ray_step_many(group, flags)
        for g, b in zip(group, before):
            for v in b:
                assert np.array_equal(g.get(v), b[v]), (what, v)
        return compare(many, flags, what)

    advance(37)
    first = step([1] * K, "restart everywhere")
    assert first == [None] * K
    advance(37)
    second = step([0] * K, "all nine items")
    assert all(r is not None for r in second)
    assert all(np.isfinite(list(r.values())).all() for r in second)
    assert any(r["D"] != 0.0 or r["cd"] != 0.0 for r in second)
    advance(23)
    mixed = [k % 2 for k in range(K)]
    third = step(mixed, "mixed flags")
    assert [r is None for r in third] == [bool(f) for f in mixed]
    advance(23)
    # the complement through the C entry: out + 9 k stays untouched where tested[k] is 0
    flags = np.array([1 - f for f in mixed], np.int32)
    out, tested = np.full(9 * K, -7.5), np.full(K, -1, np.int32)
    hs = (C.c_void_p * K)(*[g.h for g in group])
    rc = hprlp.lib().hprlp_solver_ray_step_many(hs, K, flags.ctypes.data_as(hprlp.c_int_p), out.ctypes.data_as(hprlp.c_dbl_p),
                                                tested.ctypes.data_as(hprlp.c_int_p))
    assert rc == 0, hprlp.last_error()
    assert list(tested) == [0 if f else 1 for f in flags]
    many = []
    for k in range(K):
        if not tested[k]:
            assert np.array_equal(out[9 * k:9 * k + 9], np.full(9, -7.5)), k
            many.append(None)
            continue
        r = dict(zip(hprlp.Solver.RAY_SLOTS, (float(v) for v in out[9 * k:9 * k + 9])))
        r.update(D=r["DY"] + r["DZ"], V=max(r["VY"], r["VZ"]), cd=r["CD"], W=max(r["WD"], r["WQ"]), yn=r["YN"], dn=r["DN"])
        many.append(r)
    compare(many, list(flags), "the complement")
    close_all(group + ctrl, models)


# ---- 2, 3: whole solves ----------------------------------------------------------------------------------------------------------
# (the parameters under which tests/test_gpu_detect.py takes the two planted LPs to their verdicts on the small path; on an MI355X
# the seven end at iterations 4050, 2100, 300, 450 with their verdicts and at 2250, 700, 1900 OPTIMAL)
PRM = dict(use_presolve=False, stop_tol=1e-4, max_iter=50000, use_CR_scaling=False)


def seven_with_verdicts():
    """The two planted LPs that tests/test_gpu_detect.py takes to their verdicts on the small path, the two edge cases and three
    feasible planted LPs."""
    return [lpgen.planted_infeasible_lp(400, 600, 2400, 21), lpgen.planted_unbounded_lp(400, 600, 2400, 21), as_lp(EDGE["infeasible"]),
            as_lp(EDGE["unbounded"]), planted(CLASS_SHAPES[0]), planted(SECOND), lpgen.planted_lp(*TINY)]


WANT = ["PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL", "OPTIMAL", "OPTIMAL"]


@pytest.fixture(scope="module")
def seven():
    """Models, each member's run() alone with detection on (result and certificate; computed once, never changed), and the group
    solve of the seven with its counts."""
    lps = seven_with_verdicts()
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(**PRM)
    alone = []
    for m in models:
        s = hprlp.Solver(m, prm)
        s.set_detection()
        s.prepare()
        r = s.run(max_trace=1)
        alone.append((r, s.certificate()))
        s.close()
    results, certs = hprlp.solve_many_detect(models, prm)
    counts = hprlp.last_run_many_detect_counts()
    yield lps, models, alone, results, certs, counts
    for m in models:
        m.free()


def test_solve_many_detect_equals_each_members_own_run(gpu, seven):
    lps, models, alone, results, certs, counts = seven
    print("verdict iterations", [(r.status, r.iter) for r in results], counts)
    assert [r.status for r in results] == WANT
    for k in range(7):
        assert_same_result(results[k], alone[k][0], k)
        assert_same_certificate(certs[k], alone[k][1], k)
        if WANT[k] != "OPTIMAL":
            check_certificate(lps[k], results[k], WANT[k])
        else:
            assert certs[k].kind == 0 and (certs[k].m, certs[k].n) == (lps[k]["m"], lps[k]["n"])
    assert counts["certs_served"] == 4 and counts["ray_served"] > 0


def test_the_count_does_not_enter(gpu, seven):
    """The same seven once and four times over: equal members walk equal trajectories, so rounds, waits, group launches and copies
    are EQUAL; the only operations issued for one member are the K iteration-0 evaluations; the served ray tests and certificates
    scale by four; a round with verdicts costs one wait more, whatever the number of verdicts in it."""
    lps, models, alone, results, certs, c7 = seven
    out28, certs28 = hprlp.solve_many_detect(models * 4, hprlp.Parameters(**PRM))
    c28 = hprlp.last_run_many_detect_counts()
    print("counts K = 7", c7, "K = 28", c28)
    for k in range(28):
        assert_same_result(out28[k], alone[k % 7][0], k)
        assert_same_certificate(certs28[k], alone[k % 7][1], k)
    for f in ("rounds", "waits", "group_launches", "copies"):
        assert c7[f] == c28[f] and c7[f] > 0, (f, c7, c28)
    assert c7["own"] == 7 and c28["own"] == 28, (c7, c28)
    assert c28["ray_served"] == 4 * c7["ray_served"] and c7["ray_served"] > 0
    assert c28["certs_served"] == 4 * c7["certs_served"] == 16
    assert c28["served"] == 4 * c7["served"]
    verdict_rounds = len({r.iter for r in results if r.status in VERDICT})   # (one loop, one check_iter: a round is an iteration)
    assert c7["waits"] <= 3 * c7["rounds"] + verdict_rounds, (c7, verdict_rounds)
    assert c7["copies"] == c7["waits"]


# ---- 4: riders -----------------------------------------------------------------------------------------------------------------
def test_riders_get_what_they_get_alone(gpu):
    """One group: a member off the small path with detection on (its ray tests stay its own), a lone detection member among the
    members of the group launches (every ray kind holds one task: the member's own launches by the own-launch rule), a started
    member and two plain ones with detection off (no ray task).  Everybody equals run() alone."""
    lps = [long_row_lp(), as_lp(EDGE["infeasible"]), planted(SECOND), planted(CLASS_SHAPES[0]), planted(CLASS_SHAPES[2])]
    models = [make(lp) for lp in lps]
    plain = hprlp.Parameters(use_presolve=False, stop_tol=1e-4)   # (1e-4: the off-path member issues every launch itself)
    prms = [plain, hprlp.Parameters(use_presolve=False, stop_tol=1e-8, max_iter=3000), plain, plain, plain]
    group, ctrl = prepared(models, prms), prepared(models, prms)
    assert not (group[0].info()["tiled"] & 4)
    x0 = 0.9 * lps[2]["x_star"]
    for s in (group, ctrl):
        s[0].set_detection()
        s[1].set_detection()
        s[2].set_start(x0, None)
    out = hprlp.Solver.run_many(group)
    counts = hprlp.last_run_many_detect_counts()
    alone = [c.run() for c in ctrl]
    print("statuses", [r.status for r in out], "iterations", [r.iter for r in out], counts)
    assert [r.status for r in out] == ["OPTIMAL", "PRIMAL_INFEASIBLE", "OPTIMAL", "OPTIMAL", "OPTIMAL"]
    for k in range(5):
        assert_same_result(out[k], alone[k], k)
        assert_same_certificate(group[k].certificate(), ctrl[k].certificate(), k)
    assert group[1].certificate().kind == 1 and group[0].certificate().kind == 0
    # the lone member's periodic evaluations behind iteration 0, and its one certificate, went through the group's recorder
    assert counts["ray_served"] == out[1].iter // 150 and counts["certs_served"] == 1, counts
    assert counts["own"] >= 5 + 2 * (out[0].iter // 150), counts
    close_all(group + ctrl, models)


# ---- 5, 6: detection that finds nothing, detection off -------------------------------------------------------------------------
def test_detection_on_feasible_members_changes_nothing(gpu):
    lps = [planted(CLASS_SHAPES[0]), planted(SECOND), lpgen.planted_lp(*TINY)]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-6, max_iter=20000)
    on, certs = hprlp.solve_many_detect(models, prm)
    c_on = hprlp.last_run_many_detect_counts()
    off = hprlp.solve_many(models, prm)
    c_off = hprlp.last_run_many_detect_counts()
    print("statuses", [(r.status, r.iter) for r in on], c_on, c_off)
    assert all(r.status in ("OPTIMAL", "ITER_LIMIT") for r in on)
    for k in range(3):
        assert_same_result(on[k], off[k], k)
        assert certs[k].kind == 0 and certs[k].y is None and certs[k].d is None
    assert c_on["ray_served"] > 0 and c_on["certs_served"] == 0 and c_off["ray_served"] == 0
    for f in ("rounds", "waits", "copies", "own", "served"):   # (detection adds launches to a periodic round, and nothing else)
        assert c_on[f] == c_off[f], (f, c_on, c_off)
    for m in models:
        m.free()


def test_no_detection_through_the_new_entry_is_solve_many(gpu):
    lps = [as_lp(EDGE["infeasible"]), planted(CLASS_SHAPES[0])]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-8, max_iter=1200)
    a, certs = hprlp.solve_many_detect(models, prm, eps_primal=None, eps_dual=None)
    c_a = hprlp.last_run_many_detect_counts()
    b = hprlp.solve_many(models, prm)
    c_b = hprlp.last_run_many_detect_counts()
    assert a[0].status == b[0].status == "ITER_LIMIT" and a[0].iter == 1200
    for k in range(2):
        assert_same_result(a[k], b[k], k)
        assert certs[k].kind == 0 and (certs[k].m, certs[k].n) == (lps[k]["m"], lps[k]["n"])
    assert c_a == c_b and c_a["ray_served"] == 0
    for m in models:
        m.free()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_members_untouched(gpu):
    """A sharded member, the same handle twice, a solver never scaled, a first step without restart: -1 with a message that names
    the entry (and the member), and every member's vectors are what they were."""
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
        with pytest.raises(RuntimeError, match=word) as e:
            hprlp.Solver.ray_step_many(members, [1] * len(members))
        assert "hprlp_solver_ray_step_many" in str(e.value)
    for flags, k in (([0, 0], 0), ([1, 0], 1)):
        with pytest.raises(RuntimeError, match="needs restart") as e:
            hprlp.Solver.ray_step_many(good, flags)
        assert "hprlp_solver_ray_step_many" in str(e.value) and f"member {k}" in str(e.value)
    for s in good:   # (nobody's ray vectors were begun by a refused call)
        with pytest.raises(RuntimeError):
            s.get("ray_d")
    for s, b in zip(good, before):
        for k in b:
            assert np.array_equal(s.get(k), b[k]), k
    assert hprlp.Solver.ray_step_many(good, [1, 1]) == [None, None]   # (and the members still work)
    sharded.close()
    unscaled.close()
    hprlp.Solver.free_local_group(local)
    close_all(good, models)
