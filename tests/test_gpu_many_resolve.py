"""Group re-solve of many small LPs on the GPU (hprlp_solver_set_data_many / hprlp_solver_resolve_many; csrc/many.cpp, the
k_*_many kernels of the group re-solve in csrc/kernels.hip; DESIGN.md "Many small LPs", group re-solve).  The group entries change
who issues the launches and how the vectors travel, never the arithmetic or its order: every member must be bit for bit where
set_data() / resolve() leave it alone.  So everything below is == or np.array_equal; nothing has a tolerance.  (Of scalars() the
three wall times are left out: they are clock readings, not results.)"""
import numpy as np
import pytest

import evalcases
from conftest import hprlp, lpgen
from test_gpu_detect import EDGE, as_lp
from test_gpu_many import SIX, assert_same_result, long_row_lp, make, planted, prepared
from test_gpu_many_setup import SCALED, SWITCHES, TIMES, odd_rows_lp
from test_gpu_small import CHECK_VECS, VECS
from test_resolve import base_lp, changed

pytestmark = pytest.mark.gpu

DATA_VECS = ("AL", "AU", "l", "u", "c")
PLAN = [(1, False), (7, True)]
PARTS = ("c", "bounds", "both", "obj", "nothing")
DETECT = 8  # the member with detection on: the tiny infeasible LP
_lps = {}


def eleven_lps():
    """The six class shapes, the odd-rows LP, the LP with every bound kind, the tiny infeasible LP (m, n below one wave and odd:
    the 16-byte pair tail of k_data_bc) and the two network LPs of tests/test_resolve.py."""
    if "all" not in _lps:
        _lps["all"] = [planted(s) for s in SIX] + [odd_rows_lp(), evalcases.case_lp("small", lpgen), as_lp(EDGE["infeasible"]),
                                                    base_lp(11), base_lp(12)]
    return _lps["all"]


def new_data(lp, seed, part):
    """set_data's keyword arguments, by part: c moved by 1e-3 relative, the row sides moved outwards by 1e-3 (1 + |side|) at most
    (infinite sides stay; a feasible LP stays feasible, the infeasible one infeasible), l and u as they are."""
    rng = np.random.default_rng(seed)
    m, n = lp["m"], lp["n"]
    c = np.asarray(lp["c"], float) * (1 + 1e-3 * rng.normal(size=n))
    AL, AU = np.asarray(lp["AL"], float), np.asarray(lp["AU"], float)
    bounds = dict(AL=AL - 1e-3 * rng.uniform(size=m) * (1 + np.abs(AL)), AU=AU + 1e-3 * rng.uniform(size=m) * (1 + np.abs(AU)),
                  l=np.asarray(lp["l"], float), u=np.asarray(lp["u"], float))
    if part == "c":
        return dict(c=c)
    if part == "bounds":
        return bounds
    if part == "both":
        return dict(bounds, c=c)
    if part == "obj":
        return dict(obj_constant=0.5 + seed)
    if part == "nothing":
        return None
    if part == "c1e-3":   # (the changes of tests/test_resolve.py)
        return dict(c=changed(lp, "c1e-3")["c"])
    new = changed(lp, "rows1e-3")
    return dict(AL=new["AL"], AU=new["AU"], l=new["l"], u=new["u"])


def params(switches="default", k=None):
    if k == DETECT:
        return hprlp.Parameters(use_presolve=False, stop_tol=1e-8, max_iter=3000, **SWITCHES[switches])
    # (the perturbed planted LPs converge slowly: the limit keeps every solve short, and equality of bits is the criterion)
    return hprlp.Parameters(use_presolve=False, stop_tol=1e-4, max_iter=5000, **SWITCHES[switches])


def group_and_controls(lps, switches="default", detect=()):
    models = [make(lp) for lp in lps]
    prms = [params(switches, DETECT if k in detect else None) for k in range(len(lps))]
    group, ctrl = prepared(models, prms), prepared(models, prms)
    for k in detect:
        group[k].set_detection()
        ctrl[k].set_detection()
    return models, group, ctrl


def give_data(group, ctrl, data):
    hprlp.Solver.set_data_many(group, data)
    cnt = hprlp.last_resolve_many_counts()
    for c, d in zip(ctrl, data):
        if d:
            c.set_data(**d)
    return cnt


def same_data_state(g, c, what):
    for v in DATA_VECS:
        assert np.array_equal(g.get(v), c.get(v)), (what, v)
    sg, sc = g.scalars(), c.scalars()
    for k in sg:
        if k not in TIMES:
            assert sg[k] == sc[k], (what, k, sg[k], sc[k])


def close(solvers, models=()):
    for s in solvers:
        s.close()
    for m in models:
        m.free()


def eleven_parts():
    """Every part at least twice over the eleven members; the two network LPs get the changes of tests/test_resolve.py."""
    return [PARTS[k % 5] for k in range(9)] + ["c1e-3", "rows1e-3"]


def starts_for(lps, shift=0, cold=()):
    """Per member (x0, y0, sigma), kind (k + shift) % 6: cold, x0 only, y0 only, both, a point outside [l, u] with multipliers of
    the wrong sign on the one-sided rows (the projection), a sigma override; the members of `cold` get no start."""
    rng = np.random.default_rng(23 + shift)
    out = []
    for k, lp in enumerate(lps):
        m, n = lp["m"], lp["n"]
        l, u, AL, AU = (np.asarray(lp[v], float) for v in ("l", "u", "AL", "AU"))
        near = 0.9 * np.asarray(lp["x_star"], float) if "x_star" in lp else rng.uniform(0.0, 1.0, size=n)
        y_any = 0.1 * rng.normal(size=m)
        outside = np.where(np.isfinite(u), u + 1.0, np.where(np.isfinite(l), l - 1.0, 0.0))
        wrong = np.where(np.isinf(AL), 1.0, np.where(np.isinf(AU), -1.0, 0.5))  # y > 0 needs a lower side, y < 0 an upper side
        kind = 0 if k in cold else (k + shift) % 6
        out.append([(None, None, None), (near, None, None), (None, y_any, None), (near, y_any, None), (outside, wrong, None),
                    (None, None, 0.7)][kind])
    return out


def resolve_both(group, ctrl, starts):
    xs, ys, sg = ([s[i] for s in starts] for i in range(3))
    many = hprlp.Solver.resolve_many(group, xs, ys, sg)
    cnt = hprlp.last_resolve_many_counts()
    alone = [c.resolve(x, y, -1.0 if s is None else s) for c, (x, y, s) in zip(ctrl, starts)]
    return many, alone, cnt


@pytest.mark.parametrize("switches", list(SWITCHES))
def test_data_by_bits(gpu, switches):
    """1: a different part per member through set_data_many against set_data alone: the five vectors, the scalars, then the
    first iterations (the bound codes)."""
    lps = eleven_lps()
    models, group, ctrl = group_and_controls(lps, switches)
    assert all(s.info()["tiled"] & 4 for s in group)  # (all on the small path)
    untouched = {k: {v: group[k].get(v) for v in DATA_VECS} for k in range(11)}
    parts = eleven_parts()
    data = [new_data(lp, 100 + k, parts[k]) for k, lp in enumerate(lps)]
    cnt = give_data(group, ctrl, data)
    print(switches, cnt)
    given = sum(1 for p in parts if p not in ("obj", "nothing"))
    assert cnt["members served by group launches"] == given and cnt["members that went their own way"] == 0, cnt
    assert cnt["host waits outside the loop"] == 1 and cnt["memsets"] == 0, cnt
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_data_state(g, c, (switches, k, parts[k]))
        kept = {"c": ("AL", "AU", "l", "u"), "c1e-3": ("AL", "AU", "l", "u"), "bounds": ("c",), "rows1e-3": ("c",), "both": (),
                "obj": DATA_VECS, "nothing": DATA_VECS}[parts[k]]
        for v in kept:   # (the group that was not given keeps its bits)
            assert np.array_equal(g.get(v), untouched[k][v]), (switches, k, v)
        for v in {"c", "AL"} - set(kept):   # (... and what was given has arrived)
            assert not np.array_equal(g.get(v), untouched[k][v]), (switches, k, v)
    for normal, check in PLAN:
        hprlp.Solver.iterate_many(group, [normal] * 11, check)
        for c in ctrl:
            c.iterate(normal, check)
        for k, (g, c) in enumerate(zip(group, ctrl)):
            for v in VECS + (CHECK_VECS if check else ()):
                assert np.array_equal(g.get(v), c.get(v)), (switches, k, v)
    close(group + ctrl, models)


def test_resolve_by_bits_and_history_and_run_many(gpu):
    """2, 3 (first half) and 8 on the eleven members: data, then resolve_many with a different start per member against resolve
    alone; a second round with other data and starts on the same handles against controls that never ran the first; run_many on
    the same group is what it was."""
    lps = eleven_lps()
    models, group, ctrl = group_and_controls(lps, detect=(DETECT,))
    parts = eleven_parts()
    give_data(group, ctrl, [new_data(lp, 100 + k, parts[k]) for k, lp in enumerate(lps)])
    starts = starts_for(lps, cold=(DETECT,))
    many, alone, cnt = resolve_both(group, ctrl, starts)
    print("round 1", cnt, [r.iter for r in many], [r.status for r in many])
    assert cnt["members served by group launches"] == 11 and cnt["members that went their own way"] == 0, cnt
    for k in range(11):
        assert_same_result(many[k], alone[k], k)
    assert many[DETECT].status == "PRIMAL_INFEASIBLE"
    print("statuses", [r.status for r in many])
    assert "OPTIMAL" in [r.status for r in many]   # (each ends as it does alone, whatever that is)
    kg, kc = group[DETECT].certificate(), ctrl[DETECT].certificate()
    assert kg.kind == kc.kind == 1 and kg.iter == kc.iter == many[DETECT].iter
    assert (kg.objective, kg.violation) == (kc.objective, kc.violation)
    assert np.array_equal(kg.y, kc.y) and np.array_equal(kg.z, kc.z)
    # the starts were not ignored: the same members cold (history does not enter, so the controls serve again)
    cold = [c.resolve() for c in ctrl]
    assert any(many[k].iter != cold[k].iter or not np.array_equal(many[k].x, cold[k].x) for k in (1, 2, 3, 4, 7, 9, 10))
    assert many[5].iter != cold[5].iter or not np.array_equal(many[5].x, cold[5].x)  # (the sigma override)
    # 8: run_many after set_data_many is what it always was: every iteration-0 evaluation a member's own (the detection member
    # is left out here: its ray tests are counted as its own operations too)
    rest = [g for k, g in enumerate(group) if k != DETECT]
    for g in rest:
        lam = g.scalars()["lambda_max"]
        g.reset()
        g.init(-1.0, lam)
    again = hprlp.Solver.run_many(rest)
    rm = hprlp.last_run_many_counts()
    print("run_many", rm)
    assert rm["own"] == 10, rm
    for g, c in zip(again, [r for k, r in enumerate(cold) if k != DETECT]):
        assert_same_result(g, c, "run_many")
    # 3: a second round on the same handles: full data, so that a control created now is where the group's member is
    fresh_models, unused, fresh = group_and_controls(lps, detect=(DETECT,))
    close(unused)
    # (obj_constant too: two members were given one in the first round, and it enters the gap)
    data2 = [dict(new_data(lp, 200 + k, "both"), obj_constant=1.5) for k, lp in enumerate(lps)]
    give_data(group, fresh, data2)
    many2, alone2, cnt2 = resolve_both(group, fresh, starts_for(lps, shift=2, cold=(DETECT,)))
    print("round 2", cnt2, [r.iter for r in many2])
    for k in range(11):
        assert_same_result(many2[k], alone2[k], ("round 2", k))
    close(group + ctrl + fresh, models + fresh_models)


def test_history_third_round(gpu):
    """3 (second half): three rounds on four members, each against controls created for that round alone."""
    lps = [planted(SIX[0]), planted(SIX[4]), base_lp(11), odd_rows_lp()]
    models, group, unused = group_and_controls(lps)
    close(unused)
    for rnd in range(3):
        ctrl = prepared(models, [params()] * 4)
        data = [new_data(lp, 300 + 10 * rnd + k, "both") for k, lp in enumerate(lps)]
        give_data(group, ctrl, data)
        many, alone, cnt = resolve_both(group, ctrl, starts_for(lps, shift=1 + rnd))
        for k in range(4):
            assert_same_result(many[k], alone[k], (rnd, k))
        close(ctrl)
    close(group, models)


def test_the_count_does_not_enter(gpu):
    """4: 5 and 20 copies of the 300 x 500 planted LP: the same counts outside the loop, one wait for the data, at most two for
    the re-solve, no memset, every iteration-0 evaluation served by the group; and fewer launches than two members alone."""
    lp = planted(SIX[0])
    model = make(lp)
    seen = {}
    for K in (5, 20):
        group = prepared([model] * K, [params()] * K)
        hprlp.Solver.set_data_many(group, [new_data(lp, 400 + k, "both") for k in range(K)])
        d = hprlp.last_resolve_many_counts()
        out = hprlp.Solver.resolve_many(group, x=[0.9 * lp["x_star"]] * K)
        r = hprlp.last_resolve_many_counts()
        print(K, d, r)
        assert len(out) == K and all(o.iter > 0 for o in out)
        assert d["members served by group launches"] == K and r["members served by group launches"] == K
        seen[K] = (d, r)
        close(group)
    served = "members served by group launches"
    for i in (0, 1):
        assert {k: v for k, v in seen[5][i].items() if k != served} == {k: v for k, v in seen[20][i].items() if k != served}
    d, r = seen[20]
    assert d["host waits outside the loop"] == 1 and d["memsets"] == 0 and d["members that went their own way"] == 0, d
    assert r["host waits outside the loop"] <= 2 and r["memsets"] == 0 and r["members that went their own way"] == 0, r
    assert r["loop operations issued for one member"] == 0, r
    # against a silent fall-back: two members, each alone, take more launches outside the loop than the twenty together
    alone_data = alone_resolve = 0
    for k in range(2):
        one = prepared([model], [params()])
        hprlp.Solver.set_data_many(one, [new_data(lp, 400 + k, "both")])
        c = hprlp.last_resolve_many_counts()
        assert c["members that went their own way"] == 1 and c[served] == 0, c
        alone_data += c["launches outside the loop"]
        hprlp.Solver.resolve_many(one, x=[0.9 * lp["x_star"]])
        c = hprlp.last_resolve_many_counts()
        assert c["members that went their own way"] == 1 and c[served] == 0, c
        alone_resolve += c["launches outside the loop"]
        close(one)
    assert d["launches outside the loop"] < alone_data and r["launches outside the loop"] < alone_resolve, (d, r, alone_data, alone_resolve)
    model.free()


def test_a_group_of_one(gpu):
    """5: the single entries' bits, counted as going its own way."""
    lp = base_lp(12)
    models, group, ctrl = group_and_controls([lp])
    cnt = give_data(group, ctrl, [new_data(lp, 5, "both")])
    assert cnt["members that went their own way"] == 1 and cnt["members served by group launches"] == 0, cnt
    same_data_state(group[0], ctrl[0], "one")
    many, alone, cnt = resolve_both(group, ctrl, [(0.9 * lp["x_star"], None, None)])
    assert cnt["members that went their own way"] == 1 and cnt["members served by group launches"] == 0, cnt
    assert_same_result(many[0], alone[0], "one")
    close(group + ctrl, models)


def test_a_member_off_the_small_path(gpu):
    """6: a 300-entry row among three others: the same bits for all four, one on its own, three served."""
    lps = [planted(SIX[0]), long_row_lp(), planted(SIX[4]), base_lp(11)]
    models, group, ctrl = group_and_controls(lps)
    assert not (group[1].info()["tiled"] & 4)
    lps[1] = dict(lps[1], x_star=np.full(600, 0.5))
    cnt = give_data(group, ctrl, [new_data(lp, 600 + k, "both") for k, lp in enumerate(lps)])
    assert cnt["members that went their own way"] == 1 and cnt["members served by group launches"] == 3, cnt
    for k in range(4):
        same_data_state(group[k], ctrl[k], k)
    many, alone, cnt = resolve_both(group, ctrl, starts_for(lps))
    assert cnt["members that went their own way"] == 1 and cnt["members served by group launches"] == 3, cnt
    for k in range(4):
        assert_same_result(many[k], alone[k], k)
    close(group + ctrl, models)


def test_refusals_leave_the_members_untouched(gpu):
    """7: RuntimeError naming the member; scaled vectors and iterates are the same before and after."""
    lps = [planted(SIX[0]), planted(SIX[4]), base_lp(11)]
    models = [make(lp) for lp in lps]
    prm = params()
    good = prepared(models, [prm] * 3)
    hprlp.Solver.iterate_many(good, [5, 5, 5], True)
    before = [{k: s.get(k) for k in SCALED + VECS + CHECK_VECS} for s in good]
    local = hprlp.Solver.local_group(1)
    sharded = hprlp.Solver.create_local(models[0], prm, 0, 1, local)
    sharded.scale()
    unscaled = hprlp.Solver(models[1], prm)
    full = [new_data(lp, 700 + k, "both") for k, lp in enumerate(lps)]
    half = [full[0], full[1], {k: v for k, v in full[2].items() if k != "AU"}]
    nan_c = [full[0], dict(full[1], c=np.where(np.arange(lps[1]["n"]) == 7, np.nan, full[1]["c"])), full[2]]
    inf_x = np.where(np.arange(lps[2]["n"]) == 3, np.inf, 0.5)

    def both(members, d, word):
        return [(lambda: hprlp.Solver.set_data_many(members, d), word), (lambda: hprlp.Solver.resolve_many(members), word)]

    cases = both([good[0], good[1], good[0]], [full[0], full[1], full[0]], "members 0 and 2 are the same solver")
    cases += both([good[0], unscaled], [full[0], full[1]], "member 1 was never scaled")
    cases += both([good[0], sharded, good[2]], [full[0], full[0], full[2]], "member 1 is a sharded solver")
    cases += [(lambda: hprlp.Solver.set_data_many(good, half), "member 2: AL, AU, l and u are given together"),
              (lambda: hprlp.Solver.set_data_many(good, nan_c), r"member 1: c\[7\] is NaN"),
              (lambda: hprlp.Solver.resolve_many(good, x=[None, None, inf_x]), r"member 2: warm start: x0\[3\] is not finite")]
    for call, word in cases:
        with pytest.raises(RuntimeError, match=word) as e:
            call()
        assert "hprlp_solver_set_data_many" in str(e.value) or "hprlp_solver_resolve_many" in str(e.value), str(e.value)
    for s, b in zip(good, before):
        for k in b:
            assert np.array_equal(s.get(k), b[k]), k
    sharded.close()
    unscaled.close()
    hprlp.Solver.free_local_group(local)
    close(good, models)
