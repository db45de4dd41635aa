"""Group matrix values of many small LPs on the GPU (hprlp_solver_set_matrix_values_many; csrc/many.cpp: set_matrix_values_many and
scale_walk, the three kinds ValuesCheckTask / ValuesInTask / VectorsInTask of csrc/kernels.hip on the bodies of csrc/values_body.h;
DESIGN.md "Many small LPs", group matrix values).  The group entry changes who issues the launches and how the values travel, never
the arithmetic or its order: every member must be bit for bit where its own hprlp_solver_set_matrix_values leaves it, which is a
fresh solver on the changed model after scale().  So every assertion on results below is == or np.array_equal; nothing has a
tolerance.  (Of scalars() the three wall times are left out: they are clock readings, not results.)

A member with a locality ordering runs at the suite's large reordered shape (1.6 M rows, the default thresholds; a single solver's
ordering at a small shape under HPRLP_REORDER_ANYWAY is tests/test_gpu_reorder_small.py, the group's reordered member is not forced there); it
has a test of its own (about two seconds on an MI355X)."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from conftest import hprlp
from test_gpu_many import SIX, assert_same_result, long_row_lp, make, planted, prepared
from test_gpu_many_resolve import close, eleven_lps, new_data, params
from test_gpu_many_setup import SCALED, SWITCHES, TIMES, odd_rows_lp, same_first_iterations
from test_gpu_small import CHECK_VECS, VECS
from test_resolve import base_lp

pytestmark = pytest.mark.gpu

ITERATES = VECS + CHECK_VECS
SERVED, OWN, MAPS = "members served by group launches", "members that went their own way", "members whose value maps were built"
_lps = {}


def pattern_lp(A, seed):
    """A feasible LP on the pattern and values of A: row sides one around A x0, 0 <= x <= 2."""
    A = sparse.csr_matrix(A)
    A.sort_indices()
    m, n = A.shape
    rng = np.random.default_rng(seed)
    b = A @ rng.uniform(0.0, 1.0, size=n)
    return dict(m=m, n=n, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.astype(float), AL=b - 1.0,
                AU=b + 1.0, l=np.zeros(n), u=np.full(n, 2.0), c=rng.normal(size=n))


def random_pattern(m, n, nnz, seed):
    rng = np.random.default_rng(seed)
    flat = rng.choice(m * n, size=nnz, replace=False)
    v = rng.normal(size=nnz) * 0.3 + np.sign(rng.normal(size=nnz))
    return sparse.csr_matrix((v, (flat // n, flat % n)), shape=(m, n))


def four_lps():
    """Odd nnz (301: the scatter's last lane stores one entry alone) and even nnz (300: every lane a 16-byte pair), more than one
    workgroup of pairs neither way; nnz == 1 (no pair at all); 5 x 6 with an empty row, an empty column and a row of one entry."""
    if "four" not in _lps:
        rows = [0, 0, 0, 1, 3, 3, 3, 4, 4]
        cols = [0, 1, 4, 5, 0, 2, 4, 1, 5]
        holes = sparse.csr_matrix((np.array([1.5, -2.0, 0.5, 3.0, -1.0, 2.5, 1.0, -0.75, 2.0]), (rows, cols)), shape=(5, 6))
        one = sparse.csr_matrix((np.array([2.0]), ([1], [2])), shape=(3, 4))
        _lps["four"] = [pattern_lp(random_pattern(40, 70, 301, 41), 42), pattern_lp(random_pattern(70, 40, 300, 43), 44), pattern_lp(one, 45),
                        pattern_lp(holes, 46)]
        assert [len(lp["values"]) for lp in _lps["four"]] == [301, 300, 1, 9]
    return _lps["four"]


def fifteen_lps():
    return eleven_lps() + four_lps()


def new_values(lp, seed):
    """set_matrix's keyword arguments: val * (1 + 1e-3 normal) with a few stored zeros -- three anywhere from 20 entries on, and
    the entry of the first row that has one entry only (the 1 x 1 matrix apart) --, all five vectors moved as new_data(.., "both")."""
    rng = np.random.default_rng(1000 + seed)
    val = np.asarray(lp["values"], float)
    nnz = len(val)
    v = val * (1 + 1e-3 * rng.normal(size=nnz))
    if nnz >= 20:
        v[rng.choice(nnz, size=3, replace=False)] = 0.0
    lone = np.flatnonzero(np.diff(np.asarray(lp["rowptr"])) == 1)
    if nnz > 1 and len(lone):
        v[lp["rowptr"][lone[0]]] = 0.0
    return dict(new_data(lp, seed, "both"), values=v)


def changed_lp(lp, d):
    return dict(lp, values=d["values"], AL=d["AL"], AU=d["AU"], l=d["l"], u=d["u"], c=d["c"])


def set_alone(s, d):
    """hprlp_solver_set_matrix_values itself (Solver.set_matrix goes on to the power iteration)."""
    a = {k: np.ascontiguousarray(d[k], dtype=np.float64) for k in ("values", "c", "AL", "AU", "l", "u")}
    p = lambda k: a[k].ctypes.data_as(hprlp.c_dbl_p)
    oc = None if d.get("obj_constant") is None else C.byref(C.c_double(float(d["obj_constant"])))
    rc = hprlp.lib().hprlp_solver_set_matrix_values(s.h, p("values"), len(a["values"]), p("c"), oc, p("AL"), p("AU"), p("l"), p("u"))
    assert rc == 0, hprlp.last_error()


def state(s):
    d = {k: s.get(k) for k in SCALED + ITERATES}
    d["scalars"] = {k: v for k, v in s.scalars().items() if k not in TIMES}
    d["info"], d["describe"] = s.info(), s.describe()
    return d


def assert_same_state(a, b, what):
    for k in SCALED + ITERATES:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in a["scalars"]:
        assert a["scalars"][k] == b["scalars"][k], (what, k, a["scalars"][k], b["scalars"][k])
    assert a["info"] == b["info"] and a["describe"] == b["describe"], (what, a["info"], b["info"], a["describe"], b["describe"])


def give(group, ctrl, data):
    hprlp.Solver.set_matrix_many(group, data)
    cnt = hprlp.last_values_many_counts()
    for c, d in zip(ctrl, data):
        if d is not None:
            set_alone(c, d)
    return cnt


def same_after_the_call(group, ctrl, what):
    for k, (g, c) in enumerate(zip(group, ctrl)):
        sg = state(g)
        assert_same_state(sg, state(c), (what, k))
        for v in ITERATES:
            assert not sg[v].any(), (what, k, v)   # (every state vector is zero)
        assert g.transfer() == c.transfer(), (what, k, g.transfer(), c.transfer())


def solve_both(group, ctrl, what):
    """power_iteration_many + init + resolve_many against each control's own power iteration, init and resolve."""
    many = hprlp.Solver.power_iteration_many(group)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        lam, it = c.power_iteration()
        assert many[k] == (lam, it), (what, k, many[k], lam, it)
        g.init(-1.0, 1.01 * lam)
        c.init(-1.0, 1.01 * lam)
    got = hprlp.Solver.resolve_many(group)
    for k, (r, c) in enumerate(zip(got, ctrl)):
        assert_same_result(r, c.resolve(), (what, k))
    return got


def test_bits_against_the_members_own_call(gpu):
    """1: fifteen members; the first call (the maps are built in it), the solve, a second call with other values, the solve, then
    the single entry and the group entry alternating on the same handles."""
    lps = fifteen_lps()
    K = len(lps)
    models = [make(lp) for lp in lps]
    prms = [params()] * K
    group, ctrl = prepared(models, prms), prepared(models, prms)
    small = [bool(s.info()["tiled"] & 4) for s in group]
    print("on the small path", small)
    assert all(small)
    maps_before = [c.value_maps() for c in ctrl]   # (hprlp_solver_value_maps builds them on demand: the controls' are the reference)
    data = [new_values(lp, 10 + k) for k, lp in enumerate(lps)]
    lone_zero = [k for k, (lp, d) in enumerate(zip(lps, data))
                 if any(np.diff(lp["rowptr"])[i] == 1 and d["values"][lp["rowptr"][i]] == 0.0 for i in range(lp["m"]))]
    assert 14 in lone_zero, lone_zero   # (the 5 x 6 LP: a stored zero that is its row's only entry)
    old = [g.get("A_val") for g in group]
    cnt = give(group, ctrl, data)
    print("first call", cnt)
    assert cnt[SERVED] == K and cnt[OWN] == 0 and cnt[MAPS] == K, cnt
    same_after_the_call(group, ctrl, "first")
    for k, (g, c) in enumerate(zip(group, ctrl)):
        a, t = g.value_maps()
        assert np.array_equal(a, maps_before[k][0]) and np.array_equal(t, maps_before[k][1]), k
        assert not np.array_equal(g.get("A_val"), old[k]) or len(lps[k]["values"]) == 1, k   # (the values have arrived)
    got = solve_both(group, ctrl, "first")
    print("statuses", [r.status for r in got], [r.iter for r in got])
    assert all(r.iter > 0 for r in got)
    data2 = [new_values(lp, 50 + k) for k, lp in enumerate(lps)]
    cnt = give(group, ctrl, data2)
    print("second call", cnt)
    assert cnt[SERVED] == K and cnt[OWN] == 0 and cnt[MAPS] == 0, cnt
    same_after_the_call(group, ctrl, "second")
    solve_both(group, ctrl, "second")
    # the two entries on one handle, in turn: single, group, single, group -- the controls take the single one every time
    for rnd in range(2):
        d1 = [new_values(lp, 100 + 20 * rnd + k) for k, lp in enumerate(lps)]
        for g, c, d in zip(group, ctrl, d1):
            set_alone(g, d)
            set_alone(c, d)
        give(group, ctrl, [new_values(lp, 110 + 20 * rnd + k) for k, lp in enumerate(lps)])
        same_after_the_call(group, ctrl, ("alternating", rnd))
    close(group + ctrl, models)


def test_bits_against_fresh_solvers(gpu):
    """2: the header's claim, without the single entry: create_many + scale_many on the base models, set_matrix_many, against
    create_many + scale_many on the changed models; then the power iteration, init and the solve on both sides."""
    lps = fifteen_lps()
    K = len(lps)
    data = [new_values(lp, 300 + k) for k, lp in enumerate(lps)]
    models = [make(lp) for lp in lps]
    fresh_models = [make(changed_lp(lp, d)) for lp, d in zip(lps, data)]
    prm = params()
    group = hprlp.Solver.create_many(models, prm)
    hprlp.Solver.scale_many(group)
    hprlp.Solver.set_matrix_many(group, data)
    cnt = hprlp.last_values_many_counts()
    print(cnt)
    assert cnt[SERVED] == K and cnt[OWN] == 0, cnt
    fresh = hprlp.Solver.create_many(fresh_models, prm)
    hprlp.Solver.scale_many(fresh)
    for k, (g, f) in enumerate(zip(group, fresh)):
        assert_same_state(state(g), state(f), ("fresh", k))
    lam_g, lam_f = hprlp.Solver.power_iteration_many(group), hprlp.Solver.power_iteration_many(fresh)
    assert lam_g == lam_f, (lam_g, lam_f)
    for g, f, (lam, _) in zip(group, fresh, lam_g):
        g.init(-1.0, 1.01 * lam)
        f.init(-1.0, 1.01 * lam)
    rg, rf = hprlp.Solver.resolve_many(group), hprlp.Solver.resolve_many(fresh)
    for k in range(K):
        assert_same_result(rg[k], rf[k], ("fresh", k))
    close(group + fresh, models + fresh_models)


@pytest.mark.parametrize("switches", list(SWITCHES))
def test_every_switch_set(gpu, switches):
    """3: five members under one switch set (Curtis-Reid, Ruiz, Pock-Chambolle, b / c scaling off in turn: the stages a member
    skips), then the first iterations."""
    lps = [planted(SIX[0]), odd_rows_lp()] + four_lps()[:2] + [base_lp(11)]
    models = [make(lp) for lp in lps]
    prms = [params(switches)] * 5
    group, ctrl = prepared(models, prms), prepared(models, prms)
    cnt = give(group, ctrl, [new_values(lp, 400 + k) for k, lp in enumerate(lps)])
    print(switches, cnt)
    assert cnt[SERVED] == 5 and cnt[OWN] == 0, cnt
    same_after_the_call(group, ctrl, switches)
    same_first_iterations(group, ctrl, switches)
    close(group + ctrl, models)


def test_members_with_different_switches_in_one_call(gpu):
    """3, mixed: six members, one switch set each, in one call."""
    lps = [planted(SIX[0]), odd_rows_lp()] + four_lps()[:2] + [base_lp(11), four_lps()[3]]
    models = [make(lp) for lp in lps]
    prms = [params(name) for name in SWITCHES]
    group, ctrl = prepared(models, prms), prepared(models, prms)
    cnt = give(group, ctrl, [new_values(lp, 450 + k) for k, lp in enumerate(lps)])
    assert cnt[SERVED] == 6 and cnt[OWN] == 0, cnt
    same_after_the_call(group, ctrl, "mixed")
    same_first_iterations(group, ctrl, "mixed")
    close(group + ctrl, models)


def test_who_joins(gpu):
    """4: a member off the small path goes its own way inside the same call and ends on its own bits; a group of one issues the
    member's own launches; a skipped member keeps every bit, the iterates of an earlier solve included."""
    lps = [planted(SIX[0]), long_row_lp(), planted(SIX[4])]
    models = [make(lp) for lp in lps]
    prms = [params()] * 3
    group, ctrl = prepared(models, prms), prepared(models, prms)
    assert not (group[1].info()["tiled"] & 4)
    cnt = give(group, ctrl, [new_values(lp, 500 + k) for k, lp in enumerate(lps)])
    print("two and one", cnt)
    assert cnt[SERVED] == 2 and cnt[OWN] == 1, cnt
    same_after_the_call(group, ctrl, "two and one")
    solve_both(group, ctrl, "two and one")
    # a group of one: the member's own call, counted as going its own way; then the same through a list of one joining member
    for k in (1, 0):
        d = new_values(lps[k], 520 + k)
        cnt = give([group[k]], [ctrl[k]], [d])
        print("one", k, cnt)
        assert cnt[SERVED] == 0 and cnt[OWN] == 1, cnt
        same_after_the_call([group[k]], [ctrl[k]], ("one", k))
    # two members that cannot join (one of them twice would be refused: a second long-row solver)
    extra_g, extra_c = prepared([models[1]], prms[:1])[0], prepared([models[1]], prms[:1])[0]
    d = [new_values(lps[1], 530), new_values(lps[1], 531)]
    cnt = give([group[1], extra_g], [ctrl[1], extra_c], d)
    assert cnt[SERVED] == 0 and cnt[OWN] == 2, cnt
    same_after_the_call([group[1], extra_g], [ctrl[1], extra_c], "nobody joins")
    # a skipped member: members 0 and 2 get values, member 1 of this list (planted(SIX[4])) none; it has solved before
    trio, trio_c = [group[0], group[2], extra_g], [ctrl[0], ctrl[2], extra_c]
    solve_both([group[2]], [ctrl[2]], "before the skip")
    kept = state(group[2])
    assert any(kept[v].any() for v in VECS)   # (non-zero iterates left by the solve)
    cnt = give(trio, trio_c, [new_values(lps[0], 540), None, new_values(lps[1], 541)])
    print("skip", cnt)
    assert cnt[SERVED] == 0 and cnt[OWN] == 2, cnt   # (one joining member alone is no group)
    assert_same_state(state(group[2]), kept, "skipped")
    same_after_the_call([group[0], extra_g], [ctrl[0], extra_c], "beside the skipped one")
    quad = hprlp.Solver(models[0], prms[0])
    quad.prepare()
    quad_c = hprlp.Solver(models[0], prms[0])
    quad_c.prepare()
    cnt = give([group[0], group[2], quad], [ctrl[0], ctrl[2], quad_c], [new_values(lps[0], 550), None, new_values(lps[0], 551)])
    assert cnt[SERVED] == 2 and cnt[OWN] == 0, cnt
    assert_same_state(state(group[2]), kept, "skipped between two served")
    same_after_the_call([group[0], quad], [ctrl[0], quad_c], "served around the skipped one")
    close(group + ctrl + [extra_g, extra_c, quad, quad_c], models)


def test_a_member_with_a_locality_ordering_goes_its_own_way(gpu):
    """4, the ordered member, at the default thresholds (the group's reordered member is not run under HPRLP_REORDER_ANYWAY, the
    hook of tests/test_gpu_reorder_small.py): the one shape the suite's other large reordered cases use (a randomly permuted banded 1 600 000 x 1 600 000 matrix, 10 per row; tests/test_gpu_matrix_values.py), between two
    small members that join.  Its values travel in the group's block and pass the group's check, then it runs its own call."""
    from conftest import lpgen
    m = n = 1_600_000
    rp, ci, v = lpgen.banded_csr(m, n, 10, 16000, 5)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))
    A.sum_duplicates()
    rng = np.random.default_rng(8)
    pr, pc = rng.permutation(m), rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[pc] = np.arange(n)
    B = A[pr]
    B = sparse.csr_matrix((B.data, inv[B.indices], B.indptr), shape=(m, n))
    B.sort_indices()
    big = lpgen._plant(np.random.default_rng(32), B)
    big.update(m=m, n=n, rowptr=B.indptr.astype(np.int32), colind=B.indices.astype(np.int32), values=B.data.copy())
    lps = [planted(SIX[0]), big, planted(SIX[4])]
    models = [make(lp) for lp in lps]
    prms = [params()] * 3
    group, ctrl = prepared(models, prms, scale_only=True), prepared(models[1:2], prms[1:2], scale_only=True)
    assert group[1].info()["reordered"] and ctrl[0].info()["reordered"]
    data = [new_values(lp, 560 + k) for k, lp in enumerate(lps)]
    hprlp.Solver.set_matrix_many(group, data)
    cnt = hprlp.last_values_many_counts()
    print("ordered member", cnt)
    assert cnt[SERVED] == 2 and cnt[OWN] == 1, cnt
    set_alone(ctrl[0], data[1])
    for k in SCALED:
        assert np.array_equal(group[1].get(k), ctrl[0].get(k)), k
    sg, sc = group[1].scalars(), ctrl[0].scalars()
    assert all(sg[k] == sc[k] for k in sg if k not in TIMES), (sg, sc)
    assert group[1].info() == ctrl[0].info() and group[1].describe() == ctrl[0].describe()
    bad = dict(data[1], values=np.where(np.arange(len(data[1]["values"])) == 12_000_001, np.inf, data[1]["values"]))
    kept = {k: group[0].get(k) for k in SCALED}
    with pytest.raises(RuntimeError, match=r"member 1: val\[12000001\] is not finite"):
        hprlp.Solver.set_matrix_many(group, [new_values(lps[0], 570), bad, new_values(lps[2], 572)])
    for k in SCALED:   # (the ordered member and a joining one, after the refusal)
        assert np.array_equal(group[1].get(k), ctrl[0].get(k)), k
        assert np.array_equal(group[0].get(k), kept[k]), k
    close(group + ctrl, models)


def test_refusals_leave_everybody_alone(gpu):
    """5: five members with iterates of a few steps; every refused call returns -1 with the member in the message and leaves all
    five bit for bit; the clean call afterwards gives the bits of test 1."""
    lps = [planted(SIX[0]), planted(SIX[4]), base_lp(11), four_lps()[0], odd_rows_lp()]
    models = [make(lp) for lp in lps]
    prms = [params()] * 5
    group, ctrl = prepared(models, prms), prepared(models, prms)
    hprlp.Solver.iterate_many(group, [5] * 5, True)
    for c in ctrl:
        c.iterate(5, True)
    before = [state(s) for s in group]
    assert all(any(b[v].any() for v in VECS) for b in before)
    clean = [new_values(lp, 600 + k) for k, lp in enumerate(lps)]

    def bad_values(d, inf_at=7, nan_at=2):
        v = d["values"].copy()
        v[inf_at], v[nan_at] = np.inf, np.nan
        return dict(d, values=v)

    def with_member(k, d):
        return [d if i == k else clean[i] for i in range(5)]

    nan_AU = dict(clean[2], AU=np.where(np.arange(lps[2]["m"]) == 4, np.nan, clean[2]["AU"]))
    unscaled = hprlp.Solver(models[1], prms[1])
    n0 = len(lps[0]["values"])
    cases = [(group, with_member(3, bad_values(clean[3])), r"member 3: val\[2\] is not finite"),
             (group, [clean[0], bad_values(clean[1], 11, 30), clean[2], bad_values(clean[3]), clean[4]], r"member 1: val\[11\] is not finite"),
             (group, with_member(2, nan_AU), r"member 2: AU\[4\] is NaN"),
             (group, with_member(0, dict(clean[0], values=clean[0]["values"][:-1])), "member 0: nnz is %d, the model has %d" % (n0 - 1, n0)),
             (group, with_member(4, {k: v for k, v in clean[4].items() if k != "c"}), "member 4: val, c, AL, AU, l and u are all required"),
             (group, with_member(4, dict(obj_constant=1.0)), "member 4: val, c, AL, AU, l and u are all required"),
             ([group[0], group[1], group[0]], [clean[0], clean[1], clean[0]], "members 0 and 2 are the same solver"),
             ([group[0], unscaled, group[2]], [clean[0], clean[1], clean[2]], "member 1 was never scaled")]
    for members, data, word in cases:
        with pytest.raises(RuntimeError, match=word) as e:
            hprlp.Solver.set_matrix_many(members, data)
        assert "hprlp_solver_set_matrix_values_many" in str(e.value), str(e.value)
        for k, (s, b) in enumerate(zip(group, before)):
            assert_same_state(state(s), b, (word, k))
    unscaled.close()
    cnt = give(group, ctrl, clean)
    assert cnt[SERVED] == 5 and cnt[OWN] == 0, cnt
    same_after_the_call(group, ctrl, "clean after the refusals")
    solve_both(group, ctrl, "clean after the refusals")
    close(group + ctrl, models)


def test_the_count_does_not_enter(gpu):
    """6: 5 and 20 copies of the 300 x 500 planted LP, default switches, second call (the maps are there): every slot but the
    served members is the same.  Host waits: the check's one and the scaling's (what scale_many reports for the same group).
    Memsets: the flag words'.  Host-to-device copies: the staging block, the table of the check's run, and one table copy per
    run of the scaling walk -- the walk runs what it has recorded in front of each of its waits, so that is its wait count."""
    lp = planted(SIX[0])
    model = make(lp)
    seen = {}
    for K in (5, 20):
        group = hprlp.Solver.create_many([model] * K, params())
        hprlp.Solver.scale_many(group)
        scale = hprlp.last_setup_many_counts()
        assert scale["members served by group scaling launches"] == K, scale
        hprlp.Solver.set_matrix_many(group, [new_values(lp, 700 + k) for k in range(K)])
        first = hprlp.last_values_many_counts()
        hprlp.Solver.set_matrix_many(group, [new_values(lp, 800 + k) for k in range(K)])
        second = hprlp.last_values_many_counts()
        print(K, "scale_many", scale, "first", first, "second", second)
        assert first[MAPS] == K and second[MAPS] == 0 and second[SERVED] == K and second[OWN] == 0, (first, second)
        assert second["host waits"] == 1 + scale["scaling host waits"], (second, scale)
        assert second["memsets"] == 1, second
        assert second["host-to-device copies"] == 1 + 1 + scale["scaling host waits"], (second, scale)
        assert second["device-to-host copies"] == 1 + scale["scaling host waits"], (second, scale)
        # the check, then scatter, gather and zeroing in front of the scaling's own launches
        assert second["kernel launches"] == 1 + 3 + scale["scaling launches"], (second, scale)
        seen[K] = second
        close(group)
    assert {k: v for k, v in seen[5].items() if k != SERVED} == {k: v for k, v in seen[20].items() if k != SERVED}, seen
    model.free()
