"""Wide members on the GPU: solvers past the single-workgroup size that iterate in the group launches (many.cpp: record_normal,
power_wide, loop_many; kernels.hip: k_spmv_fused_many<XEpi<false> / YEpi<false> / PlainPushEpi / PlainEpi<true>>,
k_mapped_many<PwNormalizeTask>, k_reduce_many<PwErrTask>; DESIGN.md "Many small LPs", wide members).  The criterion is the series':
a workgroup of a group kernel runs the single kernel's body as workgroup lb of its member's own grid, so every assertion on a
result is == or np.array_equal against the member's own launches; nothing has a tolerance.

The members are the smallest LPs that are off the small path for each reason and still reach every row kind of the stream kernel:
  W1  2049 x 2600, 9000 entries   one row past the small path's 2048: 33 row blocks, a ragged last workgroup of four waves
  W2  700 x 1100, 13000 entries   past the small path's 12 288 entries
  W3  long_row_lp()               a 300-entry row (vector mode)
  W4  60 x 5000                   rows of 3000 (vector mode: the eight-wide trips, the four-wide trip and the masked tail), 64 and 65
                                  entries, two empty rows, an empty column, every bound kind
  N1  40 x 6000                   a row of 4200 entries, past kSplitRow = 4096: split rows, cannot join
  S1  300 x 500, 2500 entries     on the small path"""
import re

import numpy as np
import pytest
from scipy import sparse

import evalcases
from conftest import hprlp, lpgen
from test_gpu_many import FIELDS, assert_same_result, close_all, long_row_lp, prepared
from test_gpu_many_detect import assert_same_certificate
from test_gpu_many_resolve import new_data
from test_gpu_many_setup import SCALED, TIMES
from test_gpu_many_values import new_values, set_alone
from test_gpu_small import CHECK_VECS, VECS, make

pytestmark = pytest.mark.gpu

_lps = {}


def with_long_rows(m, n, base_nnz, row_lens, seed, empty_rows=(), empty_cols=()):
    A0 = lpgen.planted_lp(m, n, base_nnz, seed, dense_col_frac=0.0)["A"]
    A, facts = evalcases._with_lines(A0, row_lens, (), seed + 1, empty_rows=empty_rows, empty_cols=empty_cols)
    assert sorted(facts["rows"].values()) == sorted(row_lens), facts
    lp = evalcases.all_bounds_lp(A, seed + 2)
    lp["facts"] = facts
    return lp


def lp_of(name):
    if name not in _lps:
        if name == "W1":
            _lps[name] = lpgen.planted_lp(2049, 2600, 9000, 5)
        elif name == "W2":
            _lps[name] = lpgen.planted_lp(700, 1100, 13000, 5)
        elif name == "W3":
            _lps[name] = long_row_lp()
        elif name == "W4":
            lp = with_long_rows(60, 5000, 2500, (3000, 64, 65), 61, empty_rows=(0, 0), empty_cols=(0,))
            lr, lc = np.diff(lp["rowptr"]), np.diff(lp["A"].tocsc().indptr)
            assert (lr[lp["facts"]["empty_rows"]] == 0).all() and (lc[lp["facts"]["empty_cols"]] == 0).all()
            _lps[name] = lp
        elif name == "N1":
            _lps[name] = with_long_rows(40, 6000, 2000, (4200,), 71)
        elif name == "S1":
            _lps[name] = lpgen.planted_lp(300, 500, 2500, 5)
        else:
            raise KeyError(name)
    return _lps[name]


def form(s):
    """(on the small path, A tiled or A^T tiled, split rows of A, split rows of A^T) from info() and describe()."""
    d = s.describe()
    split = [int(v) for v in re.findall(r"stream kernel \(k_spmv_fused, \d+ row blocks, (\d+) split rows\)", d)]
    tiled = s.info()["tiled"]
    return bool(tiled & 4), bool(tiled & 3), split


def wide_group(names, prms=None, scale_only=False, flag=True):
    """Models, a group with every member marked wide (flag) and its controls, which are never marked."""
    models = [make(lp_of(n)) for n in names]
    group, ctrl = prepared(models, prms, scale_only), prepared(models, prms, scale_only)
    if flag:
        for g in group:
            g.set_group_wide()
    return models, group, ctrl


def test_the_members_are_what_the_tests_take_them_for(gpu):
    names = ["W1", "W2", "W3", "W4", "N1", "S1"]
    models = [make(lp_of(n)) for n in names]
    solvers = prepared(models, scale_only=True)
    for n, s in zip(names, solvers):
        small, tiled, split = form(s)
        print(n, s.info(), s.describe())
        assert not tiled and len(split) == 2, (n, s.describe())
        if n == "S1":
            assert small and split == [0, 0]
            assert s.set_group_wide() is True          # (it joins anyway)
        elif n == "N1":
            assert not small and split[0] > 0, (n, split)
            assert s.set_group_wide() is False         # (stored, but it cannot join)
        else:
            assert not small and split == [0, 0], (n, split)
            assert s.set_group_wide() is True
            assert s.set_group_wide(False) is False
    for n, s in zip(names, solvers):                   # (every member is more than one workgroup of four waves on either matrix)
        i = s.info()
        if n == "N1":                                  # (its grid counts the workgroups that finish the split row as well)
            continue
        assert i["grid_y"] == (i["blocks_A"] + 3) // 4 and i["grid_x"] == (i["blocks_AT"] + 3) // 4, (n, i)
        assert n == "S1" or (i["grid_y"] > 1 and i["grid_x"] > 1), (n, i)
    ragged = [n for n, s in zip(names, solvers) if s.info()["blocks_A"] % 4 or s.info()["blocks_AT"] % 4]
    assert ragged, "no member has a ragged last workgroup"
    local = hprlp.Solver.local_group(1)
    sharded = hprlp.Solver.create_local(models[0], hprlp.Parameters(use_presolve=False), 0, 1, local)
    with pytest.raises(RuntimeError, match="sharded"):
        sharded.set_group_wide()
    sharded.close()
    hprlp.Solver.free_local_group(local)
    close_all(solvers, models)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_iterates_equal_the_members_own_launches_bit_for_bit(gpu):
    """[W1, W2, W3, W4, S1], all wide, against five controls that run alone, through the plan of tests/test_gpu_many.py; one round
    gives two members 7 and 6 iterations (two segments), one round gives a member none."""
    names = ["W1", "W2", "W3", "W4", "S1"]
    models, group, ctrl = wide_group(names, scale_only=True)
    for g, c in zip(group, ctrl):
        lam, _ = c.power_iteration()
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    plan = [(1, False), (7, True), (64, False), (149, True), (3, False)]
    for step, (normal, check) in enumerate(plan):
        counts = [normal] * 5
        if step == 1:
            counts[3] = 6          # W1 .. W3 run 7, W4 runs 6: two segments
        if step == 2:
            counts[2] = 0          # in no segment
            before = {k: group[2].get(k) for k in VECS}
            k_before = (group[2].scalars()["kx"], group[2].scalars()["ky"])
        hprlp.Solver.iterate_many(group, counts, check)
        wc = hprlp.last_many_wide_counts()
        for c, cnt in zip(ctrl, counts):
            c.iterate(cnt, check)
        for i, (g, c) in enumerate(zip(group, ctrl)):
            for k in VECS + (CHECK_VECS if check else ()):
                assert np.array_equal(g.get(k), c.get(k)), (step, names[i], k)
            sg, sc = g.scalars(), c.scalars()
            assert (sg["kx"], sg["ky"]) == (sc["kx"], sc["ky"]), (step, names[i])
        wide_counts = [cnt for cnt in counts[:4] if cnt > 0]
        assert wc["joined"] == 4 and wc["refused"] == 0, wc
        assert wc["segments"] == len(set(wide_counts)) and wc["normal_launches"] == 2 * max(wide_counts), (step, wc)
        assert wc["member_iterations"] == sum(wide_counts), (step, wc)
        if step == 2:
            assert all(np.array_equal(group[2].get(k), before[k]) for k in VECS)
            assert (group[2].scalars()["kx"], group[2].scalars()["ky"]) == k_before
    assert group[0].scalars()["kx"] != group[3].scalars()["kx"]  # (the 7 / 6 round left them apart)
    assert group[0].get("x").any() and group[3].get("y").any()
    close_all(group + ctrl, models)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_power_iterations_equal_the_members_own(gpu):
    names = ["W1", "W2", "W3", "W4"]
    models, group, ctrl = wide_group(names, scale_only=True)
    many = hprlp.Solver.power_iteration_many(group)
    wc = hprlp.last_many_wide_counts()
    alone = [c.power_iteration() for c in ctrl]
    print("power iterations", many, wc)
    assert many == alone, (many, alone)
    assert len({it for _, it in many}) > 1       # (not one count for all: every member stopped on its own test)
    assert [g.scalars()["power_iters"] for g in group] == [it for _, it in alone]
    blocks = max(it for _, it in many) // 10
    assert wc["joined"] == 4 and wc["power_waits"] == blocks + 1 and wc["power_launches"] > 0, (wc, blocks)
    for g in group:                              # (the two scratch vectors are left zeroed, as alone)
        assert not g.get("gsm").any() and not g.get("gsn").any()
    capped = hprlp.Solver.power_iteration_many(group, max_iter=25)
    assert [it for _, it in capped] == [25] * 4
    assert capped == [c.power_iteration(max_iter=25) for c in ctrl]
    short = hprlp.Solver.power_iteration_many(group, max_iter=7)   # (no block at all: lambda stays 1.0)
    assert short == [c.power_iteration(max_iter=7) for c in ctrl] and short[0] == (1.0, 7)
    # the iterates after the group's power iteration are the controls' (the scratch vectors are the half-steps' gathered ones)
    for g, c, (lam, _) in zip(group, ctrl, alone):
        g.init(-1.0, lam * 1.01)
        c.init(-1.0, lam * 1.01)
    hprlp.Solver.iterate_many(group, [5] * 4, True)
    for g, c in zip(group, ctrl):
        c.iterate(5, True)
        for k in VECS + CHECK_VECS:
            assert np.array_equal(g.get(k), c.get(k)), k
    close_all(group + ctrl, models)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_whole_runs_equal_each_members_own_run(gpu):
    names = ["W1", "W2", "W3", "W4", "N1", "S1"]
    prms = [hprlp.Parameters(use_presolve=False, stop_tol=1e-6, max_iter=20000)] * 6
    models, group, ctrl = wide_group(names, prms, flag=False)
    joins = [g.set_group_wide() for g in group[:5]]
    assert joins == [True, True, True, True, False]
    out = hprlp.Solver.run_many(group)
    wc, rc = hprlp.last_many_wide_counts(), hprlp.last_run_many_counts()
    alone = [c.run(max_trace=1) for c in ctrl]
    print("iterations", [(r.status, r.iter) for r in out], wc, rc)
    for k in range(6):
        assert_same_result(out[k], alone[k], names[k])
    assert wc["joined"] == 4 and wc["refused"] == 1, wc
    assert wc["normal_launches"] > 0 and wc["member_iterations"] > 0
    assert len({r.iter for r in out[:4]}) > 1    # (they finish at different iterations: the group is seen to shrink)
    close_all(group + ctrl, models)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_the_counts_do_not_depend_on_the_number_of_members(gpu):
    """K solvers on the same W1 model walk the same trajectory, so rounds and restarts are the same for every K."""
    model = make(lp_of("W1"))
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-30, max_iter=450)

    def run(K, flag):
        group = prepared([model] * K, [prm] * K)
        if flag:
            assert all(g.set_group_wide() for g in group)
        out = hprlp.Solver.run_many(group)
        rc, wc = hprlp.last_run_many_counts(), hprlp.last_many_wide_counts()
        close_all(group)
        assert all(r.status == "ITER_LIMIT" and r.iter == 450 for r in out)
        for r in out[1:]:
            assert_same_result(r, out[0], K)
        return out[0], rc, wc

    r2, c2, w2 = run(2, True)
    r6, c6, w6 = run(6, True)
    print("K = 2", c2, w2, "K = 6", c6, w6)
    assert_same_result(r2, r6, "K")
    for f in ("rounds", "waits", "group_launches", "copies"):
        assert c2[f] == c6[f] and c2[f] > 0, (f, c2, c6)
    assert c2["own"] == 2 and c6["own"] == 6, (c2, c6)          # (only the iteration-0 evaluations)
    assert w2["joined"] == 2 and w6["joined"] == 6
    # 450 iterations: every one is a normal iteration or a check step; the rounds at 0, 150, 300 and 450 evaluate, and each of the
    # first three is followed by a check step (a restart's comes inside the restart, and costs the next segment one iteration)
    checks = c2["rounds"] - 1
    assert 0 < checks <= 450
    restarts = (c2["waits"] - c2["rounds"]) // 2
    for w in (w2, w6):
        assert w["normal_launches"] == 2 * (450 - checks - restarts), (w, c2, checks, restarts)
        assert w["segments"] == checks                          # (equal members: one segment per round)
    assert w6["member_iterations"] == 3 * w2["member_iterations"] == 3 * 2 * (450 - checks - restarts)
    # the flag off: the parent's counts -- every round's normal iterations and check step are a member's own
    off, coff, _ = run(2, False)
    again, cagain, _ = run(2, False)
    print("flag off", coff)
    assert_same_result(off, r2, "flag off")
    assert coff["own"] > 2 and coff == cagain, (coff, cagain)  # (nothing is latched)
    assert coff["rounds"] == c2["rounds"]
    model.free()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
DETECT_PRM = dict(use_presolve=False, stop_tol=1e-4, max_iter=50000, use_CR_scaling=False)


def test_detection_of_wide_members_is_the_groups(gpu):
    """W1's pattern with a planted infeasible right-hand side and an unbounded twin (as tests/test_gpu_many_detect.py makes them),
    in a wide group with two feasible members: verdict, iteration and certificate are each member's own run() with detection.
    (Seeds: with that file's 21 the infeasible LP on this pattern is unbounded in its cost as well and ends DUAL_INFEASIBLE; 23 and
    25 end with one verdict of each kind, on an MI355X at iterations 1050 and 450: two rounds with a certificate.)"""
    A = lp_of("W1")["A"]
    lps = [lpgen.planted_infeasible_lp(2049, 2600, 9000, 23, A=A), lpgen.planted_unbounded_lp(2049, 2600, 9000, 25, A=A), lp_of("W2"), lp_of("W3")]
    models = [make(lp) for lp in lps]
    prms = [hprlp.Parameters(**DETECT_PRM)] * 4
    group, ctrl = prepared(models, prms), prepared(models, prms)
    for g, c in zip(group, ctrl):
        assert g.set_group_wide()
        g.set_detection()
        c.set_detection()
    out = hprlp.Solver.run_many(group)
    counts, wc = hprlp.last_run_many_detect_counts(), hprlp.last_many_wide_counts()
    alone = [c.run(max_trace=1) for c in ctrl]
    print("verdicts", [(r.status, r.iter) for r in out], counts, wc)
    assert [r.status for r in out] == ["PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL", "OPTIMAL"]
    for k in range(4):
        assert_same_result(out[k], alone[k], k)
        assert_same_certificate(group[k].certificate(), ctrl[k].certificate(), k)
    assert group[0].certificate().kind == 1 and group[1].certificate().kind == 2 and group[2].certificate().kind == 0
    assert counts["certs_served"] == 2 and counts["ray_served"] > 0, counts
    assert counts["own"] == 4 and wc["joined"] == 4              # (only the iteration-0 evaluations are a member's own)
    close_all(group + ctrl, models)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_solve_many_wide_equals_each_models_own_solve(gpu):
    names = ["W1", "W2", "W3", "S1"]
    models = [make(lp_of(n)) for n in names]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-6, max_iter=20000)
    out, certs = hprlp.solve_many_wide(models, prm)
    wc, rc = hprlp.last_many_wide_counts(), hprlp.last_run_many_counts()
    print("iterations", [(r.status, r.iter) for r in out], wc, rc, hprlp.last_setup_many_counts())
    for k, m in enumerate(models):
        assert_same_result(out[k], m.solve(prm), names[k])
        assert certs[k].kind == 0
    assert wc["joined"] == 3 and wc["refused"] == 0 and wc["normal_launches"] > 0 and wc["power_launches"] > 0, wc
    assert rc["own"] == 4                                        # (only the iteration-0 evaluations)
    assert hprlp.last_setup_many_counts()["members served by group scaling launches"] == 4
    close_all((), models)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
SERVED, OWN = "members served by group launches", "members that went their own way"


def test_the_other_group_entries_serve_wide_members(gpu):
    """scale_many, set_data_many + resolve_many and set_matrix_values_many on [W1, W3, S1], all wide: their kinds run a member's
    own grid at any size, so the wide members are SERVED by the group launches, with the bits of their own calls."""
    names = ["W1", "W3", "S1"]
    lps = [lp_of(n) for n in names]
    models = [make(lp) for lp in lps]
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-4, max_iter=3000)
    group, ctrl = [hprlp.Solver(m, prm) for m in models], [hprlp.Solver(m, prm) for m in models]
    for g in group:
        g.set_group_wide()
    hprlp.Solver.scale_many(group)
    sc = hprlp.last_setup_many_counts()
    assert sc["members served by group scaling launches"] == 3 and sc["members that scaled on their own"] == 0, sc
    for g, c, n in zip(group, ctrl, names):
        c.scale()
        for k in SCALED:
            assert np.array_equal(g.get(k), c.get(k)), (n, k)
        sg, scl = g.scalars(), c.scalars()
        for k in sg:
            if k not in TIMES:
                assert sg[k] == scl[k], (n, k)
    many = hprlp.Solver.power_iteration_many(group)
    for g, c, pw in zip(group, ctrl, many):
        lam, it = c.power_iteration()
        assert pw == (lam, it)
        g.init(-1.0, 1.01 * lam)
        c.init(-1.0, 1.01 * lam)
    # new data, then the re-solve
    data = [new_data(lp, 30 + k, "both") for k, lp in enumerate(lps)]
    hprlp.Solver.set_data_many(group, data)
    cnt = hprlp.last_resolve_many_counts()
    assert cnt[SERVED] == 3 and cnt[OWN] == 0, cnt
    for g, c, d, n in zip(group, ctrl, data, names):
        c.set_data(**d)
        for k in ("AL", "AU", "l", "u", "c"):
            assert np.array_equal(g.get(k), c.get(k)), (n, k)
    got = hprlp.Solver.resolve_many(group)
    cnt = hprlp.last_resolve_many_counts()
    assert cnt[SERVED] == 3 and cnt[OWN] == 0 and cnt["loop operations issued for one member"] == 0, cnt
    for r, c, n in zip(got, ctrl, names):
        assert_same_result(r, c.resolve(), n)
    assert all(r.iter > 0 for r in got)
    # new matrix values
    values = [new_values(lp, 70 + k) for k, lp in enumerate(lps)]
    hprlp.Solver.set_matrix_many(group, values)
    cnt = hprlp.last_values_many_counts()
    assert cnt[SERVED] == 3 and cnt[OWN] == 0, cnt
    for g, c, d, n in zip(group, ctrl, values, names):
        set_alone(c, d)
        for k in SCALED + VECS + CHECK_VECS:
            assert np.array_equal(g.get(k), c.get(k)), (n, k)
    many = hprlp.Solver.power_iteration_many(group)
    for g, c, pw in zip(group, ctrl, many):
        assert pw == c.power_iteration()
    close_all(group + ctrl, models)
