"""Group device re-solve of many small LPs on the GPU (hprlp_solver_set_data_many_device, hprlp_solver_resolve_many_device,
hprlp_solver_set_matrix_values_many_device; csrc/many.cpp, the group kind DataCheckTask of csrc/kernels.hip; DESIGN.md "Many small
LPs", group device re-solve).  The device entries change where the vectors are read and where the solutions are written, never the
arithmetic or its order: every member must be bit for bit where the HOST group entry with the same numbers leaves it.  The
reference of every comparison is therefore a second, identically prepared group driven through the host group entries (a third
set of singly driven solvers where a test says so), and everything below is == or np.array_equal: nothing has a tolerance.  (Of
scalars() the wall times are left out: they are clock readings, not results.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import hprlp
from resolve_device_cases import dev, loaded_hip_runtime, torch_
from test_gpu_many import SIX, assert_same_result, long_row_lp, make, planted, prepared
from test_gpu_many_resolve import (DATA_VECS, DETECT, close, eleven_lps, eleven_parts, group_and_controls, new_data, params,
                                   same_data_state, starts_for)
from test_gpu_many_values import assert_same_state, new_values, state
from test_resolve import base_lp

pytestmark = pytest.mark.gpu

SERVED, OWN = "members served by group launches", "members that went their own way"
SET_DATA, RESOLVE, SET_MATRIX = ("hprlp_solver_set_data_many_device", "hprlp_solver_resolve_many_device",
                                 "hprlp_solver_set_matrix_values_many_device")


def tensors(d):
    """A member's dict of numpy vectors as a dict of device tensors (obj_constant stays a host number)."""
    return None if d is None else {k: (v if k == "obj_constant" else dev(v)) for k, v in d.items()}


def to_host(r):
    for f in ("x", "y", "z"):
        v = getattr(r, f)
        if v is not None and not isinstance(v, np.ndarray):
            assert v.is_cuda and v.dtype == torch_().float64
            setattr(r, f, v.cpu().numpy())
    return r


def give_data(group, ctrl, data, tdata=None):
    """set_data_many_tensors on the device group, set_data_many with the same numbers on the control."""
    hprlp.Solver.set_data_many_tensors(group, tdata if tdata is not None else [tensors(d) for d in data])
    cnt, dcnt = hprlp.last_resolve_many_counts(), hprlp.last_many_device_counts()
    hprlp.Solver.set_data_many(ctrl, data)
    return cnt, dcnt


def t_or_none(v):
    return None if v is None else dev(v)


def resolve_both(group, ctrl, starts, out=None):
    xs, ys, sg = ([s[i] for s in starts] for i in range(3))
    got = hprlp.Solver.resolve_many_tensors(group, [t_or_none(x) for x in xs], [t_or_none(y) for y in ys], sg, out=out)
    cnt, dcnt = hprlp.last_resolve_many_counts(), hprlp.last_many_device_counts()
    ref = hprlp.Solver.resolve_many(ctrl, xs, ys, sg)
    return [to_host(r) for r in got], ref, cnt, dcnt


def words(s):
    t = s.transfer()
    return t["h2d_bytes"], t["d2h_bytes"], t["device_entry"]


def assert_same_certificate(g, c, it):
    kg, kc = g.certificate(), c.certificate()
    assert kg.kind == kc.kind == 1 and kg.iter == kc.iter == it
    assert (kg.objective, kg.violation) == (kc.objective, kc.violation)
    assert np.array_equal(kg.y, kc.y) and np.array_equal(kg.z, kc.z)


# ---- 1. set_data ---------------------------------------------------------------------------------------------------------------------
def test_set_data_by_bits_and_counts(gpu):
    """Every part at least twice over the eleven members, as tensors, against set_data_many with the same numbers; nothing but
    task tables goes up, and copies back and waits are the same at K = 4 and K = 11."""
    seen = {}
    for K in (4, 11):
        lps, parts = eleven_lps()[:K], eleven_parts()[:K]
        models, group, ctrl = group_and_controls(lps)
        untouched = {k: {v: group[k].get(v) for v in DATA_VECS} for k in range(K)}
        data = [new_data(lp, 100 + k, parts[k]) for k, lp in enumerate(lps)]
        cnt, dcnt = give_data(group, ctrl, data)
        print(K, cnt, dcnt)
        given = [k for k, p in enumerate(parts) if p not in ("obj", "nothing")]
        assert cnt[SERVED] == len(given) and cnt[OWN] == 0, cnt
        assert dcnt["members served by group launches"] == len(given) and dcnt["members on their own"] == 0, dcnt
        assert dcnt["check-kernel launches"] == 1 and dcnt["flag words copied back"] == K and dcnt["waits before the first write"] == 1, dcnt
        assert dcnt["device pointers checked"] == sum(len([v for v in d if v != "obj_constant"]) for d in data if d), dcnt
        for k, (g, c) in enumerate(zip(group, ctrl)):
            same_data_state(g, c, (K, k, parts[k]))
            if k in given:
                assert words(g) == (0, 0, 1), (K, k, g.transfer())
                assert any(not np.array_equal(g.get(v), untouched[k][v]) for v in ("c", "AL")), (K, k)   # (what was given has arrived)
            if parts[k] == "nothing":
                assert all(np.array_equal(g.get(v), untouched[k][v]) for v in DATA_VECS), (K, k)
        seen[K] = cnt
        close(group + ctrl, models)
    # host-to-device: the tables of the check's launch and of the data passes' run, nothing else
    assert seen[4]["host-to-device copies"] <= 2 and seen[11]["host-to-device copies"] <= 2, seen
    for key in ("device-to-host copies", "host waits outside the loop", "host-to-device copies", "memsets"):
        assert seen[4][key] == seen[11][key], (key, seen)
    assert seen[11]["host waits outside the loop"] == 2 and seen[11]["memsets"] == 1, seen   # (the check's, the scalars')


# ---- 2. resolve ----------------------------------------------------------------------------------------------------------------------
def test_resolve_by_bits_three_rounds(gpu):
    """The six start kinds against resolve_many; the detection member's verdict and certificate; a second round that writes the
    solution over the tensors it started from; a third round back on the host entries of the same group."""
    torch = torch_()
    lps = eleven_lps()
    models, group, ctrl = group_and_controls(lps, detect=(DETECT,))
    parts = eleven_parts()
    give_data(group, ctrl, [new_data(lp, 100 + k, parts[k]) for k, lp in enumerate(lps)])
    got, ref, cnt, dcnt = resolve_both(group, ctrl, starts_for(lps, cold=(DETECT,)))
    print("round 1", cnt, dcnt, [r.iter for r in got], [r.status for r in got])
    assert cnt[SERVED] == 11 and cnt[OWN] == 0 and cnt["loop operations issued for one member"] == 0, cnt
    assert cnt["host-to-device copies"] <= 3 and cnt["memsets"] == 1, cnt   # (tables only: the check's, the loop's first, the solution's)
    assert dcnt["check-kernel launches"] == 1 and dcnt["waits before the first write"] == 1, dcnt
    for k in range(11):
        assert_same_result(got[k], ref[k], ("round 1", k))
        assert words(group[k]) == (0, 0, 1), (k, group[k].transfer())
    assert got[DETECT].status == "PRIMAL_INFEASIBLE" and "OPTIMAL" in [r.status for r in got]
    assert_same_certificate(group[DETECT], ctrl[DETECT], got[DETECT].iter)
    # all cold: no check launch, no extra wait
    cold, cold_ref, cnt0, dcnt0 = resolve_both(group, ctrl, [(None, None, None)] * 11)
    assert dcnt0["check-kernel launches"] == 0 and dcnt0["waits before the first write"] == 0 and cnt0["memsets"] == 0, (cnt0, dcnt0)
    assert cnt0["host waits outside the loop"] == cnt["host waits outside the loop"] - 1, (cnt0, cnt)
    for k in range(11):
        assert_same_result(cold[k], cold_ref[k], ("cold", k))
    assert any(got[k].iter != cold[k].iter or not np.array_equal(got[k].x, cold[k].x) for k in (1, 2, 3, 4, 7, 9, 10))   # (the starts were read)
    # round 2: other data; x and y of round 1 carried on the device, the solution written over them (the detection member cold)
    give_data(group, ctrl, [dict(new_data(lp, 200 + k, "both"), obj_constant=1.5) for k, lp in enumerate(lps)])
    xs = [None if k == DETECT else dev(got[k].x) for k in range(11)]
    ys = [None if k == DETECT else dev(got[k].y) for k in range(11)]
    out = [(xs[k] if xs[k] is not None else torch.empty(lp["n"], dtype=torch.float64, device="cuda"),
            ys[k] if ys[k] is not None else torch.empty(lp["m"], dtype=torch.float64, device="cuda"),
            None if k == 3 else torch.empty(lp["n"], dtype=torch.float64, device="cuda")) for k, lp in enumerate(lps)]   # (one z not wanted)
    carried = hprlp.Solver.resolve_many_tensors(group, xs, ys, out=out)
    ref2 = hprlp.Solver.resolve_many(ctrl, [None if k == DETECT else got[k].x for k in range(11)],
                                     [None if k == DETECT else got[k].y for k in range(11)])
    for k in range(11):
        assert carried[k].x is out[k][0] and carried[k].y is out[k][1] and carried[k].z is out[k][2]
        r = to_host(carried[k])
        assert (r.status, r.iter, r.primal_obj, r.residuals, r.gap) == (ref2[k].status, ref2[k].iter, ref2[k].primal_obj, ref2[k].residuals, ref2[k].gap), k
        assert np.array_equal(r.x, ref2[k].x) and np.array_equal(r.y, ref2[k].y), k
        assert (r.z is None and k == 3) or np.array_equal(r.z, ref2[k].z), k
    # round 3: the host entries on the device group
    data3 = [new_data(lp, 300 + k, "both") for k, lp in enumerate(lps)]
    hprlp.Solver.set_data_many(group, data3)
    hprlp.Solver.set_data_many(ctrl, data3)
    starts = starts_for(lps, shift=2, cold=(DETECT,))
    xs, ys, sg = ([s[i] for s in starts] for i in range(3))
    back, ref3 = hprlp.Solver.resolve_many(group, xs, ys, sg), hprlp.Solver.resolve_many(ctrl, xs, ys, sg)
    for k in range(11):
        assert_same_result(back[k], ref3[k], ("round 3", k))
        assert words(group[k])[2] == 0
    # ... and the device entries once more
    give_data(group, ctrl, [new_data(lp, 400 + k, "c") for k, lp in enumerate(lps)])
    again, ref4, _, _ = resolve_both(group, ctrl, starts_for(lps, shift=4, cold=(DETECT,)))
    for k in range(11):
        assert_same_result(again[k], ref4[k], ("round 4", k))
    close(group + ctrl, models)


# ---- 3. packed tensors ---------------------------------------------------------------------------------------------------------------
def test_packed_tensors_and_the_lookups(gpu):
    """All members' vectors cut from ONE tensor per kind at running offsets, the first slice at element 1: slices that are 8-byte
    but not 16-byte aligned.  Each packed tensor is an allocation of its own (above the size from which torch's allocator gives a
    tensor its own block), so the runtime is asked once per kind whatever K is."""
    torch = torch_()
    seen = {}
    for K in (4, 11):
        lps = eleven_lps()[:K]
        models, group, ctrl = group_and_controls(lps)
        data = [new_data(lp, 500 + k, "both") for k, lp in enumerate(lps)]
        packed = None
        torch.cuda.empty_cache()   # (no cached block of an earlier test that two of the five could share)
        packed = {v: torch.empty(1_500_000, dtype=torch.float64, device="cuda") for v in DATA_VECS}   # (12 MB each)
        at = {v: 1 for v in DATA_VECS}
        tdata, odd = [], 0
        for d in data:
            td = {}
            for v in DATA_VECS:
                a = np.ascontiguousarray(d[v], dtype=np.float64)
                td[v] = packed[v][at[v]:at[v] + a.shape[0]]
                td[v].copy_(torch.from_numpy(a))
                odd += td[v].data_ptr() % 16 == 8
                at[v] += a.shape[0]
            tdata.append(td)
        assert odd >= K   # (every kind's first slice at least)
        cnt, dcnt = give_data(group, ctrl, data, tdata)
        print(K, cnt, dcnt)
        assert cnt[SERVED] == K and cnt[OWN] == 0, cnt
        for k, (g, c) in enumerate(zip(group, ctrl)):
            same_data_state(g, c, ("packed", K, k))
        seen[K] = dcnt
        # the starts and the solutions packed the same way
        n_all, m_all = sum(lp["n"] for lp in lps), sum(lp["m"] for lp in lps)
        X, Z = (torch.zeros(1 + n_all, dtype=torch.float64, device="cuda") for _ in range(2))
        Y = torch.zeros(1 + m_all, dtype=torch.float64, device="cuda")
        starts = starts_for(lps, shift=3)
        xs, ys, out, an, am = [], [], [], 1, 1
        for lp, (x0, y0, _) in zip(lps, starts):
            vx, vy, vz = X[an:an + lp["n"]], Y[am:am + lp["m"]], Z[an:an + lp["n"]]
            an, am = an + lp["n"], am + lp["m"]
            if x0 is not None:
                vx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
            if y0 is not None:
                vy.copy_(torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float64)))
            xs.append(vx if x0 is not None else None)
            ys.append(vy if y0 is not None else None)
            out.append((vx, vy, vz))
        got = hprlp.Solver.resolve_many_tensors(group, xs, ys, [s[2] for s in starts], out=out)
        ref = hprlp.Solver.resolve_many(ctrl, [s[0] for s in starts], [s[1] for s in starts], [s[2] for s in starts])
        for k in range(K):
            assert_same_result(to_host(got[k]), ref[k], ("packed", K, k))
        close(group + ctrl, models)
    assert seen[4]["lookups issued to the runtime"] == seen[11]["lookups issued to the runtime"] == len(DATA_VECS), seen
    assert seen[4]["device pointers checked"] == 5 * 4 and seen[11]["device pointers checked"] == 5 * 11, seen


# ---- 4. set_matrix -------------------------------------------------------------------------------------------------------------------
def solve_both(group, ctrl, what):
    many, many_c = hprlp.Solver.power_iteration_many(group), hprlp.Solver.power_iteration_many(ctrl)
    assert many == many_c, what
    for g, c, (lam, _) in zip(group, ctrl, many):
        g.init(-1.0, 1.01 * lam)
        c.init(-1.0, 1.01 * lam)
    got, ref = hprlp.Solver.resolve_many_tensors(group), hprlp.Solver.resolve_many(ctrl)
    for k in range(len(group)):
        assert_same_result(to_host(got[k]), ref[k], (what, k))
    return got


def test_set_matrix_by_bits(gpu):
    """Values and the five vectors as tensors against set_matrix_many: every named device vector (A_val, AT_val, row_norm,
    col_norm, the five data vectors, the iterates), the scalars, then power iteration and re-solve; twice (the first call builds
    the value maps).  The device call waits as often as the host call."""
    lps = eleven_lps()
    models, group, ctrl = group_and_controls(lps)
    for rnd in range(2):
        data = [new_values(lp, 10 + 40 * rnd + k) for k, lp in enumerate(lps)]
        if rnd == 1:
            data[4] = None   # (a member that is skipped keeps every bit)
            kept = state(group[4])
        hprlp.Solver.set_matrix_many_tensors(group, [tensors(d) for d in data])
        cnt, dcnt = hprlp.last_values_many_counts(), hprlp.last_many_device_counts()
        hprlp.Solver.set_matrix_many(ctrl, data)
        host = hprlp.last_values_many_counts()
        print(rnd, cnt, dcnt, host)
        K = sum(d is not None for d in data)
        assert cnt[SERVED] == K and cnt[OWN] == 0 and host[SERVED] == K, (cnt, host)
        assert cnt["host waits"] == host["host waits"] == 4, (cnt, host)
        assert cnt["host-to-device copies"] == host["host-to-device copies"] - 1, (cnt, host)   # (the host call's staging block)
        assert cnt["memsets"] == 1 and dcnt["check-kernel launches"] == 2 and dcnt["flag words copied back"] == 22, (cnt, dcnt)
        assert dcnt["device pointers checked"] == 6 * K and dcnt["waits before the first write"] == 1, dcnt
        for k, (g, c) in enumerate(zip(group, ctrl)):
            assert_same_state(state(g), state(c), (rnd, k))
            if data[k] is not None:
                assert words(g) == (0, 0, 1), (k, g.transfer())
        if rnd == 1:
            assert_same_state(state(group[4]), kept, "skipped")
        else:
            solve_both(group, ctrl, rnd)
    close(group + ctrl, models)


# ---- 5. members that do not join -------------------------------------------------------------------------------------------------------
def drive_singly(singles, lps, data, starts, values):
    """The third set: every solver through its own *_tensors calls."""
    ref = []
    for s, d, (x0, y0, sg) in zip(singles, data, starts):
        s.set_data_tensors(**tensors(d))
        ref.append(to_host(s.resolve_tensors(t_or_none(x0), t_or_none(y0), -1.0 if sg is None else sg)))
    lams = [s.set_matrix_tensors(**tensors(v)) for s, v in zip(singles, values)]
    return ref, lams, [to_host(s.resolve_tensors()) for s in singles]


def drive_group(group, lps, data, starts, values):
    hprlp.Solver.set_data_many_tensors(group, [tensors(d) for d in data])
    c_data = hprlp.last_resolve_many_counts()
    xs, ys, sg = ([s[i] for s in starts] for i in range(3))
    got = [to_host(r) for r in hprlp.Solver.resolve_many_tensors(group, [t_or_none(x) for x in xs], [t_or_none(y) for y in ys], sg)]
    c_res = hprlp.last_resolve_many_counts()
    hprlp.Solver.set_matrix_many_tensors(group, [tensors(v) for v in values])
    c_val = hprlp.last_values_many_counts()
    lams = hprlp.Solver.power_iteration_many(group)
    for g, (lam, _) in zip(group, lams):
        g.init(-1.0, 1.01 * lam)
    return got, lams, [to_host(r) for r in hprlp.Solver.resolve_many_tensors(group)], (c_data, c_res, c_val)


def compare_with_singles(group, singles, lps, seed, want_own, want_served):
    data = [new_data(lp, seed + k, "both") for k, lp in enumerate(lps)]
    starts = starts_for(lps)
    values = [new_values(lp, seed + 50 + k) for k, lp in enumerate(lps)]
    got, lams, after, counts = drive_group(group, lps, data, starts, values)
    ref, lams_s, after_s = drive_singly(singles, lps, data, starts, values)
    print(counts)
    for c in counts:
        assert c[OWN] == want_own and c[SERVED] == want_served, c
    assert list(lams) == list(lams_s), (lams, lams_s)
    for k in range(len(lps)):
        assert_same_result(got[k], ref[k], ("resolve", k))
        assert_same_result(after[k], after_s[k], ("after new values", k))
        assert_same_state(state(group[k]), state(singles[k]), k)
        assert words(group[k]) == (0, 0, 1)


def test_a_member_off_the_small_path_and_a_group_of_one(gpu):
    lps = [planted(SIX[0]), dict(long_row_lp(), x_star=np.full(600, 0.5)), planted(SIX[4]), base_lp(11)]
    models = [make(lp) for lp in lps]
    group, singles = prepared(models, [params()] * 4), prepared(models, [params()] * 4)
    assert not (group[1].info()["tiled"] & 4)
    compare_with_singles(group, singles, lps, 600, want_own=1, want_served=3)
    close(group + singles, models)
    lp = base_lp(12)
    models = [make(lp)]
    group, singles = prepared(models, [params()]), prepared(models, [params()])
    compare_with_singles(group, singles, [lp], 650, want_own=1, want_served=0)
    close(group + singles, models)


def test_a_member_with_a_locality_ordering(gpu):
    """The group's reordered member at the default thresholds (HPRLP_REORDER_ANYWAY, the hook of tests/test_gpu_reorder_small.py,
    is a single solver's matter), so this is the suite's large reordered shape (a randomly permuted banded
    1 600 000 x 1 600 000 matrix, 10 per row; tests/test_gpu_many_values.py) between two small members that join: new data and a
    re-solve from a start, against the member's own *_tensors calls."""
    from scipy import sparse
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
    short = hprlp.Parameters(use_presolve=False, stop_tol=1e-9, max_iter=300, check_iter=150)
    prms = [params(), short, params()]
    group, single = prepared(models, prms), prepared(models[1:2], prms[1:2])
    assert group[1].info()["reordered"] and single[0].info()["reordered"]
    data = [new_data(lp, 700 + k, "both") for k, lp in enumerate(lps)]
    x0, y0 = 0.9 * big["x_star"], 0.9 * big["y_star"]
    hprlp.Solver.set_data_many_tensors(group, [tensors(d) for d in data])
    cnt = hprlp.last_resolve_many_counts()
    assert cnt[OWN] == 1 and cnt[SERVED] == 2, cnt
    got = hprlp.Solver.resolve_many_tensors(group, [None, dev(x0), None], [None, dev(y0), None])
    cnt = hprlp.last_resolve_many_counts()
    assert cnt[OWN] == 1 and cnt[SERVED] == 2, cnt
    single[0].set_data_tensors(**tensors(data[1]))
    ref = to_host(single[0].resolve_tensors(dev(x0), dev(y0)))
    same_data_state(group[1], single[0], "ordered")
    r = to_host(got[1])
    assert r.iter == ref.iter == 300 and np.abs(r.x).max() > 0
    assert_same_result(r, ref, "ordered")
    close(group + single, models)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_member_as_it_was(gpu):
    """After each refused call every member's vectors and scalars are the control's, and a following cold re-solve gives the
    control's result."""
    torch = torch_()
    L = hprlp.lib()
    lps = eleven_lps()[:7]
    K = len(lps)
    models, group, ctrl = group_and_controls(lps)
    data = [new_data(lp, 800 + k, "both") for k, lp in enumerate(lps)]
    give_data(group, ctrl, data)
    ref = hprlp.Solver.resolve_many(ctrl)
    first = [to_host(r) for r in hprlp.Solver.resolve_many_tensors(group)]
    before = [state(c) for c in ctrl]
    stream = torch.cuda.current_stream().cuda_stream
    hs = (C.c_void_p * K)(*[s.h for s in group])

    def still_fine(tag):
        for k, (g, b) in enumerate(zip(group, before)):
            assert_same_state(state(g), b, (tag, k))
        got = hprlp.Solver.resolve_many_tensors(group)
        for k in range(K):
            assert_same_result(to_host(got[k]), ref[k], (tag, k))

    for k in range(K):
        assert_same_result(first[k], ref[k], k)
    still_fine("nothing")
    clean = [tensors(d) for d in data]
    ptr = lambda t: C.cast(C.c_void_p(t.data_ptr()), hprlp.c_dbl_p)

    def raw_data(change):
        arr = (hprlp.CMemberData * K)()
        for k, td in enumerate(clean):
            for v in DATA_VECS:
                setattr(arr[k], v, ptr(td[v]))
        change(arr)
        return arr

    # a host numpy array's address
    host_c = np.ascontiguousarray(data[2]["c"], dtype=np.float64)
    arr = raw_data(lambda a: setattr(a[2], "c", host_c.ctypes.data_as(hprlp.c_dbl_p)))
    assert L.hprlp_solver_set_data_many_device(hs, K, arr, stream) == -1
    msg = hprlp.last_error()
    print("host address ->", msg)
    assert msg.startswith(SET_DATA + ": member 2: c ") and ("device memory" in msg or "runtime" in msg), msg
    still_fine("a host address")
    # a buffer one element short, cut at the end of its allocation (an allocation of its own: a tensor of n - 1 is a piece of
    # torch's larger block, whose range is what the runtime reports)
    hip = loaded_hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 8 * (lps[1]["n"] - 1)) == 0
    try:
        arr = raw_data(lambda a: setattr(a[1], "u", C.cast(short, hprlp.c_dbl_p)))
        assert L.hprlp_solver_set_data_many_device(hs, K, arr, stream) == -1
        msg = hprlp.last_error()
        print("short buffer ->", msg)
        assert msg.startswith(SET_DATA + ": member 1: u is too short"), msg
        still_fine("a short buffer")
        dst = (hprlp.CMemberOut * K)()
        dst[1].z = short.value
        res = (hprlp.CResults * K)()
        assert L.hprlp_solver_resolve_many_device(hs, K, None, dst, stream, res) == -1
        msg = hprlp.last_error()
        print("short output ->", msg)
        assert msg.startswith(RESOLVE + ": member 1: z is too short"), msg
        still_fine("a short output buffer")
    finally:
        assert hip.hipFree(short) == 0

    def with_member(k, d):
        return [tensors(d) if i == k else clean[i] for i in range(K)]

    def nan_at(v, i):
        v = np.array(v, dtype=np.float64)
        v[i] = np.nan
        return v

    # a NaN in AU of member 3 and in c of member 5 together: the lowest member is named
    both = with_member(3, dict(data[3], AU=nan_at(data[3]["AU"], lps[3]["m"] - 1)))
    both[5] = tensors(dict(data[5], c=nan_at(data[5]["c"], 0)))
    with pytest.raises(RuntimeError, match=r"^%s: member 3: AU\[%d\] is NaN" % (SET_DATA, lps[3]["m"] - 1)):
        hprlp.Solver.set_data_many_tensors(group, both)
    dcnt = hprlp.last_many_device_counts()
    assert dcnt["check-kernel launches"] == 1 and dcnt["members served by group launches"] == 0, dcnt
    still_fine("NaN in AU and c")
    # ... and within one member the order of the vectors is c, AL, AU, l, u
    two = with_member(4, dict(data[4], u=nan_at(data[4]["u"], 0), AL=nan_at(data[4]["AL"], 5)))
    with pytest.raises(RuntimeError, match=r"member 4: AL\[5\] is NaN"):
        hprlp.Solver.set_data_many_tensors(group, two)
    still_fine("NaN in AL and u of one member")
    # an inf in x0
    inf_x = np.full(lps[2]["n"], 0.5)
    inf_x[3] = np.inf
    with pytest.raises(RuntimeError, match=r"^%s: member 2: warm start: x0\[3\] is not finite" % RESOLVE):
        hprlp.Solver.resolve_many_tensors(group, x=[None, None, dev(inf_x)] + [None] * (K - 3))
    still_fine("inf in x0")
    with pytest.raises(RuntimeError, match=r"^%s: member 0: sigma is NaN" % RESOLVE):
        hprlp.Solver.resolve_many_tensors(group, sigma=[float("nan")] + [None] * (K - 1))
    # a non-finite value together with a NaN vector of a higher member: the vector's message wins
    values = [new_values(lp, 850 + k) for k, lp in enumerate(lps)]
    bad = [tensors(v) for v in values]
    v1 = values[1]["values"].copy()
    v1[7] = np.inf
    bad[1] = tensors(dict(values[1], values=v1))
    bad[4] = tensors(dict(values[4], l=nan_at(values[4]["l"], 2)))
    with pytest.raises(RuntimeError, match=r"^%s: member 4: l\[2\] is NaN" % SET_MATRIX):
        hprlp.Solver.set_matrix_many_tensors(group, bad)
    still_fine("a non-finite value and a NaN vector")
    bad[4] = tensors(values[4])
    with pytest.raises(RuntimeError, match=r"^%s: member 1: val\[7\] is not finite" % SET_MATRIX):
        hprlp.Solver.set_matrix_many_tensors(group, bad)
    still_fine("a non-finite value")
    # an incomplete bounds group, a wrong nnz, the same handle twice
    half = with_member(2, {k: v for k, v in data[2].items() if k != "AU"})
    with pytest.raises(RuntimeError, match=r"^%s: member 2: AL, AU, l and u are given together" % SET_DATA):
        hprlp.Solver.set_data_many_tensors(group, half)
    still_fine("an incomplete bounds group")
    n0 = len(values[0]["values"])
    wrong = [tensors(v) for v in values]
    wrong[0] = tensors(dict(values[0], values=values[0]["values"][:-1]))
    with pytest.raises(RuntimeError, match=r"^%s: member 0: nnz is %d, the model has %d" % (SET_MATRIX, n0 - 1, n0)):
        hprlp.Solver.set_matrix_many_tensors(group, wrong)
    still_fine("a wrong nnz")
    twice = [group[0], group[1], group[0]]
    for call, entry in ((lambda: hprlp.Solver.set_data_many_tensors(twice, [clean[0], clean[1], clean[0]]), SET_DATA),
                        (lambda: hprlp.Solver.resolve_many_tensors(twice), RESOLVE),
                        (lambda: hprlp.Solver.set_matrix_many_tensors(twice, [tensors(values[k]) for k in (0, 1, 0)]), SET_MATRIX)):
        with pytest.raises(RuntimeError, match=r"^%s: members 0 and 2 are the same solver" % entry):
            call()
    still_fine("the same handle twice")
    # the clean calls afterwards
    hprlp.Solver.set_matrix_many_tensors(group, [tensors(v) for v in values])
    hprlp.Solver.set_matrix_many(ctrl, values)
    for k, (g, c) in enumerate(zip(group, ctrl)):
        assert_same_state(state(g), state(c), ("clean", k))
    close(group + ctrl, models)


# ---- 7. a side stream ------------------------------------------------------------------------------------------------------------------
def test_inputs_produced_on_a_side_stream(gpu):
    """The contract stated: inputs produced by torch kernels on a non-default stream, which the entries are handed; the caller
    does not synchronise between producing them and the calls."""
    torch = torch_()
    lps = eleven_lps()[:5]
    models, group, ctrl = group_and_controls(lps)
    base = [dev(lp["c"]) for lp in lps]
    f = [dev(1 + 1e-3 * np.random.default_rng(70 + k).normal(size=lp["n"])) for k, lp in enumerate(lps)]
    x_base = [dev(0.9 * np.asarray(lp["x_star"], float)) if "x_star" in lp else None for lp in lps]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = [b * g for b, g in zip(base, f)]   # (produced on the side stream, which the entries are handed as the inputs' stream)
        x0 = [None if x is None else x * 1.0 for x in x_base]
        hprlp.Solver.set_data_many_tensors(group, [dict(c=c) for c in c2])
        got = hprlp.Solver.resolve_many_tensors(group, x=x0)
    side.synchronize()
    hprlp.Solver.set_data_many(ctrl, [dict(c=c.cpu().numpy()) for c in c2])
    ref = hprlp.Solver.resolve_many(ctrl, x=[None if x is None else x.cpu().numpy() for x in x0])
    for k, (g, c) in enumerate(zip(group, ctrl)):
        same_data_state(g, c, ("side stream", k))
        assert_same_result(to_host(got[k]), ref[k], ("side stream", k))
    close(group + ctrl, models)
