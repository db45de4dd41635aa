"""Streams with parents on the GPU (include/hprlp_amd.h hprlp_batched_solver_solve_stream_parents / _device, DESIGN.md "Streamed
batches", "Parents"): a queued problem starts from the x, y that an earlier problem of the same queue returned, as soon as that
problem has left and a slot is free.

What is held: for a problem p that sat in slot k, status, iter, x, y, z, primal_obj, residuals, gap and certificate are BIT FOR BIT
those of a plain BatchedSolver.solve() of min(width, N) members whose slot k holds p -- a COLD solve for a cold root, else a WARM
solve whose X0[:, k], Y0[:, k] are the x, y the stream returned for p's parent (a started root: its own columns).  The reference
batches are built from the call's own record and solved on a second handle.  The record is the schedule
hprlp.stream_schedule(iter // check_iter, width, parent) of the GPU's own counts.  Every comparison is made under "no lambda bump"
on both sides, which every test asserts.  All cases run on the planted 300 x 400 network LP of the stream tests."""
import ctypes as C

import numpy as np
import pytest

from conftest import hprlp
from test_gpu_batched_device import T, on_host, torch_, tree_handle
from test_gpu_batched_stream import CERT_SCALARS, CHECK, SCALARS, cert_column, no_bump, params, planted
from test_gpu_batched_stream_device import RECORD, same_stream, scalars_answer
from test_gpu_detect import model_of
from test_gpu_warm import make_batch

pytestmark = pytest.mark.gpu
GARBAGE = 7.0   # in the X0 / Y0 columns of children: a child ignores its own columns


def same_member(out, p, ref, k, detect, tag):
    assert out["status"][p] == ref["status"][k] and out["iter"][p] == ref["iter"][k], \
        (tag, p, k, out["status"][p], ref["status"][k], out["iter"][p], ref["iter"][k])
    for f in ("x", "y", "z"):
        assert np.array_equal(out[f][:, p], ref[f][:, k]), (tag, f, p, k)
    for f in SCALARS:
        assert out[f][p] == ref[f][k], (tag, f, p, k, out[f][p], ref[f][k])
    if detect is None:
        return
    co, cr = out["certificates"], ref["certificates"]
    for f in CERT_SCALARS:
        assert co[f][p] == cr[f][k], (tag, f, p, k)
    for f in ("y", "z", "d"):
        a, b = cert_column(co, f, p), cert_column(cr, f, k)
        if a is None or b is None:
            assert (a is None or not a.any()) and (b is None or not b.any()), (tag, f, p, k)
        else:
            assert np.array_equal(a, b), (tag, f, p, k)


def check_against_references(h2, args, out, width, prm, parent, X0=None, Y0=None, detect=None):
    """Batch g holds in slot k the g-th problem that occupied slot k.  Its cold members go into a cold solve() and its started
    members into a warm one, each with the member in its own slot and a copy of one of the solve's own members in every other."""
    N = args[0].shape[1]
    W = min(width, N)
    parent = np.asarray(parent)
    assert (out["event_in"] >= 0).all()
    lists = [[] for _ in range(W)]
    for p in np.lexsort((np.arange(N), out["event_in"])):
        lists[out["slot"][p]].append(int(p))
    cold = lambda p: parent[p] < 0 and X0 is None
    solves = 0
    for g in range(max(len(lst) for lst in lists)):
        for want_cold in (True, False):
            real = [k for k, lst in enumerate(lists) if g < len(lst) and cold(lst[g]) == want_cold]
            if not real:
                continue
            idx = np.array([lists[k][g] if k in real else lists[real[0]][g] for k in range(W)])
            kw = dict(param=prm)
            if not want_cold:
                sx = np.stack([out["x"][:, parent[p]] if parent[p] >= 0 else X0[:, p] for p in idx], axis=1)
                sy = np.stack([out["y"][:, parent[p]] if parent[p] >= 0 else Y0[:, p] for p in idx], axis=1)
                kw.update(X0=sx, Y0=sy)
            if detect is not None:
                kw.update(eps_primal=detect, eps_dual=detect)
            ref = h2.solve(*(a[:, idx] for a in args), **kw)
            no_bump(h2)
            solves += 1
            for k in real:
                same_member(out, idx[k], ref, k, detect, ("batch", g, "cold" if want_cold else "started"))
    return solves


def check_record(h, out, width, parent, X0=None):
    """The record is the parents schedule of the GPU's own counts, the loop is as long as its makespan, and stream_parents_info()
    agrees with counts taken from the record."""
    N = len(out["iter"])
    W = min(width, N)
    parent = np.asarray(parent)
    assert (out["iter"] % CHECK == 0).all()
    slot, ein, eout = hprlp.stream_schedule(out["iter"] // CHECK, width, parent)
    for f, want in zip(RECORD, (slot, ein, eout)):
        assert np.array_equal(out[f], want), (f, list(out[f]), list(want))
    info = h.stream_info()
    assert info["count"] == N and info["width"] == width
    assert info["loop_iterations"] == int(eout.max()) * CHECK and info["evaluations"] == int(eout.max()) + 1
    assert info["refills"] == N - min(W, int((parent < 0).sum()))   # (the entries after the initial fill, which takes roots alone)
    idle = 0
    for e in range(int(eout.max())):   # after event e the loop goes on: the slots without a member while a problem still waits
        if (ein > e).any():
            idle += W - int(((ein <= e) & (e < eout)).sum())
    pinfo = h.stream_parents_info()
    roots = int((parent < 0).sum())
    assert pinfo == dict(roots=roots, cold_members=roots if X0 is None else 0, children_started=N - roots, idle_slot_events=idle), (pinfo, idle)
    return info, pinfo


def chains(nchain, periods, seed=2):
    """nchain chains x `periods` periods, numbered period by period: period t + 1 of a chain is period t with C perturbed by 1e-3."""
    lp = planted()
    Cm, AL, AU, L, U = make_batch(lp, nchain, seed)
    rng = np.random.default_rng(seed + 100)
    Cs = [Cm]
    for _ in range(periods - 1):
        Cs.append(Cs[-1] * (1 + 1e-3 * rng.normal(size=Cm.shape)))
    rep = lambda a: np.concatenate([a] * periods, axis=1)
    parent = np.array([-1 if p < nchain else p - nchain for p in range(nchain * periods)])
    return lp, (np.concatenate(Cs, axis=1), rep(AL), rep(AU), rep(L), rep(U)), parent


def root_starts(h2, lp, args, parent):
    """A point on the way (a solve to 1e-2) in the roots' columns, GARBAGE in the children's."""
    N = args[0].shape[1]
    roots = np.flatnonzero(np.asarray(parent) < 0)
    rough = h2.solve(*(a[:, roots] for a in args), param=params(stop_tol=1e-2))
    no_bump(h2)
    X0, Y0 = np.full((lp["n"], N), GARBAGE), np.full((lp["m"], N), GARBAGE)
    X0[:, roots], Y0[:, roots] = rough["x"], rough["y"]
    return X0, Y0


# ---- 1. chains, per kernel form; 5. the record --------------------------------------------------------------------------------------
@pytest.mark.parametrize("started", [False, True], ids=["cold_roots", "started_roots"])
@pytest.mark.parametrize("width,chunk,tol,nchain,periods", [(3, 0, 1e-6, 5, 4), (12, 0, 1e-6, 5, 4), (64, 0, 1e-4, 5, 4), (70, 8, 1e-4, 5, 4),
                                                            (64, 0, 1e-4, 66, 2), (70, 8, 1e-4, 72, 2)])
def test_chains_give_the_bits_of_plain_batches(gpu, monkeypatch, width, chunk, tol, nchain, periods, started):
    """width 3: children wait for slots (kb_half); 12: 7 slots are empty at event 0 (kb_halfN<16>); 64 and 70 on 20 problems: 20
    slots, 15 of them empty at event 0 (one chunk of 32, whatever HPRLP_BATCH_CHUNK says below 64 members: kb_halfN<32>); 66 chains
    x 2 periods through 64 slots: kb_half64, roots that wait too; 72 x 2 through 70 slots in chunks of 8: kb_halfN<8>, two chunks'
    worth of dead columns -- slot_elem in every geometry."""
    if chunk:
        monkeypatch.setenv("HPRLP_BATCH_CHUNK", str(chunk))
    lp, args, parent = chains(nchain, periods)
    N = nchain * periods
    model = model_of(lp)
    prm = params(stop_tol=tol)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    X0, Y0 = root_starts(h2, lp, args, parent) if started else (None, None)
    out = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, parent=parent)
    no_bump(h, streamed=True)
    geo = h.info()
    assert (geo["Bp"], geo["Bc"]) == {(3, 0, 5): (4, 4), (12, 0, 5): (16, 16), (64, 0, 5): (32, 32), (70, 8, 5): (32, 32),
                                      (64, 0, 66): (64, 64), (70, 8, 72): (128, 8)}[(width, chunk, nchain)]
    assert out["status"] == ["OPTIMAL"] * N
    solves = check_against_references(h2, args, out, width, prm, parent, X0, Y0)
    info, pinfo = check_record(h, out, width, parent, X0)
    kids = np.flatnonzero(parent >= 0)
    assert (out["event_in"][kids] >= out["event_out"][parent[kids]]).all()
    if width == 12:
        assert pinfo["idle_slot_events"] > 0 and sorted(out["slot"][:5]) == list(range(5)) and out["slot"].max() < 5
    print("width", width, "chunk", chunk, "chains", nchain, "x", periods, "started" if started else "cold", "iter", list(out["iter"][:10]),
          "loop", info["loop_iterations"], "reference solves", solves, pinfo)
    h.close(); h2.close(); model.free()


def test_the_start_has_the_bits_of_prepare_batchs(gpu):
    """The rounding of kb_slot_start is batch_units.h's on both sides: a root started by the kernel from the staged X0 / Y0 and
    the same problem started by a plain warm solve, whose start is scaled on the host, stop after the same iterations at the same
    bits -- with use_bc_scaling on (a division by the member's own scale) and off."""
    lp, args, parent = chains(3, 1)
    model = model_of(lp)
    for bc in (True, False):
        prm = params(stop_tol=1e-4, use_bc_scaling=bc)
        h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
        X0, Y0 = root_starts(h2, lp, args, parent)
        X0 *= 1.0 + 2.0 ** -30   # (no round numbers)
        out = h.solve_stream(*args, width=3, X0=X0, Y0=Y0, parent=parent)
        ref = h2.solve(*args, X0=X0, Y0=Y0, param=prm)
        no_bump(h, streamed=True); no_bump(h2)
        for k in range(3):
            same_member(out, k, ref, k, None, ("bc", bc))
        h.close(); h2.close()
    model.free()


# ---- 2. a binary tree ---------------------------------------------------------------------------------------------------------------
def tree_queue(h2, prm, depth=4):
    """15 nodes, one root: a child is its parent with one variable's u lowered, or l raised, to the parent's rounded value.  The
    data are fixed before the call, level by level, from plain cold solves on h2 (the branching variable only has to be a
    sensible one: the stream's own parents' points are what the children start from)."""
    lp = planted()
    cols = [tuple(a[:, :1] for a in make_batch(lp, 1, 2))]
    parent = [-1]
    level = [0]
    for _ in range(depth - 1):
        sol = h2.solve(*(np.concatenate([cols[p][i] for p in level], axis=1) for i in range(5)), param=prm)
        no_bump(h2)
        nxt = []
        for j, p in enumerate(level):
            x = sol["x"][:, j]
            frac = np.abs(x - np.round(x))
            v = int(np.argmax(frac))
            for down in (True, False):
                Cm, AL, AU, L, U = (np.array(a) for a in cols[p])
                if down:
                    U[v, 0] = np.floor(x[v])
                else:
                    L[v, 0] = np.ceil(x[v])
                nxt.append(len(cols))
                cols.append((Cm, AL, AU, L, U))
                parent.append(p)
        level = nxt
    args = tuple(np.concatenate([c[i] for c in cols], axis=1) for i in range(5))
    return lp, args, np.array(parent)


@pytest.mark.parametrize("width", [4, 64])
def test_a_binary_tree(gpu, width):
    """Width 4: nodes wait for slots; 64: 15 slots, 14 of them empty at event 0, filled as the levels open."""
    model = model_of(planted())
    prm = params(stop_tol=1e-4, max_iter=15000)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    lp, args, parent = tree_queue(h2, prm)
    assert len(parent) == 15 and list(parent[:3]) == [-1, 0, 0]
    out = h.solve_stream(*args, width=width, parent=parent)
    no_bump(h, streamed=True)
    assert set(out["status"]) <= {"OPTIMAL", "ITER_LIMIT"} and out["status"][0] == "OPTIMAL"
    check_against_references(h2, args, out, width, prm, parent)
    info, pinfo = check_record(h, out, width, parent)
    assert list(out["event_in"][:3]) == [0, out["event_out"][0], out["event_out"][0]] and pinfo["idle_slot_events"] > 0
    if width == 64:
        assert h.info()["Bp"] == 16 and len(set(out["slot"])) > 4
    print("width", width, "iter", list(out["iter"]), "slots", list(out["slot"]), pinfo)
    h.close(); h2.close(); model.free()


# ---- 3. the cascade -----------------------------------------------------------------------------------------------------------------
def test_a_child_that_ends_at_once_hands_on_to_its_own_child_within_the_event(gpu):
    """Problems 0, 2, 3 are one LP: the root starts from its solution to 1e-8 and the stream runs at 1e-6, so the root, its child and
    the child's child each end at their iteration-0 evaluation, one pass after the other within event 0.  Problem 1 is a cold root."""
    lp = planted()
    two = make_batch(lp, 2, 2)
    args = tuple(a[:, [0, 1, 0, 0]] for a in two)
    parent = np.array([-1, -1, 0, 2])
    model = model_of(lp)
    prm = params()
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    fine = h2.solve(*(a[:, :1] for a in two), param=params(stop_tol=1e-8, max_iter=199950))
    no_bump(h2)
    assert fine["status"] == ["OPTIMAL"]
    rough = h2.solve(*(a[:, 1:2] for a in two), param=params(stop_tol=1e-2))
    X0, Y0 = np.full((lp["n"], 4), GARBAGE), np.full((lp["m"], 4), GARBAGE)
    X0[:, 0], Y0[:, 0] = fine["x"][:, 0], fine["y"][:, 0]
    X0[:, 1], Y0[:, 1] = rough["x"][:, 0], rough["y"][:, 0]
    out = h.solve_stream(*args, width=2, X0=X0, Y0=Y0, parent=parent)
    no_bump(h, streamed=True)
    assert out["status"] == ["OPTIMAL"] * 4 and list(out["iter"][[0, 2, 3]]) == [0, 0, 0] and out["iter"][1] > 0
    assert list(out["slot"]) == [0, 1, 0, 0] and list(out["event_in"]) == [0, 0, 0, 0] and list(out["event_out"][[0, 2, 3]]) == [0, 0, 0]
    check_against_references(h2, args, out, 2, prm, parent, X0, Y0)
    info, _ = check_record(h, out, 2, parent, X0)
    assert info["refill_passes"] == 2 and info["refills"] == 2 and info["refill_evaluations"] == 1
    h.close(); h2.close(); model.free()


# ---- 4. detection -------------------------------------------------------------------------------------------------------------------
def test_a_verdict_and_the_child_that_starts_from_its_iterate(gpu):
    """A chain of three: the middle one is infeasible by its bounds -- the variables of one row are fixed so that the row's activity
    exceeds its upper side -- and ends with a verdict and the reference batch's certificate; its child, the root's LP again, still
    runs, from the verdict's iterate."""
    lp = planted()
    one = make_batch(lp, 1, 2)
    Cm, AL, AU, L, U = (np.concatenate([a] * 3, axis=1) for a in one)
    rp, ci, val = np.asarray(lp["rowptr"]), np.asarray(lp["colind"]), np.asarray(lp["values"], dtype=float)
    for i in range(lp["m"]):
        cols, a = ci[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
        hi = np.where(a > 0, U[cols, 1], L[cols, 1])   # the row's largest activity within the bounds
        if np.isfinite(AU[i, 1]) and (a > 0).any() and a @ hi > AU[i, 1] + 5.0:
            L[cols, 1] = U[cols, 1] = hi
            break
    else:
        raise AssertionError("no row to make infeasible")
    args, parent = (Cm, AL, AU, L, U), np.array([-1, 0, 1])
    model = model_of(lp)
    prm = params(max_iter=30000)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out = h.solve_stream(*args, width=2, parent=parent, eps_primal=1e-8, eps_dual=1e-8)
    no_bump(h, streamed=True)
    print("statuses", out["status"], "iter", list(out["iter"]))
    assert out["status"] == ["OPTIMAL", "PRIMAL_INFEASIBLE", "OPTIMAL"] and int(out["certificates"]["kind"][1]) == 1
    assert out["iter"][2] > 0 and out["event_in"][2] == out["event_out"][1]
    check_against_references(h2, args, out, 2, prm, parent, detect=1e-8)
    check_record(h, out, 2, parent)
    h.close(); h2.close(); model.free()


# ---- 6. parent all -1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("started", [False, True], ids=["cold", "started"])
def test_all_roots_is_the_stream_without_parents(gpu, started):
    lp = planted()
    N, width = 10, 4
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    X0, Y0 = root_starts(h2, lp, args, np.full(N, -1)) if started else (None, None)
    out = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, parent=np.full(N, -1))
    ref = h2.solve_stream(*args, width=width, X0=X0, Y0=Y0)
    no_bump(h, streamed=True); no_bump(h2, streamed=True)
    same_stream(out, ref, "all roots")
    assert h.stream_info() == h2.stream_info()
    assert h.stream_parents_info() == dict(roots=N, cold_members=0 if started else N, children_started=0, idle_slot_events=0)
    with pytest.raises(RuntimeError, match="not a parents call"):
        h2.stream_parents_info()
    h.close(); h2.close(); model.free()


# ---- 7. twins -----------------------------------------------------------------------------------------------------------------------
def raw_device_call(h, args, width, parent, prm, X0=None, Y0=None):
    """hprlp_batched_solver_solve_stream_parents_device itself, with x, y, z buffers filled with NaN before the call."""
    torch = torch_()
    n, m, N = args[0].shape[0], args[1].shape[0], args[0].shape[1]
    keep = [T(a).T.contiguous() for a in args] + [None if v is None else T(v).T.contiguous() for v in (X0, Y0)]
    ptr = lambda t: None if t is None else t.data_ptr()
    xb, yb, zb = (torch.full((N, rows), float("nan"), dtype=torch.float64, device="cuda") for rows in (n, m, n))
    res = dict(primal_obj=np.zeros(N), residuals=np.zeros(N), gap=np.zeros(N), iter=np.zeros(N, dtype=np.intc))
    status = C.create_string_buffer(64 * N)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    sc = hprlp.CBatchedScalars(primal_obj=dp(res["primal_obj"]), residuals=dp(res["residuals"]), gap=dp(res["gap"]),
                               iter=res["iter"].ctypes.data_as(C.POINTER(C.c_int)), status=C.cast(status, C.POINTER(C.c_char)))
    par = np.ascontiguousarray(parent, dtype=np.intc)
    cprm = prm.to_c()
    torch.cuda.synchronize()
    rc = hprlp.lib().hprlp_batched_solver_solve_stream_parents_device(
        h._h, N, width, *(ptr(t) for t in keep[:5]), None, C.byref(cprm), ptr(keep[5]), ptr(keep[6]),
        par.ctypes.data_as(C.POINTER(C.c_int)), None, None, torch.cuda.current_stream().cuda_stream, xb.data_ptr(), yb.data_ptr(),
        zb.data_ptr(), C.byref(sc))
    assert rc == 0, hprlp.last_error()
    out = dict(res, x=xb.T.cpu().numpy(), y=yb.T.cpu().numpy(), z=zb.T.cpu().numpy())
    out["status"] = [status.raw[64 * k:64 * (k + 1)].split(b"\0")[0].decode() for k in range(N)]
    rec = [np.zeros(N, dtype=np.intc) for _ in range(3)]
    assert hprlp.lib().hprlp_batched_solver_stream_record(h._h, *(r.ctypes.data_as(C.POINTER(C.c_int)) for r in rec)) == N
    out["slot"], out["event_in"], out["event_out"] = rec
    return out


@pytest.mark.parametrize("case", ["chains", "chains_started", "tree"])
def test_the_device_entry_equals_the_host_entry(gpu, case):
    model = model_of(planted())
    if case == "tree":
        prm, width = params(stop_tol=1e-4, max_iter=15000), 4
        h2 = hprlp.BatchedSolver(model, prm)
        lp, args, parent = tree_queue(h2, prm)
        X0 = Y0 = None
    else:
        prm, width = params(stop_tol=1e-4), 12
        h2 = hprlp.BatchedSolver(model, prm)
        lp, args, parent = chains(5, 4)
        X0, Y0 = root_starts(h2, lp, args, parent) if case == "chains_started" else (None, None)
    h2.close()
    h = tree_handle(model, prm)
    ref = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, parent=parent)
    ref_info, ref_pinfo, ref_sc = h.stream_info(), h.stream_parents_info(), scalars_answer(h)
    assert isinstance(ref_sc, str)   # (scalars() is refused after a stream call)
    got = on_host(h.solve_stream_tensors(*[T(a) for a in args], width=width, X0=T(X0), Y0=T(Y0), parent=parent))
    no_bump(h, streamed=True)
    same_stream(got, ref, case)
    assert h.stream_info() == ref_info and h.stream_parents_info() == ref_pinfo and scalars_answer(h) == ref_sc
    raw = raw_device_call(h, args, width, parent, prm, X0, Y0)   # ... and into buffers that held NaN
    same_stream(raw, ref, case + " (NaN-filled buffers)")
    N = len(parent)
    late = raw_device_call(h, args, width, parent, params(stop_tol=1e-4, time_limit=0.0), X0, Y0)
    assert late["status"] == ["TIME_LIMIT"] * N and not late["iter"].any() and list(late["event_in"]) == [-1] * N
    assert list(late["slot"]) == [-1] * N
    for f in ("x", "y", "z"):
        assert not late[f].any() and np.isfinite(late[f]).all(), f
    host_late = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, parent=parent, prm=params(stop_tol=1e-4, time_limit=0.0))
    same_stream(late, host_late, case + " (time limit 0)")
    h.close(); model.free()


# ---- 8. handle hygiene --------------------------------------------------------------------------------------------------------------
def test_the_handle_after_a_parents_call(gpu):
    lp, args, parent = chains(5, 4)
    width = 8
    first = tuple(a[:, :width] for a in args)
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    h, never = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out1 = h.solve_stream(*args, width=width, parent=parent)
    captures = h.info()["graph_captures"]
    alive = h.info()["graphs_alive"]
    assert captures > 0
    out2 = h.solve_stream(*args, width=width, parent=parent)
    no_bump(h, streamed=True)
    assert h.info()["graph_captures"] == captures and h.info()["graphs_alive"] == alive   # (no panel moved)
    same_stream(out1, out2, "twice")
    for refused in (lambda: h.solve(*first, carry=True), lambda: h.ray_step(restart=True), lambda: h.get_panel("X_bar")):
        with pytest.raises(RuntimeError, match="streamed"):
            refused()
    same = lambda g, w, tag: same_stream(g, w, tag, record=False)
    same(h.solve(*first), never.solve(*first), "plain")
    same(h.solve_stream(*args, width=width), never.solve_stream(*args, width=width), "old stream")
    # The graphs are kept by run length: a plain solve and a plain stream place their check iterations differently and may capture
    # lengths the parents call never ran.  What must hold is that no call DROPPED a graph -- every capture of the handle's life is
    # alive -- and that the parents call, once more, finds all of its own.
    info = h.info()
    assert alive == captures and info["graphs_alive"] == info["graph_captures"] >= captures, (info, captures, alive)
    out3 = h.solve_stream(*args, width=width, parent=parent)
    same_stream(out1, out3, "after a plain solve and a plain stream")
    assert h.info()["graph_captures"] == info["graph_captures"] and h.info()["graphs_alive"] == info["graphs_alive"]
    # a refused call is followed by a valid carry of the solve before it
    want = [never.solve(*first), never.solve(*first, carry=True)]
    for refuse in ("parent", "nan"):
        got = h.solve(*first)
        before = h.info()
        if refuse == "parent":
            bad = parent.copy()
            bad[7] = 9
            with pytest.raises(RuntimeError, match=r"parent\[7\] = 9"):
                h.solve_stream(*args, width=width, parent=bad)
        else:   # a NaN in X0 of a root past W, in the device entry: found by the norm passes before any panel is written
            lp2, args2, parent2 = chains(10, 2)
            X0, Y0 = np.zeros((lp["n"], 20)), np.zeros((lp["m"], 20))
            X0[17, 9] = np.nan
            with pytest.raises(RuntimeError, match="not finite"):
                h.solve_stream_tensors(*[T(a) for a in args2], width=width, X0=T(X0), Y0=T(Y0), parent=parent2)
        assert h.info() == before
        same(got, want[0], "before the refusal: " + refuse)
        same(h.solve(*first, carry=True), want[1], "carry after the refusal: " + refuse)
    no_bump(h); no_bump(never)
    h.close(); never.close(); model.free()
