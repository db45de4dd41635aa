"""Streamed batches on the GPU (include/hprlp_amd.h hprlp_batched_solver_solve_stream, DESIGN.md "Streamed batches"): N problems
over one matrix through `width` slots, a finished member's slot taking the next queued problem at the same evaluation.

What is held: for a problem p that sat in slot k, status, iter, x, y, z, primal_obj, residuals, gap and certificate are BIT FOR
BIT those of a plain BatchedSolver.solve() of min(width, N) members whose slot k holds p -- the reference batches are built from
the stream's own record (batch g holds, in slot k, the g-th problem that occupied slot k) and solved on a second handle -- on
every kernel form of the half-steps; and the record itself is the schedule hprlp.stream_schedule() gives for the GPU's own
iteration counts.  Every comparison is made under "no lambda bump" on either side, which every test asserts
(BatchedSolver.lambda_max(), stream_info()["lambda_bumps"]).

All cases but the detection's run on the planted 300 x 400 network LP of tests/test_gpu_warm.py with make_batch(lp, N, 2) and
use_CR_scaling off (the CPU oracle solves all 192 members of that recipe OPTIMAL without a bump at 1e-4, 600 to 3 150
iterations, and the first 24 at 1e-6, 2 100 to 9 750)."""
import functools
import os

import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_batched_detect import MIXED_PRM, _mixed
from test_gpu_detect import model_of
from test_gpu_warm import make_batch

pytestmark = pytest.mark.gpu
CHECK = 150
SCALARS = ("primal_obj", "residuals", "gap")
CERT_SCALARS = ("kind", "iter", "objective", "violation")


@functools.lru_cache(maxsize=None)
def planted():
    return lpgen.planted_lp(300, 400, 2400, 7, values="network")


def params(**kw):
    return hprlp.Parameters(**dict(dict(stop_tol=1e-6, max_iter=45000, use_presolve=False, use_CR_scaling=False), **kw))


def no_bump(h, streamed=False):
    created, last = h.lambda_max()
    assert created == last, (created, last)
    if streamed:
        assert h.stream_info()["lambda_bumps"] == 0


def slot_lists(out, W):
    """The problems that occupied each slot, in order (a problem that never started sits in none)."""
    lists = [[] for _ in range(W)]
    for p in np.argsort(out["event_in"], kind="stable"):
        if out["event_in"][p] >= 0:
            lists[out["slot"][p]].append(int(p))
    for k, lst in enumerate(lists):
        assert lst == sorted(lst) and all(out["event_out"][a] == out["event_in"][b] for a, b in zip(lst[:-1], lst[1:])), (k, lst)
    return lists


def cert_column(cert, f, p):
    return None if cert[f] is None else cert[f][:, p]


def check_against_reference_batches(h2, args, out, width, prm, X0=None, Y0=None, detect=None):
    """Batch g holds in slot k the g-th problem that occupied slot k (any other problem where there is none: problem 0); solved by
    plain solve() on h2.  Returns the largest iter of each batch's own members."""
    N = args[0].shape[1]
    W = min(width, N)
    lists = slot_lists(out, W)
    largest = []
    for g in range(max(len(lst) for lst in lists)):
        idx = np.array([lst[g] if g < len(lst) else 0 for lst in lists])
        real = [k for k, lst in enumerate(lists) if g < len(lst)]
        kw = dict(param=prm)
        if X0 is not None:
            kw.update(X0=X0[:, idx])
        if Y0 is not None:
            kw.update(Y0=Y0[:, idx])
        if detect is not None:
            kw.update(eps_primal=detect, eps_dual=detect)
        ref = h2.solve(*(a[:, idx] for a in args), **kw)
        no_bump(h2)
        for k in real:
            p = idx[k]
            assert out["status"][p] == ref["status"][k] and out["iter"][p] == ref["iter"][k], \
                (p, g, k, out["status"][p], ref["status"][k], out["iter"][p], ref["iter"][k])
            for f in ("x", "y", "z"):
                assert np.array_equal(out[f][:, p], ref[f][:, k]), (f, p, g, k)
            for f in SCALARS:
                assert out[f][p] == ref[f][k], (f, p, g, k, out[f][p], ref[f][k])
            if detect is not None:
                co, cr = out["certificates"], ref["certificates"]
                for f in CERT_SCALARS:
                    assert co[f][p] == cr[f][k], (f, p, g, k)
                for f in ("y", "z", "d"):
                    a, b = cert_column(co, f, p), cert_column(cr, f, k)
                    if a is None or b is None:   # (no member of the call has a ray of this kind: the member's is zero on the other side)
                        assert (a is None or not a.any()) and (b is None or not b.any()), (f, p, g, k)
                    else:
                        assert np.array_equal(a, b), (f, p, g, k)
        largest.append(int(max(ref["iter"][k] for k in real)))
    return largest


def check_record(h, out, width, largest, check_iter=CHECK):
    """The record is the schedule of the GPU's own iteration counts; the loop is as long as that schedule and no longer than the
    reference batches one after the other."""
    assert (out["iter"] % check_iter == 0).all()
    slot, ein, eout = hprlp.stream_schedule(out["iter"] // check_iter, width)
    assert np.array_equal(out["slot"], slot) and np.array_equal(out["event_in"], ein) and np.array_equal(out["event_out"], eout)
    info = h.stream_info()
    assert info["count"] == len(out["iter"]) and info["width"] == width
    assert info["loop_iterations"] == int(eout.max()) * check_iter
    assert info["loop_iterations"] <= sum(largest), (info, largest)
    assert info["refills"] == max(len(out["iter"]) - width, 0)
    assert info["evaluations"] == int(eout.max()) + 1
    return info


# ---- 1. bits, per kernel form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,chunk,tol", [(3, 0, 1e-6), (12, 0, 1e-6), (64, 0, 1e-4), (70, 0, 1e-4), (70, 8, 1e-4)])
def test_stream_gives_the_bits_of_plain_batches(gpu, monkeypatch, width, chunk, tol):
    """width 3: kb_half; 12: kb_halfN<16>; 64: kb_half64; 70: two chunks of 64 with 58 dead columns; 70 with chunks of 8: kb_halfN<8>."""
    if chunk:
        monkeypatch.setenv("HPRLP_BATCH_CHUNK", str(chunk))
    lp = planted()
    N = 2 * width + width // 2
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params(stop_tol=tol)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out = h.solve_stream(*args, width=width)
    no_bump(h, streamed=True)
    geo = h.info()
    assert (geo["Bp"], geo["Bc"]) == {(3, 0): (4, 4), (12, 0): (16, 16), (64, 0): (64, 64), (70, 0): (128, 64), (70, 8): (128, 8)}[(width, chunk)]
    assert out["status"] == ["OPTIMAL"] * N and out["x"].shape == (lp["n"], N)
    largest = check_against_reference_batches(h2, args, out, width, prm)
    info = check_record(h, out, width, largest)
    print("width", width, "chunk", chunk, "loop iterations", info["loop_iterations"], "batches", largest, sum(largest), "refill evaluations",
          info["refill_evaluations"], "passes", info["refill_passes"])
    assert (out["event_in"][:width] == 0).all() and (out["event_in"][width:] > 0).all()
    h.close(); h2.close(); model.free()


# ---- 2. starts and the cascade --------------------------------------------------------------------------------------------------
def test_starts_and_a_slot_handed_on_twice_within_one_event(gpu):
    lp = planted()
    N, width = 6, 4
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params()
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    fine = h2.solve(*args, param=params(stop_tol=1e-8, max_iter=199950))
    assert fine["status"] == ["OPTIMAL"] * N
    no_bump(h2)
    X0, Y0 = np.zeros((lp["n"], N)), np.zeros((lp["m"], N))
    for p in (0, 4):
        X0[:, p], Y0[:, p] = fine["x"][:, p], fine["y"][:, p]
    out = h.solve_stream(*args, width=width, X0=X0, Y0=Y0)
    no_bump(h, streamed=True)
    assert out["status"] == ["OPTIMAL"] * N
    assert out["iter"][0] == 0 and out["iter"][4] == 0 and (out["iter"][[1, 2, 3, 5]] > 0).all()
    rec = lambda p: (int(out["slot"][p]), int(out["event_in"][p]), int(out["event_out"][p]))
    assert rec(0) == (0, 0, 0) and rec(4) == (0, 0, 0), (rec(0), rec(4))
    assert rec(5)[:2] == (0, 0) and rec(5)[2] == out["iter"][5] // CHECK
    largest = check_against_reference_batches(h2, args, out, width, prm, X0, Y0)
    info = check_record(h, out, width, largest)
    assert len(largest) == 3   # (slot 0 held three problems)
    two = [max(out["iter"][:4]), max(out["iter"][4:])]
    assert info["loop_iterations"] < sum(two), (info, two)
    assert info["refill_passes"] == 2 and info["refill_evaluations"] == 1
    h.close(); h2.close(); model.free()


@pytest.mark.parametrize("which", ["x", "y"])
def test_a_start_for_one_side_only(gpu, which):
    """Only X0 or only Y0: the refill zeroes the other side's panel column (kb_slot_clear) and the masked start kernels seed from it."""
    lp = planted()
    N, width = 7, 3
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    rough = h2.solve(*args, param=params(stop_tol=1e-2))   # (a point on the way: a start that is neither zero nor a solution)
    no_bump(h2)
    X0, Y0 = (rough["x"], None) if which == "x" else (None, rough["y"])
    out = h.solve_stream(*args, width=width, X0=X0, Y0=Y0)
    no_bump(h, streamed=True)
    assert out["status"] == ["OPTIMAL"] * N and (out["iter"] > 0).all()
    largest = check_against_reference_batches(h2, args, out, width, prm, X0, Y0)
    check_record(h, out, width, largest)
    assert h.stream_info()["refills"] == N - width
    cold = h.solve_stream(*args, width=width)
    assert not np.array_equal(cold["iter"], out["iter"]) or not np.array_equal(cold["x"], out["x"])   # (the start was used)
    h.close(); h2.close(); model.free()


@pytest.mark.parametrize("width", (5, 8))
def test_count_at_most_width_is_the_plain_solve(gpu, width):
    lp = planted()
    N = 5
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out = h.solve_stream(*args, width=width)
    ref = h2.solve(*args)
    no_bump(h, streamed=True); no_bump(h2)
    assert h.info()["Bp"] == h2.info()["Bp"] == 8
    assert out["status"] == ref["status"] and np.array_equal(out["iter"], ref["iter"])
    for f in ("x", "y", "z") + SCALARS:
        assert np.array_equal(out[f], ref[f]), f
    info = h.stream_info()
    assert info["refills"] == 0 and info["refill_passes"] == 0 and info["loop_iterations"] == int(ref["iter"].max())
    assert list(out["slot"]) == list(range(N)) and not out["event_in"].any() and np.array_equal(out["event_out"] * CHECK, ref["iter"])
    h.close(); h2.close(); model.free()


# ---- 3. detection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,N", [(8, 20), (64, 96)])
def test_stream_with_detection_gives_the_reference_batches_certificates(gpu, width, N):
    members, model, args = _mixed(N)
    prm = hprlp.Parameters(**MIXED_PRM)
    assert prm.max_iter % CHECK == 0
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out = h.solve_stream(*args, width=width, eps_primal=1e-8, eps_dual=1e-8)
    no_bump(h, streamed=True)
    assert out["status"] == [s for _, s in members]
    largest = check_against_reference_batches(h2, args, out, width, prm, detect=1e-8)
    check_record(h, out, width, largest)
    cert = out["certificates"]
    assert [int(k) for k in cert["kind"]] == [{"OPTIMAL": 0, "PRIMAL_INFEASIBLE": 1, "DUAL_INFEASIBLE": 2}[s] for _, s in members]
    lists = slot_lists(out, width)
    followed = [lst[i] for lst in lists for i in range(len(lst) - 1) if cert["kind"][lst[i]] != 0]
    assert followed, "no member with a verdict had a successor in its slot"
    h.close(); h2.close(); model.free()


def test_stream_with_starts_and_detection(gpu):
    """Starts and detection together: the refill seeds the new members and clears their ray panels in the same pass."""
    width, N = 8, 20
    members, model, args = _mixed(N)
    prm = hprlp.Parameters(**MIXED_PRM)
    rng = np.random.default_rng(11)
    X0, Y0 = 0.1 * rng.normal(size=args[0].shape), 0.1 * rng.normal(size=args[1].shape)
    h, h2 = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, eps_primal=1e-8, eps_dual=1e-8)
    no_bump(h, streamed=True)
    assert {"PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL"} <= set(out["status"])
    largest = check_against_reference_batches(h2, args, out, width, prm, X0, Y0, detect=1e-8)
    check_record(h, out, width, largest)
    assert h.stream_info()["refills"] == N - width
    h.close(); h2.close(); model.free()


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------
def test_limits_and_the_refused_max_iter(gpu):
    lp = planted()
    N, width = 10, 4
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    prm = params()
    h = hprlp.BatchedSolver(model, prm)
    # every member runs into its own iteration limit, the late ones too
    out = h.solve_stream(*args, width=width, prm=params(max_iter=3 * CHECK))
    no_bump(h, streamed=True)
    assert out["status"] == ["ITER_LIMIT"] * N and (out["iter"] == 3 * CHECK).all()
    assert list(out["event_in"]) == [0] * 4 + [3] * 4 + [6] * 2 and (out["event_out"] - out["event_in"] == 3).all()
    assert h.stream_info()["loop_iterations"] == 9 * CHECK
    h2 = hprlp.BatchedSolver(model, prm)
    largest = check_against_reference_batches(h2, args, out, width, params(max_iter=3 * CHECK))
    assert largest == [3 * CHECK] * 3
    # the call's time limit
    out = h.solve_stream(*args, width=width, prm=params(time_limit=0.0))
    no_bump(h, streamed=True)
    assert out["status"] == ["TIME_LIMIT"] * N and not out["iter"].any()
    assert list(out["event_in"]) == [0] * 4 + [-1] * 6 and list(out["slot"][4:]) == [-1] * 6
    for f in ("x", "y", "z"):
        assert not out[f].any(), f
    # a max_iter between two events is refused, and the handle is as it was
    plain = h.solve(*(a[:, :4] for a in args))
    before = h.info()
    with pytest.raises(RuntimeError, match="multiple of check_iter"):
        h.solve_stream(*args, width=width, prm=params(max_iter=3 * CHECK + 1))
    assert h.info() == before
    carried = h.solve(*(a[:, :4] for a in args), carry=True)   # (the previous solve is still there to be carried)
    fresh = hprlp.BatchedSolver(model, prm)
    want = fresh.solve(*(a[:, :4] for a in args))
    want_carried = fresh.solve(*(a[:, :4] for a in args), carry=True)
    for got, ref in ((plain, want), (carried, want_carried), (h.solve(*(a[:, :4] for a in args)), want)):
        assert got["status"] == ref["status"] and np.array_equal(got["iter"], ref["iter"])
        for f in ("x", "y", "z") + SCALARS:
            assert np.array_equal(got[f], ref[f]), f
    with pytest.raises(RuntimeError, match="not finite"):
        h.solve_stream(*args, width=width, X0=np.full((lp["n"], N), np.nan))
    h.close(); h2.close(); fresh.close(); model.free()


# ---- 5. neighbours --------------------------------------------------------------------------------------------------------------
def test_plain_solves_after_a_stream_and_the_graphs(gpu):
    lp = planted()
    N, width = 20, 8
    args = make_batch(lp, N, 2)
    first = tuple(a[:, :width] for a in args)
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    h, never = hprlp.BatchedSolver(model, prm), hprlp.BatchedSolver(model, prm)
    out1 = h.solve_stream(*args, width=width)
    captures = h.info()["graph_captures"]
    assert captures > 0
    out2 = h.solve_stream(*args, width=width)
    no_bump(h, streamed=True)
    assert h.info()["graph_captures"] == captures   # (no panel moved: the captured graphs survive every refill and the next call)
    assert out1["status"] == out2["status"] and np.array_equal(out1["iter"], out2["iter"])
    for f in ("x", "y", "z", "slot", "event_in", "event_out") + SCALARS:
        assert np.array_equal(out1[f], out2[f]), f
    for refused in (lambda: h.solve(*first, carry=True), lambda: h.ray_step(restart=True), lambda: h.get_panel("X_bar")):
        with pytest.raises(RuntimeError, match="streamed"):
            refused()
    got = [h.solve(*first), h.solve(*first, carry=True)]
    want = [never.solve(*first), never.solve(*first, carry=True)]
    no_bump(h); no_bump(never)
    for g, w in zip(got, want):
        assert g["status"] == w["status"] and np.array_equal(g["iter"], w["iter"])
        for f in ("x", "y", "z") + SCALARS:
            assert np.array_equal(g[f], w[f]), f
    assert np.array_equal(h.get_panel("X_bar"), never.get_panel("X_bar"))
    h.close(); never.close(); model.free()


def test_the_three_entries_on_one_handle(gpu):
    """Stream, device entry, stream with detection (it allocates the ray panels and Zray), host entry, carry: the staging blocks,
    the workspace steps and the bookkeeping are shared by the three entries, and each call gives the bits of the same single call
    on a fresh handle (the carry: of the same pair of calls).  The geometry never changes: nothing is captured after the first call."""
    from test_gpu_batched_device import T, on_host
    lp = planted()
    N, width = 10, 4
    args = make_batch(lp, N, 2)
    first = tuple(a[:, :width] for a in args)
    model = model_of(lp)
    prm = params(stop_tol=1e-4, check_iter=CHECK)
    fresh = lambda: hprlp.BatchedSolver(model, prm)

    def same(got, ref, tag, streamed=False):
        assert got["status"] == ref["status"] and np.array_equal(got["iter"], ref["iter"]), (tag, got["status"], got["iter"], ref["iter"])
        for f in ("x", "y", "z") + SCALARS + (("slot", "event_in", "event_out") if streamed else ()):
            assert np.array_equal(got[f], ref[f]), (tag, f)

    h = fresh()
    # 1. a stream of the 10
    got = h.solve_stream(*args, width=width)
    no_bump(h, streamed=True)
    captures = h.info()["graph_captures"]
    assert captures > 0 and got["status"] == ["OPTIMAL"] * N
    f1 = fresh()
    ref_stream = f1.solve_stream(*args, width=width)
    no_bump(f1, streamed=True)
    same(got, ref_stream, "stream", streamed=True)
    # 2. the device entry, the first 4
    got = on_host(h.solve_tensors(*[T(a) for a in first]))
    no_bump(h)
    f2 = fresh()
    same(got, on_host(f2.solve_tensors(*[T(a) for a in first])), "tensors")
    no_bump(f2)
    # 3. a stream with detection on
    got = h.solve_stream(*args, width=width, eps_primal=1e-8, eps_dual=1e-8)
    no_bump(h, streamed=True)
    f3 = fresh()
    ref = f3.solve_stream(*args, width=width, eps_primal=1e-8, eps_dual=1e-8)
    no_bump(f3, streamed=True)
    same(got, ref, "stream with detection", streamed=True)
    assert [int(k) for k in got["certificates"]["kind"]] == [int(k) for k in ref["certificates"]["kind"]] == [0] * N
    # 4. the host entry, the first 4
    got = h.solve(*first)
    no_bump(h)
    assert h.info()["graph_captures"] == captures
    f4 = fresh()
    same(got, f4.solve(*first), "host")
    no_bump(f4)
    # 5. ... and their carry
    got = h.solve(*first, carry=True)
    no_bump(h)
    same(got, f4.solve(*first, carry=True), "carry")
    no_bump(f4)
    for s in (h, f1, f2, f3, f4):
        s.close()
    model.free()
