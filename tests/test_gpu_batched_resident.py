"""The resident batched solver (GPU): hprlp.BatchedSolver / hprlp_batched_solver_* (DESIGN.md "Resident batches").

The reference of every test is a FRESH solve_batched / solve_batched_detect / solve_batched_warm call with the same arguments,
and equality means: the same status and iter of every member, np.array_equal on x, y, z, and == on primal_obj, residuals and
gap.  Nothing else is owed a tolerance: the handle runs the same functions on the same inputs, and its new kernels (kb_panel_in,
kb_panel_out, kb_carry_start) are elementwise.  This rests on one assumption, checked first: two fresh solvers on one matrix get
the same lambda_max bits (fixed-order reductions, counter RNG start) -- test_two_fresh_calls_agree.

The LPs: matrix("long") / batch("long") of tests/test_gpu_batched_kernels.py (123 x 205; B = 3 -> kb_half, 12 -> kb_halfN<16>,
64 -> kb_half64, 70 -> two chunks of 64 with 58 dead columns), the 300 x 400 planted network LP of tests/test_gpu_warm.py at
B = 8, and the mixed batch of tests/test_gpu_batched_detect.py (infeasible, unbounded and solvable members on one matrix).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_batched_kernels import BUMP_B, BUMP_CHECK_ITER, batch, bump_case
from test_gpu_batched_detect import MIXED_PRM, _mixed
from test_gpu_warm import make_batch, model_of

pytestmark = pytest.mark.gpu

# runs through restarts (check_iter = 150 < max_iter), nobody ends early
LONG_PRM = dict(use_CR_scaling=False, check_iter=150, max_iter=451, stop_tol=1e-12, use_presolve=False)
SCALARS = ("primal_obj", "residuals", "gap")


def long_model():
    b = batch("long")
    z = np.zeros
    return hprlp.Model.from_csr(b["m"], b["n"], b["rowptr"], b["colind"], b["values"], z(b["m"]), z(b["m"]), z(b["n"]), z(b["n"]), z(b["n"]))


def long_args(B, off=0):
    """Members off .. off + B - 1 of batch("long"): (C, AL, AU, L, U), obj_constants."""
    b = batch("long")
    s = slice(off, off + B)
    return (b["C"][:, s], b["AL"][:, s], b["AU"][:, s], b["L"][:, s], b["U"][:, s]), b["objc"][s]


def assert_same(got, ref, tag):
    assert got["x"] is not None and ref["x"] is not None, (tag, hprlp.last_error())
    assert got["batch_size"] == ref["batch_size"], tag
    assert got["status"] == ref["status"], (tag, got["status"], ref["status"])
    assert list(got["iter"]) == list(ref["iter"]), (tag, list(got["iter"]), list(ref["iter"]))
    for f in ("x", "y", "z"):
        bad = np.argwhere(got[f] != ref[f])
        assert np.array_equal(got[f], ref[f]), (tag, f, "first (index, member):", bad[0].tolist(), "of", len(bad))
    for f in SCALARS:
        assert (got[f] == ref[f]).all(), (tag, f, got[f], ref[f])


def fresh(model, args, objc, prm, X0=None, Y0=None, eps=None):
    return hprlp.solve_batched_warm(model, *args, X0, Y0, objc, prm, eps_primal=eps, eps_dual=eps)


def test_two_fresh_calls_agree(gpu):
    """The assumption under every test below: nothing in a fresh call (scaling, power iteration, loop) depends on the run."""
    model, prm = long_model(), hprlp.Parameters(**LONG_PRM)
    args, objc = long_args(12)
    assert_same(fresh(model, args, objc, prm), fresh(model, args, objc, prm), "fresh twice")
    model.free()


def test_a_batch_does_not_depend_on_the_handles_history(gpu):
    model, prm = long_model(), hprlp.Parameters(**LONG_PRM)
    h = hprlp.BatchedSolver(model, prm)
    earlier = None
    # (B, first member, started from the first call's result)
    for step, (B, off, warm) in enumerate([(12, 0, False), (70, 0, False), (12, 3, True), (64, 1, False), (3, 0, False), (64, 0, False)]):
        args, objc = long_args(B, off)
        X0, Y0 = (earlier["x"], earlier["y"]) if warm else (None, None)
        got = h.solve(*args, objc, X0=X0, Y0=Y0)
        assert_same(got, fresh(model, args, objc, prm, X0, Y0), ("step", step, "B", B))
        assert got["status"] == ["ITER_LIMIT"] * B and got["power_time"] == 0.0
        assert got["time"] == pytest.approx(got["setup_time"] + got["solve_time"])
        if earlier is None:
            earlier = got
    info = h.info()
    assert (info["m"], info["n"], info["solves"], info["Bp"], info["Bc"]) == (123, 205, 6, 64, 64), info
    sec = h.seconds()
    assert all(v >= 0.0 for v in sec.values()) and sec["loop"] > 0.0 and sec["create_setup"] > 0.0, sec
    h.close(); model.free()


def test_the_workspace_and_the_graphs_stay_while_the_geometry_does(gpu):
    model = long_model()
    h = hprlp.BatchedSolver(model, hprlp.Parameters(**LONG_PRM))
    seen = []
    for B in (12, 70, 64, 64):
        args, objc = long_args(B)
        h.solve(*args, objc)
        seen.append(h.info())
    print("info per call", seen)
    a12, a70, a64, b64 = seen
    assert a12["graph_captures"] > 0 and a12["panel_allocations"] > 0
    assert a70["graph_captures"] > a12["graph_captures"] and a70["panel_allocations"] > a12["panel_allocations"]
    assert (a70["Bp"], a70["Bc"], a64["Bp"], a64["Bc"]) == (128, 64, 64, 64)
    assert b64["graph_captures"] == a64["graph_captures"] and b64["panel_allocations"] == a64["panel_allocations"]
    assert b64["graphs_alive"] == a64["graphs_alive"] > 0 and b64["solves"] == 4
    h.close(); model.free()


def test_carry_equals_the_explicit_start_on_the_planted_lp(gpu):
    lp = lpgen.planted_lp(300, 400, 2400, 7, values="network")
    B = 8
    args = make_batch(lp, B, 2)
    model = model_of(lp)
    prm = hprlp.Parameters(stop_tol=1e-6, max_iter=50000, use_presolve=False)
    h = hprlp.BatchedSolver(model, prm)
    r0 = h.solve(*args)
    assert r0["status"] == ["OPTIMAL"] * B
    assert_same(r0, fresh(model, args, None, prm), "cold")
    C2 = args[0] * (1 + 1e-3 * np.random.default_rng(40).normal(size=args[0].shape))
    args2 = (C2,) + tuple(args[1:])
    warm = h.solve(*args2, carry=True)
    assert_same(warm, fresh(model, args2, None, prm, r0["x"], r0["y"]), "carry")
    cold = h.solve(*args2)  # (a cold call after a carried one: the start panels are zero again)
    assert_same(cold, fresh(model, args2, None, prm), "cold after carry")
    # not asserted: DESIGN.md "Warm start" records that a warm start does not always help
    print("planted LP, C changed by 1e-3: cold iterations", list(cold["iter"]), "carried", list(warm["iter"]))
    h.close(); model.free()


def test_carry_equals_the_explicit_start_with_dead_columns(gpu):
    model, prm = long_model(), hprlp.Parameters(**LONG_PRM)
    h = hprlp.BatchedSolver(model, prm)
    B = 70
    args, objc = long_args(B)
    r0 = h.solve(*args, objc)
    args2, objc2 = long_args(B, 60)  # other members' data: every vector and both scales change
    warm = h.solve(*args2, objc2, carry=True)
    assert_same(warm, fresh(model, args2, objc2, prm, r0["x"], r0["y"]), "carry B = 70")
    print("long, B = 70: iterations", sorted(set(warm["iter"])))
    h.close(); model.free()


def test_refused_calls_leave_the_handle_as_it_was(gpu):
    model, prm = long_model(), hprlp.Parameters(**LONG_PRM)
    h = hprlp.BatchedSolver(model, prm)
    B = 12
    args, objc = long_args(B)
    n, m = batch("long")["n"], batch("long")["m"]

    def refused(what, *a, **kw):
        with pytest.raises(RuntimeError) as e:
            h.solve(*a, **kw)
        msg = str(e.value).split("failed: ", 1)[1]
        print(what, "->", msg)
        assert len(msg) > 10, (what, msg)
        return msg

    assert "previous" in refused("carry on the first call", *args, objc, carry=True)
    r0 = h.solve(*args, objc)
    before = h.info()
    args5, objc5 = long_args(5)
    assert "batch_size" in refused("carry with another B", *args5, objc5, carry=True)
    assert "X0" in refused("carry with X0", *args, objc, X0=r0["x"], carry=True)
    empty = tuple(a[:, :0] for a in args)
    assert "positive" in refused("B = 0", *empty, objc[:0])
    bad = r0["x"].copy()
    bad[7, 3] = np.nan
    assert "X0" in refused("NaN in X0", *args, objc, X0=bad, Y0=r0["y"])
    # a NULL vector: through the C entry itself (the wrapper has no way to say NULL)
    P = lambda a: np.asfortranarray(a, dtype=np.float64).ctypes.data_as(hprlp.c_dbl_p)
    keep = [np.asfortranarray(a, dtype=np.float64) for a in args]
    res = hprlp.CBatchedResults()
    rc = hprlp.lib().hprlp_batched_solver_solve(h._h, B, keep[0].ctypes.data_as(hprlp.c_dbl_p), None, P(keep[2]), P(keep[3]), P(keep[4]),
                                                None, None, None, None, 0, None, None, C.byref(res))
    assert rc == -1 and "null" in hprlp.last_error(), hprlp.last_error()
    assert h.info() == before
    # the handle is as the last successful call left it: a carry from r0 still works and is the fresh warm call
    args2, objc2 = long_args(B, 20)
    got = h.solve(*args2, objc2, carry=True)
    assert_same(got, fresh(model, args2, objc2, prm, r0["x"], r0["y"]), "carry after the refusals")
    h.close(); model.free()


@pytest.mark.parametrize("graphs", ["graphs", "eager"])
def test_a_call_after_a_lambda_bump_starts_from_the_created_lambda(gpu, monkeypatch, graphs):
    """The bump case of tests/test_gpu_batched_kernels.py (a quarter of the true lambda: the oracle bumps it from iteration 10 on)
    twice on one handle: the second call equals the fresh one only if it started from the created lambda, with graphs that hold
    that lambda."""
    lam_small, at, K = bump_case()
    monkeypatch.setenv("HPRLP_BATCH_LAMBDA", float(lam_small).hex())
    if graphs == "eager":
        monkeypatch.setenv("HPRLP_NO_GRAPH", "1")
    model = long_model()
    prm = hprlp.Parameters(**dict(LONG_PRM, check_iter=BUMP_CHECK_ITER, max_iter=K))
    args, objc = long_args(BUMP_B)
    ref = fresh(model, args, objc, prm)
    h = hprlp.BatchedSolver(model, prm)
    first = h.solve(*args, objc)
    c1 = h.info()["graph_captures"]
    second = h.solve(*args, objc)
    c2 = h.info()["graph_captures"]
    assert_same(first, ref, (graphs, "first"))
    assert_same(second, ref, (graphs, "second"))
    print("bump", graphs, "oracle's first bump by iteration", at, "K", K, "captures", c1, c2)
    if graphs == "graphs":
        assert c2 > c1 > 0  # the first call's graphs held the bumped lambda: dropped, captured anew
    else:
        assert c1 == c2 == 0
    h.close(); model.free()


def test_the_hooks_are_read_at_every_call(gpu, monkeypatch):
    model, prm = long_model(), hprlp.Parameters(**LONG_PRM)
    h = hprlp.BatchedSolver(model, prm)

    def step(B, off, env, tag):
        args, objc = long_args(B, off)
        with monkeypatch.context() as mp:
            for k, v in env:
                mp.setenv(k, v)
            got = h.solve(*args, objc)
            ref = fresh(model, args, objc, prm)
        assert_same(got, ref, tag)
        return h.info()

    step(70, 0, (), "B = 70")
    i = step(70, 2, (("HPRLP_BATCH_CHUNK", "16"),), "B = 70, chunks of 16")
    assert (i["Bp"], i["Bc"]) == (128, 16), i
    i = step(70, 4, (), "B = 70 after the chunk hook")
    assert (i["Bp"], i["Bc"]) == (128, 64), i
    a = step(64, 0, (), "B = 64")
    b = step(64, 1, (("HPRLP_BATCH_GRID", "3"),), "B = 64, grid cap 3")
    c = step(64, 2, (), "B = 64 after the grid hook")
    # the cap changes the captured launches, not a buffer
    assert a["graph_captures"] < b["graph_captures"] < c["graph_captures"]
    assert a["panel_allocations"] == b["panel_allocations"] == c["panel_allocations"]
    h.close(); model.free()


def test_detection_off_on_off_on_one_handle(gpu):
    members, model, args = _mixed(5)
    prm = hprlp.Parameters(**MIXED_PRM)
    ref_off = fresh(model, args, None, prm)
    ref_on = fresh(model, args, None, prm, eps=1e-8)
    assert {"PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL"} <= set(ref_on["status"]), ref_on["status"]
    h = hprlp.BatchedSolver(model, prm)
    for step, on in enumerate((False, True, False)):
        got = h.solve(*args, eps_primal=1e-8 if on else None, eps_dual=1e-8 if on else None)
        ref = ref_on if on else ref_off
        assert_same(got, ref, ("detection", step, on))
        if on:
            gc, rc = got["certificates"], ref["certificates"]
            assert set(gc["kind"]) == {0, 1, 2}
            for f in ("kind", "iter", "objective", "violation", "y", "z", "d"):
                assert (gc[f] is None) == (rc[f] is None) and (gc[f] is None or np.array_equal(gc[f], rc[f])), f
        else:
            assert "certificates" not in got
    h.close(); model.free()
