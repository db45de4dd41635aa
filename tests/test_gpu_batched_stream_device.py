"""Device-resident streams on the GPU (include/hprlp_amd.h hprlp_batched_solver_solve_stream_device, DESIGN.md "Device-resident
streams"): BatchedSolver.solve_stream_tensors takes the queue as torch tensors on the GPU, never stages a scaled copy of it -- the
norms come from kb_data_in / kb_data_bc in their form without stores, over the caller's arrays, a problem is scaled by
kb_slot_scale on its way into a slot -- and writes x, y, z straight into the caller's buffers.

The reference of every comparison is the HOST stream (numpy in, numpy out) on a handle with set_norms(1), with the same arguments.
Equality means: the same status and iter of every problem, np.array_equal on x, y, z, == on primal_obj, residuals and gap, the same
record (slot, event_in, event_out), the same stream_info() counts -- lambda bumps included: both calls run the same arithmetic from
the created lambda -- and the same answer of scalars().  Nothing is owed a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import hprlp
from test_gpu_batched_detect import MIXED_PRM, _mixed
from test_gpu_batched_device import (T, _loaded_hip_runtime, few_rows_batch, few_rows_model, on_host, planted, segment_batch,
                                     segment_batch_all_infinities, segment_lp, torch_, tree_handle)
from test_gpu_batched_stream import CERT_SCALARS, CHECK, SCALARS, params
from test_gpu_warm import make_batch, model_of

pytestmark = pytest.mark.gpu
INF = np.inf
RECORD = ("slot", "event_in", "event_out")


def same_stream(got, ref, tag, record=True):
    assert got["status"] == ref["status"], (tag, got["status"], ref["status"])
    assert list(got["iter"]) == list(ref["iter"]), (tag, list(got["iter"]), list(ref["iter"]))
    for f in ("x", "y", "z"):
        bad = np.argwhere(got[f] != ref[f])
        assert np.array_equal(got[f], ref[f]), (tag, f, "first (index, problem):", bad[0].tolist(), "of", len(bad))
    for f in SCALARS + (RECORD if record else ()):
        assert np.array_equal(got[f], ref[f]), (tag, f, got[f], ref[f])


def scalars_answer(h):
    """What scalars() says after the call: the values, or its refusal's words."""
    try:
        return {k: v.tolist() for k, v in h.scalars().items()}
    except RuntimeError as e:
        return str(e)


def both(h, args, width, X0=None, Y0=None, **kw):
    """The host stream, then the device stream, on one tree-rule handle: (host result, device result on the host), with the record,
    the counts and scalars() compared."""
    ref = h.solve_stream(*args, width=width, X0=X0, Y0=Y0, **kw)
    ref_info, ref_sc = h.stream_info(), scalars_answer(h)
    got = on_host(h.solve_stream_tensors(*[T(a) for a in args], width=width, X0=T(X0), Y0=T(Y0), **kw))
    assert h.stream_info() == ref_info, (h.stream_info(), ref_info)
    assert scalars_answer(h) == ref_sc
    return ref, got, ref_info


@functools.lru_cache(maxsize=None)
def queue(N, W):
    """make_batch of the stream tests with infinite entries in AL, AU, l, u -- in late problems too -- and C = 0 in a problem that
    enters at a refill: the substitution and the sigma = 1 rule are met by kb_slot_scale and kb_data_header, not by the initial fill alone."""
    lp = planted()
    Cm, AL, AU, L, U = (np.array(a) for a in make_batch(lp, N, 2))
    AL[:4, :] = -INF
    AU[5:8, 1:] = INF
    L[10:13, :] = np.where(np.arange(N) % 2 == 0, -INF, L[10:13, :])
    U[:4, :] = INF
    Cm[:, W + 1] = 0.0
    for a in (AL[:, W:], AU[:, W:], L[:, W:], U[:, W:]):
        assert np.isinf(a).any()
    return Cm, AL, AU, L, U


# ---- 1. bits, per kernel form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,chunk,tol", [(3, 0, 1e-6), (12, 0, 1e-6), (64, 0, 1e-4), (70, 0, 1e-4), (70, 8, 1e-4)])
def test_device_stream_gives_the_bits_of_the_host_stream(gpu, monkeypatch, width, chunk, tol):
    """width 3: kb_half; 12: kb_halfN<16>; 64: kb_half64; 70: two chunks of 64 with 58 dead columns; 70 with chunks of 8: kb_halfN<8>."""
    if chunk:
        monkeypatch.setenv("HPRLP_BATCH_CHUNK", str(chunk))
    N = 2 * width + width // 2
    args = queue(N, width)
    model = model_of(planted())
    h = tree_handle(model, params(stop_tol=tol))
    ref, got, info = both(h, args, width)
    geo = h.info()
    assert (geo["Bp"], geo["Bc"]) == {(3, 0): (4, 4), (12, 0): (16, 16), (64, 0): (64, 64), (70, 0): (128, 64), (70, 8): (128, 8)}[(width, chunk)]
    print("width", width, "chunk", chunk, "statuses", sorted(set(ref["status"])), "iter", min(ref["iter"]), "..", max(ref["iter"]), info)
    same_stream(got, ref, ("width", width, chunk))
    assert info["refills"] == N - width and (ref["event_in"][width:] > 0).all()
    assert "OPTIMAL" in ref["status"]
    h.close(); model.free()


# ---- 2. starts ------------------------------------------------------------------------------------------------------------------
def _few_rows_queue():
    """few_rows_batch twice and once more: 7 problems through 3 slots, so that every kind of member also enters at a refill."""
    return tuple(np.concatenate([a, a, a[:, :1]], axis=1) for a in few_rows_batch())


# The planted LP (the first three cases) has no infinite entry and runs with use_bc_scaling alone.  The others reach every function
# of batch_units.h that the stream entry's kernels call (the norm passes without stores, kb_data_scales, kb_data_header without a
# header, kb_slot_scale at the first fill and at a refill, kb_slot_out): infinite lower and upper row sides and bounds throughout,
# X0 alone, Y0 alone and both, with and without use_bc_scaling.  A start's map takes the member's scale as a number, 1.0 without
# use_bc_scaling, and whether X0 or Y0 is given decides nothing else: so the few-row LP takes the whole cross and the shape with
# segment boundaries each start and each setting once.
@pytest.mark.parametrize("which,shape,use_bc", [pytest.param("xy", "planted", True, id="xy"), pytest.param("x", "planted", True, id="x"),
                                                pytest.param("y", "planted", True, id="y")]
                         + [pytest.param(w, "few_rows", bc, id=f"{w}-few_rows" + ("" if bc else "-no_bc"))
                            for bc in (True, False) for w in ("xy", "x", "y")]
                         + [pytest.param("x", "segments", True, id="x-segments"), pytest.param("y", "segments", False, id="y-segments-no_bc"),
                            pytest.param("xy", "segments", False, id="xy-segments-no_bc")])
def test_starts(gpu, which, shape, use_bc):
    if shape == "planted":
        lp = planted()
        N, width = 7, 3
        args = make_batch(lp, N, 2)
        model = model_of(lp)
        prm = params(stop_tol=1e-4)
        h2 = tree_handle(model, prm)
        rough = h2.solve(*args, param=params(stop_tol=1e-2))   # (a point on the way: a start that is neither zero nor a solution)
        h2.close()
        X0, Y0 = rough["x"], rough["y"]
    else:
        if shape == "few_rows":
            model, args, (N, width) = few_rows_model(), _few_rows_queue(), (7, 3)
        else:
            m, n, rowptr, colind, values = segment_lp()
            z = np.zeros
            model = hprlp.Model.from_csr(m, n, rowptr, colind, values, z(m), z(m), z(n), z(n), z(n))
            args, (N, width) = segment_batch_all_infinities(5), (5, 2)
        prm = hprlp.Parameters(check_iter=50, max_iter=50, stop_tol=1e-12, use_presolve=False, use_bc_scaling=use_bc)
        rng = np.random.default_rng(9)
        X0, Y0 = rng.normal(size=(model.n, N)), rng.normal(size=(model.m, N)) * 0.1
    X0, Y0 = (X0 if "x" in which else None), (Y0 if "y" in which else None)
    h = tree_handle(model, prm)
    ref, got, info = both(h, args, width, X0, Y0)
    same_stream(got, ref, ("starts", which, shape, use_bc))
    assert info["refills"] == N - width and (ref["iter"] > 0).any()
    cold = h.solve_stream(*args, width=width)
    assert not np.array_equal(cold["iter"], ref["iter"]) or not np.array_equal(cold["x"], ref["x"])   # (the start was used)
    h.close(); model.free()


def test_a_slot_handed_on_twice_within_one_event(gpu):
    """A queued problem whose start is its own solution at a tight tolerance ends at its iteration-0 evaluation."""
    lp = planted()
    N, width = 6, 4
    args = make_batch(lp, N, 2)
    model = model_of(lp)
    h, h2 = tree_handle(model, params()), tree_handle(model, params())
    fine = h2.solve(*args, param=params(stop_tol=1e-8, max_iter=199950))
    assert fine["status"] == ["OPTIMAL"] * N
    X0, Y0 = np.zeros((lp["n"], N)), np.zeros((lp["m"], N))
    for p in (0, 4):
        X0[:, p], Y0[:, p] = fine["x"][:, p], fine["y"][:, p]
    ref, got, info = both(h, args, width, X0, Y0)
    same_stream(got, ref, "cascade")
    assert got["iter"][0] == 0 and got["iter"][4] == 0 and (got["iter"][[1, 2, 3, 5]] > 0).all()
    rec = lambda p: (int(got["slot"][p]), int(got["event_in"][p]), int(got["event_out"][p]))
    assert rec(0) == (0, 0, 0) and rec(4) == (0, 0, 0) and rec(5)[:2] == (0, 0), (rec(0), rec(4), rec(5))
    assert info["refill_passes"] == 2 and info["refill_evaluations"] == 1
    h.close(); h2.close(); model.free()


# ---- 3. segment boundaries ------------------------------------------------------------------------------------------------------
def test_segment_boundaries_in_the_norm_passes_and_the_scaling_fill(gpu):
    """m = SEG + 5, n = 2 SEG + 37: one and two segment boundaries with ragged last segments; every problem ends ITER_LIMIT at 50,
    so every event refills, with starts."""
    m, n, rowptr, colind, values = segment_lp()
    z = np.zeros
    model = hprlp.Model.from_csr(m, n, rowptr, colind, values, z(m), z(m), z(n), z(n), z(n))
    prm = hprlp.Parameters(check_iter=50, max_iter=50, stop_tol=1e-12, use_presolve=False)
    N, width = 5, 2
    args = segment_batch(N)
    rng = np.random.default_rng(9)
    X0, Y0 = rng.normal(size=(n, N)), rng.normal(size=(m, N)) * 0.1
    h = tree_handle(model, prm)
    ref, got, info = both(h, args, width, X0, Y0)
    assert ref["status"] == ["ITER_LIMIT"] * N and (ref["iter"] == 50).all()
    assert list(ref["event_in"]) == [0, 0, 1, 1, 2] and info["refills"] == 3
    same_stream(got, ref, "segments")
    h.close(); model.free()


def test_a_queue_longer_than_one_grid_dimension(gpu):
    """count = 65535 + 70: the norm passes run in two slices, and the problems of the second one enter at refills with the scalars
    their slice left.  The 2 x 2 LP of the known-answer tests, 10 iterations each, 128 slots: 513 events."""
    N, width = 65535 + 70, 128
    rng = np.random.default_rng(17)
    model = hprlp.Model.from_csr(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 3.0, 1.0], [-INF, -INF], [10.0, 12.0], [0.0, 0.0], [INF, INF],
                                 [-3.0, -5.0])
    Cm = np.array([[-3.0], [-5.0]]) * (1 + 0.3 * rng.random((2, N)))
    AU = np.array([[10.0], [12.0]]) * (1 + 0.3 * rng.random((2, N)))
    args = (Cm, np.full((2, N), -INF), AU, np.zeros((2, N)), np.full((2, N), INF))
    prm = hprlp.Parameters(check_iter=10, max_iter=10, stop_tol=1e-12, use_presolve=False, use_CR_scaling=False)
    h = tree_handle(model, prm)
    ref, got, info = both(h, args, width)
    assert ref["status"] == ["ITER_LIMIT"] * N and info["refills"] == N - width and int(ref["event_in"].max()) == (N - 1) // width
    same_stream(got, ref, "two slices")
    assert np.unique(got["x"][:, 65535:], axis=1).shape[1] > 1   # (the second slice's problems are problems of their own)
    h.close(); model.free()


# ---- 4. detection ---------------------------------------------------------------------------------------------------------------
def test_detection_gives_the_host_streams_verdicts_and_certificates(gpu):
    N, width = 10, 4
    members, model, args = _mixed(N)
    h = tree_handle(model, hprlp.Parameters(**MIXED_PRM))
    ref, got, info = both(h, args, width, eps_primal=1e-8, eps_dual=1e-8)
    assert ref["status"] == [s for _, s in members] and {"PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL"} <= set(ref["status"])
    same_stream(got, ref, "detection")
    gc, rc = got["certificates"], ref["certificates"]
    assert set(int(k) for k in gc["kind"]) == {0, 1, 2}
    for f in CERT_SCALARS + ("y", "z", "d"):
        assert (gc[f] is None) == (rc[f] is None) and (gc[f] is None or np.array_equal(gc[f], rc[f])), f
    # structure with detection: the ray block is the only block that grows with the queue, and only the verdicts' rays come back
    mem, tr = h.stream_memory(), h.transfer()
    m_, n_ = model.m, model.n
    rays = 8 * sum({0: 0, 1: m_ + n_, 2: n_}[int(k)] for k in gc["kind"])
    assert mem[0] == 0 and mem[1] == 8 * (2 * n_ + m_) * N
    assert 8 * 7 * N + rays <= tr["staged_d2h_bytes"] <= 8 * (7 * N + 2) + rays and rays > 0
    h.close(); model.free()


# ---- 5. count <= width, and the time limit ---------------------------------------------------------------------------------------
def test_count_at_most_width_is_solve_tensors_and_the_time_limit(gpu):
    torch = torch_()
    lp = planted()
    model = model_of(lp)
    h, h2 = tree_handle(model, params(stop_tol=1e-4)), tree_handle(model, params(stop_tol=1e-4))
    args = queue(5, 3)
    targs = [T(a) for a in args]
    for width in (5, 8):
        got = on_host(h.solve_stream_tensors(*targs, width=width))
        ref = on_host(h2.solve_tensors(*targs))
        same_stream(got, ref, ("count <= width", width), record=False)
        assert list(got["slot"]) == list(range(5)) and not got["event_in"].any() and np.array_equal(got["event_out"] * CHECK, ref["iter"])
        assert h.stream_info()["refills"] == 0 and h.info()["Bp"] == h2.info()["Bp"] == 8
    # time_limit 0 through the raw call: the output buffers hold NaN before it
    N, width = 10, 4
    args = queue(N, width)
    good = [T(a).T.contiguous() for a in args]   # (kept alive: (N, rows) contiguous = column-major rows x N)
    m, n = model.m, model.n
    outs = [torch.full((N, rows), float("nan"), dtype=torch.float64, device="cuda") for rows in (n, m, n)]
    it, status = np.full(N, -1, dtype=np.intc), C.create_string_buffer(64 * N)
    sc = hprlp.CBatchedScalars(iter=it.ctypes.data_as(hprlp.c_int_p), status=C.cast(status, C.POINTER(C.c_char)))
    prm = params(time_limit=0.0).to_c()
    rc = hprlp.lib().hprlp_batched_solver_solve_stream_device(h._h, N, width, *[t.data_ptr() for t in good], None, C.byref(prm), None, None,
                                                              None, None, torch.cuda.current_stream().cuda_stream,
                                                              *[o.data_ptr() for o in outs], C.byref(sc))
    assert rc == 0, hprlp.last_error()
    assert [status.raw[64 * k:64 * (k + 1)].split(b"\0")[0].decode() for k in range(N)] == ["TIME_LIMIT"] * N and not it.any()
    rec = [np.zeros(N, dtype=np.intc) for _ in range(3)]
    assert hprlp.lib().hprlp_batched_solver_stream_record(h._h, *(r.ctypes.data_as(hprlp.c_int_p) for r in rec)) == N
    assert list(rec[1]) == [0] * 4 + [-1] * 6 and list(rec[0][4:]) == [-1] * 6
    for o in outs:
        assert not o[width:].cpu().numpy().any()                # the queued ones: exactly zero, not NaN
        assert np.isfinite(o[:width].cpu().numpy()).all()       # the running ones: their iteration-0 point
    ref = h2.solve_stream(*args, width=width, prm=params(time_limit=0.0))
    for f, o in zip(("x", "y", "z"), outs):
        assert np.array_equal(o.T.cpu().numpy(), ref[f]), f
    h.close(); h2.close(); model.free()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_handle_as_it_was(gpu):
    torch = torch_()
    lp = planted()
    model = model_of(lp)
    m, n = model.m, model.n
    prm = params(stop_tol=1e-4)
    N, width = 10, 4
    args = queue(N, width)
    first = tuple(a[:, :width] for a in args)
    targs = [T(a) for a in args]
    h, fresh = tree_handle(model, prm), tree_handle(model, prm)
    plain = h.solve(*first)
    want, want_carried = fresh.solve(*first), fresh.solve(*first, carry=True)
    before = h.info()
    L = hprlp.lib()
    good = [t.T.contiguous() for t in targs]
    ptrs = [t.data_ptr() for t in good]
    outs = [torch.empty((N, rows), dtype=torch.float64, device="cuda") for rows in (n, m, n)]
    sc = hprlp.CBatchedScalars()

    def raw(ptrs, prm=None):
        return L.hprlp_batched_solver_solve_stream_device(h._h, N, width, *ptrs, None, None if prm is None else C.byref(prm), None, None,
                                                          None, None, None, *[o.data_ptr() for o in outs], C.byref(sc))

    def carry_still_valid(tag):
        assert h.info() == before, tag
        got = h.solve(*first, carry=True)
        for f in ("x", "y", "z") + SCALARS:
            assert np.array_equal(got[f], want_carried[f]), (tag, f)
        again = h.solve(*first)   # (and the previous solve is there again for the next refusal)
        for f in ("x", "y", "z") + SCALARS:
            assert np.array_equal(again[f], want[f]), (tag, f)
        return h.info()

    host_c = np.asfortranarray(args[0])
    assert raw([host_c.ctypes.data] + ptrs[1:]) == -1
    print("host address ->", hprlp.last_error())
    assert "batched stream: C" in hprlp.last_error() and ("device memory" in hprlp.last_error() or "runtime" in hprlp.last_error())
    before = carry_still_valid("a host address")
    hip = _loaded_hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 8 * m * (N - 1)) == 0   # one column short
    try:
        assert raw([ptrs[0], short.value] + ptrs[2:]) == -1
        print("short buffer ->", hprlp.last_error())
        assert "AL" in hprlp.last_error() and "short" in hprlp.last_error()
    finally:
        assert hip.hipFree(short) == 0
    before = carry_still_valid("a short buffer")
    bad = np.zeros((n, N))
    bad[7, width + 3] = np.nan   # a problem that would only enter at a refill
    with pytest.raises(RuntimeError, match="not finite"):
        h.solve_stream_tensors(*targs, width=width, X0=T(bad))
    before = carry_still_valid("a NaN start")
    with pytest.raises(RuntimeError, match="multiple of check_iter"):
        h.solve_stream_tensors(*targs, width=width, prm=params(max_iter=3 * CHECK + 1))
    carry_still_valid("a bad max_iter")
    for f in ("x", "y", "z") + SCALARS:
        assert np.array_equal(plain[f], want[f]), f
    assert raw(ptrs) == 0, hprlp.last_error()   # (the raw call itself works)
    assert np.array_equal(outs[0].T.cpu().numpy(), fresh.solve_stream(*args, width=width)["x"])
    h.close(); fresh.close(); model.free()


# ---- 7. structure ---------------------------------------------------------------------------------------------------------------
def test_no_copy_of_the_queue_on_the_device_or_across_the_bus(gpu):
    lp = planted()
    model = model_of(lp)
    m, n = model.m, model.n
    N, width = 10, 4
    args = queue(N, width)
    h = tree_handle(model, params(stop_tol=1e-4))
    rng = np.random.default_rng(3)
    X0 = 0.01 * rng.normal(size=(n, N))
    h.solve_stream(*args, width=width, X0=X0)
    Bp = h.info()["Bp"]
    mem, tr = h.stream_memory(), h.transfer()
    print("host stream", mem, tr)
    assert mem[0] == 8 * ((3 * n + 2 * m) * N + n * N) and mem[1] == 8 * (2 * n + m) * N
    assert tr["staged_h2d_bytes"] == mem[0] + 8 * (4 * Bp + 3 * N) and tr["device_entry"] == 0
    h.solve_stream_tensors(*[T(a) for a in args], width=width, X0=T(X0))
    mem, tr = h.stream_memory(), h.transfer()
    print("device stream", mem, tr)
    assert mem[0] == 0 and mem[1] == 0
    assert mem[2] < 8 * min(n, m) * N   # scalars, partials and tables: per problem, not per element
    assert tr["staged_h2d_bytes"] <= 8 * 4 * Bp and 8 * 7 * N <= tr["staged_d2h_bytes"] <= 8 * (7 * N + 2)
    assert tr["device_entry"] == 1
    h.close(); model.free()


# ---- 8. neighbours --------------------------------------------------------------------------------------------------------------
def test_the_entries_in_turn_on_one_handle(gpu):
    """Host stream, device stream, plain solve, solve_tensors, device stream: each gives the bits it gives on a fresh handle, and the
    graphs alive do not grow after the first round."""
    lp = planted()
    model = model_of(lp)
    prm = params(stop_tol=1e-4)
    N, width = 10, 4
    args = queue(N, width)
    first = tuple(a[:, :width] for a in args)
    targs, tfirst = [T(a) for a in args], [T(a) for a in first]
    steps = (("host stream", lambda s: s.solve_stream(*args, width=width), True),
             ("device stream", lambda s: on_host(s.solve_stream_tensors(*targs, width=width)), True),
             ("plain solve", lambda s: s.solve(*first), False),
             ("solve_tensors", lambda s: on_host(s.solve_tensors(*tfirst)), False),
             ("device stream again", lambda s: on_host(s.solve_stream_tensors(*targs, width=width)), True))
    want = []
    for tag, call, streamed in steps[:4]:   # (the fifth step is the second's call)
        f = tree_handle(model, prm)
        want.append(call(f))
        f.close()
    want.append(want[1])
    h = tree_handle(model, prm)
    alive = None
    for rnd in range(2):
        for (tag, call, streamed), ref in zip(steps, want):
            same_stream(call(h), ref, (rnd, tag), record=streamed)
        if alive is None:
            alive = h.info()["graphs_alive"]
            assert alive > 0
    assert h.info()["graphs_alive"] == alive
    h.close(); model.free()


# ---- 9. layouts -----------------------------------------------------------------------------------------------------------------
def test_a_row_major_tensor_gives_the_bits_of_a_column_major_one(gpu):
    torch = torch_()
    model = model_of(planted())
    N, width = 7, 3
    args = queue(N, width)
    h = tree_handle(model, params(stop_tol=1e-4))
    col = [T(a) for a in args]
    row = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert all(t.stride() == (1, t.shape[0]) for t in col) and all(t.is_contiguous() for t in row)
    a = on_host(h.solve_stream_tensors(*col, width=width))
    same_stream(on_host(h.solve_stream_tensors(*row, width=width)), a, "row-major")
    same_stream(on_host(h.solve_stream_tensors(col[0], row[1], col[2], row[3], col[4], width=width)), a, "mixed layouts")
    assert a["x"].shape == (model.n, N)
    h.close(); model.free()
