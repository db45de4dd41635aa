"""Device-resident batches (GPU): BatchedSolver.solve_tensors / hprlp_batched_solver_solve_device (DESIGN.md "Device-resident
batches") -- the batch's vectors come as torch tensors on the GPU, x / y / z come back as torch tensors, and the per-member scaling
with its norms runs in kb_data_in / kb_data_bc.

The reference of every comparison is the HOST entry (numpy in, numpy out) on a handle with set_norms(1), i.e. prepare_batch on the
host with the tree rule, which tests/test_batch_prep_tree.py holds to a numpy restatement without a GPU.  Equality means: the same
status and iter of every member, np.array_equal on x, y, z, and == on primal_obj, residuals and gap (assert_same of
tests/test_gpu_batched_resident.py); the seven per-member scalars of the scaling are compared bit for bit as well.  Nothing is owed
a tolerance: the kernels follow the host twin operation by operation, and the order of every sum is fixed by the vector's length.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import hprlp, lpgen
from test_gpu_batched_detect import MIXED_PRM, _mixed
from test_gpu_batched_resident import assert_same, fresh
from test_gpu_warm import make_batch, model_of

pytestmark = pytest.mark.gpu

INF = np.inf
SEG, LANES = hprlp.NORM_SEG, hprlp.NORM_LANES
PLANTED_PRM = dict(stop_tol=1e-6, max_iter=20000, use_presolve=False)


def torch_():
    import torch
    return torch


def T(a):
    """(rows, B) numpy -> float64 tensor on the GPU whose transpose is contiguous: the layout solve_tensors takes without a copy."""
    if a is None:
        return None
    t = torch_().from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).cuda().T
    assert t.stride() == (1, a.shape[0]) or a.shape[1] == 1
    return t


def on_host(res):
    """A solve_tensors result with x, y, z as numpy arrays."""
    out = dict(res)
    for f in ("x", "y", "z"):
        assert isinstance(res[f], torch_().Tensor) and res[f].is_cuda and res[f].dtype == torch_().float64
        out[f] = res[f].cpu().numpy()
    return out


def same_scalars(a, b, tag):
    for k in hprlp.BATCH_SCALARS:
        assert np.array_equal(a[k], b[k]), (tag, k, a[k], b[k])


@functools.lru_cache(maxsize=None)
def planted():
    return lpgen.planted_lp(300, 400, 2400, 7, values="network")


@functools.lru_cache(maxsize=None)
def planted_batch(B, seed=2):
    """make_batch of the resident-batch tests with infinite entries in AL, AU, l, u and C = 0 in the last member."""
    lp = planted()
    Cm, AL, AU, L, U = (np.array(a) for a in make_batch(lp, B, seed))
    AL[:4, :] = -INF
    AU[5:8, 1:] = INF
    L[10:13, :] = np.where(np.arange(B) % 2 == 0, -INF, L[10:13, :])
    U[:4, :] = INF
    Cm[:, B - 1] = 0.0
    for a in (AL, AU, L, U):
        assert np.isinf(a).any()
    return Cm, AL, AU, L, U


def tree_handle(model, prm):
    h = hprlp.BatchedSolver(model, prm)
    h.set_norms(1)
    return h


@pytest.mark.parametrize("B", [8, 70, 3])
def test_tensors_in_tensors_out_equal_the_host_entry_bit_for_bit(gpu, B):
    """B = 8; 70: two chunks of 64 with 58 padding members; 3: a panel narrower than a tile.  With the staging traffic of both."""
    model, prm = model_of(planted()), hprlp.Parameters(**PLANTED_PRM)
    args = planted_batch(B)
    m, n = model.m, model.n
    h = tree_handle(model, prm)
    ref = h.solve(*args)
    ref_sc, ref_tr, Bp = h.scalars(), h.transfer(), h.info()["Bp"]
    got = h.solve_tensors(*[T(a) for a in args])
    sc, tr = h.scalars(), h.transfer()
    print("B", B, "statuses", sorted(set(ref["status"])), "iter", min(ref["iter"]), "..", max(ref["iter"]), "host", ref_tr, "device", tr)
    assert_same(on_host(got), ref, ("B", B))
    same_scalars(sc, ref_sc, ("B", B))
    assert got["x"].shape == (n, B) and got["y"].shape == (m, B) and got["z"].shape == (n, B)
    assert got["x"].stride() == (1, n) or B == 1
    assert sc["sigma"][B - 1] == 1.0 and sc["norm_c"][B - 1] == 0.0  # the member with C = 0
    # no copy: the host entry stages the header and 3 n B + 2 m B words in and 2 n B + m B out, the device entry at most the
    # header one way and the scalars with their flag words the other
    assert ref_tr["staged_h2d_bytes"] == 8 * (4 * Bp + 3 * n * B + 2 * m * B) and ref_tr["staged_d2h_bytes"] == 8 * (2 * n * B + m * B)
    assert ref_tr["device_entry"] == 0 and tr["device_entry"] == 1 and tr["device_solves"] == 1
    assert tr["staged_h2d_bytes"] <= 8 * 4 * Bp and 8 * 7 * B <= tr["staged_d2h_bytes"] <= 8 * (7 * B + 2)
    h.close(); model.free()


@functools.lru_cache(maxsize=None)
def segment_lp():
    """Two entries per row, m = SEG + 5, n = 2 SEG + 37: a segment boundary in AL / AU, two in C / l / u, ragged last segments."""
    m, n = SEG + 5, 2 * SEG + 37
    rng = np.random.default_rng(5)
    i = np.arange(m)
    cols = np.stack([i, m + i % (n - m)], axis=1).astype(np.int32)
    vals = rng.choice([-1.0, 1.0], size=(m, 2)) * rng.uniform(0.5, 2.0, size=(m, 2))
    rowptr = (2 * np.arange(m + 1)).astype(np.int32)
    return m, n, rowptr, cols.ravel(), vals.ravel()


@functools.lru_cache(maxsize=None)
def segment_batch(B):
    m, n = SEG + 5, 2 * SEG + 37
    rng = np.random.default_rng(50 + B)
    Cm = rng.normal(size=(n, B))
    AL = -1.0 - rng.random((m, B))
    AU = 1.0 + rng.random((m, B))
    L = -rng.random((n, B))
    U = 1.0 + rng.random((n, B))
    AL[rng.random((m, B)) < 0.2] = -INF
    AU[rng.random((m, B)) < 0.2] = INF
    U[rng.random((n, B)) < 0.1] = INF
    Cm[:, B - 1] = 0.0
    return Cm, AL, AU, L, U


@functools.lru_cache(maxsize=None)
def segment_batch_all_infinities(B):
    """segment_batch with infinite lower bounds as well: every replacement of batch_units.h on both sides of the boundaries."""
    Cm, AL, AU, L, U = (np.array(a) for a in segment_batch(B))
    L[np.random.default_rng(70 + B).random(L.shape) < 0.1] = -INF
    return Cm, AL, AU, L, U


def few_rows_model():
    """The 2 x 2 LP of the known-answer tests."""
    return hprlp.Model.from_csr(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 3.0, 1.0], [-INF, -INF], [10.0, 12.0], [0.0, 0.0], [INF, INF],
                                [-3.0, -5.0])


def few_rows_batch():
    """Three members of the 2 x 2 LP (rows x members): the LP itself, one with an infinite upper row side, a finite lower one, an
    infinite lower bound and a finite upper one, and one with every side and bound finite."""
    Cm = np.array([[-3.0, -3.3, -2.5], [-5.0, -4.1, -5.5]])
    AL = np.array([[-INF, -INF, -1.0], [-INF, 2.0, -2.0]])
    AU = np.array([[10.0, 10.5, 11.0], [12.0, INF, 12.5]])
    L = np.array([[0.0, -INF, 0.0], [0.0, 0.0, -1.0]])
    U = np.array([[INF, INF, 6.0], [INF, 4.0, 7.0]])
    return Cm, AL, AU, L, U


@pytest.mark.parametrize("shape,B,use_bc", [pytest.param("segments", 3, True, id="3"), pytest.param("segments", 33, True, id="33"),
                                            pytest.param("segments+lower", 3, True, id="3-lower_bounds"),
                                            pytest.param("segments+lower", 3, False, id="3-lower_bounds-no_bc"),
                                            pytest.param("few_rows", 3, True, id="few_rows"),
                                            pytest.param("few_rows", 3, False, id="few_rows-no_bc")])
def test_segment_boundaries_and_a_partly_filled_member_tile(gpu, shape, B, use_bc):
    """Every function of batch_units.h that the batch entry's kernels call (the two norm passes, kb_data_scales, kb_data_header,
    kb_panel_out), against the host entry: with and without use_bc_scaling, infinite lower and upper row sides and bounds, no start,
    X0 alone, Y0 alone and both -- at the smallest shape with segment boundaries and on a few-row LP with a partly filled tile.
    (The first two cases are older: no infinite lower bound, and no start or both.)"""
    if shape == "few_rows":
        model, args = few_rows_model(), few_rows_batch()
    else:
        m, n, rowptr, colind, values = segment_lp()
        z = np.zeros
        model = hprlp.Model.from_csr(m, n, rowptr, colind, values, z(m), z(m), z(n), z(n), z(n))
        args = segment_batch(B) if shape == "segments" else segment_batch_all_infinities(B)
    m, n = model.m, model.n
    prm = hprlp.Parameters(check_iter=50, max_iter=50, stop_tol=1e-12, use_presolve=False, use_bc_scaling=use_bc)
    rng = np.random.default_rng(9)
    X0, Y0 = rng.normal(size=(n, B)), rng.normal(size=(m, B)) * 0.1  # (the starts' map crosses the segments too)
    starts = [(None, None), (X0, Y0)] + ([] if shape == "segments" else [(X0, None), (None, Y0)])
    h = tree_handle(model, prm)
    for step, (x0, y0) in enumerate(starts):
        ref = h.solve(*args, X0=x0, Y0=y0)
        ref_sc = h.scalars()
        got = h.solve_tensors(*[T(a) for a in args], X0=T(x0), Y0=T(y0))
        print(shape, "B", B, "use_bc", use_bc, "step", step, "statuses", sorted(set(ref["status"])), "iter", sorted(set(ref["iter"])))
        assert_same(on_host(got), ref, (shape, B, use_bc, step))
        same_scalars(h.scalars(), ref_sc, (shape, B, use_bc, step))
        assert use_bc or (ref_sc["b_scale"] == 1.0).all() and (ref_sc["c_scale"] == 1.0).all()
    h.close(); model.free()


def test_carry_across_the_two_entries_equals_the_explicit_start(gpu):
    model, prm = model_of(planted()), hprlp.Parameters(**PLANTED_PRM)
    B = 8
    args = planted_batch(B)
    C2 = args[0] * (1 + 1e-3 * np.random.default_rng(40).normal(size=args[0].shape))
    args2 = (C2,) + tuple(args[1:])
    targs, targs2 = [T(a) for a in args], [T(a) for a in args2]
    h = tree_handle(model, prm)
    # device, then device with carry = device with the previous tensors as the start = the host entry from that start
    d1 = h.solve_tensors(*targs)
    carried = on_host(h.solve_tensors(*targs2, carry=True))
    explicit = on_host(h.solve_tensors(*targs2, X0=d1["x"], Y0=d1["y"]))
    x1, y1 = d1["x"].cpu().numpy(), d1["y"].cpu().numpy()
    ref = h.solve(*args2, X0=x1, Y0=y1)
    assert_same(carried, explicit, "device -> device carry")
    assert_same(carried, ref, "device -> device carry, host reference")
    # host, then device with carry
    r1 = h.solve(*args)
    assert np.array_equal(r1["x"], x1) and np.array_equal(r1["y"], y1)
    assert_same(on_host(h.solve_tensors(*targs2, carry=True)), ref, "host -> device carry")
    # device, then host with carry
    h.solve_tensors(*targs)
    assert_same(h.solve(*args2, carry=True), ref, "device -> host carry")
    print("carry: iterations cold", list(r1["iter"]), "carried", list(ref["iter"]))
    h.close(); model.free()


def test_detection_off_on_off_through_tensors(gpu):
    members, model, args = _mixed(5)
    prm = hprlp.Parameters(**MIXED_PRM)
    h = tree_handle(model, prm)
    ref_off = h.solve(*args)
    ref_on = h.solve(*args, eps_primal=1e-8, eps_dual=1e-8)
    assert {"PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE", "OPTIMAL"} <= set(ref_on["status"]), ref_on["status"]
    targs = [T(a) for a in args]
    for step, on in enumerate((False, True, False)):
        got = on_host(h.solve_tensors(*targs, eps_primal=1e-8 if on else None, eps_dual=1e-8 if on else None))
        assert_same(got, ref_on if on else ref_off, ("detection", step, on))
        if on:
            gc, rc = got["certificates"], ref_on["certificates"]
            assert set(gc["kind"]) == {0, 1, 2}
            for f in ("kind", "iter", "objective", "violation", "y", "z", "d"):
                assert (gc[f] is None) == (rc[f] is None) and (gc[f] is None or np.array_equal(gc[f], rc[f])), f
        else:
            assert "certificates" not in got
    h.close(); model.free()


def test_a_row_major_tensor_gives_the_bits_of_a_column_major_one(gpu):
    torch = torch_()
    model, prm = model_of(planted()), hprlp.Parameters(**PLANTED_PRM)
    args = planted_batch(8)
    h = tree_handle(model, prm)
    col = [T(a) for a in args]
    row = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    assert all(t.stride() == (1, t.shape[0]) for t in col) and all(t.is_contiguous() for t in row)
    a = on_host(h.solve_tensors(*col))
    b = on_host(h.solve_tensors(*row))
    mixed = on_host(h.solve_tensors(col[0], row[1], col[2], row[3], col[4]))
    assert_same(b, a, "row-major")
    assert_same(mixed, a, "mixed layouts")
    h.close(); model.free()


def _loaded_hip_runtime():
    """The HIP runtime this process has loaded already (the library and torch share it), as a ctypes handle."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64.so" in path:
            return C.CDLL(path)
    raise AssertionError("no HIP runtime loaded")


def test_refused_calls_leave_the_handle_usable(gpu):
    torch = torch_()
    model, prm = model_of(planted()), hprlp.Parameters(**PLANTED_PRM)
    B = 8
    m, n = model.m, model.n
    args = planted_batch(B)
    targs = [T(a) for a in args]
    h = tree_handle(model, prm)
    L = hprlp.lib()

    def still_fine(tag, ref):
        assert_same(on_host(h.solve_tensors(*targs)), ref, tag)

    def refused(what, exc, *a, **kw):
        with pytest.raises(exc) as e:
            h.solve_tensors(*a, **kw)
        print(what, "->", str(e.value))
        return str(e.value)

    assert "previous" in refused("carry on the first call", RuntimeError, *targs, carry=True)
    ref = h.solve(*args)
    still_fine("after carry on the first call", ref)
    before = h.info()

    # through the raw C call: a host address where a device pointer belongs, and a device buffer one element short
    outs = [torch.empty((B, rows), dtype=torch.float64, device="cuda") for rows in (n, m, n)]
    sc = hprlp.CBatchedScalars()

    def raw(ptrs):
        return L.hprlp_batched_solver_solve_device(h._h, B, *ptrs, None, None, None, None, 0, None, None, None, outs[0].data_ptr(),
                                                   outs[1].data_ptr(), outs[2].data_ptr(), C.byref(sc))
    good = [t.T.contiguous() for t in targs]  # (kept alive: (B, rows) contiguous = column-major rows x B)
    ptrs = [t.data_ptr() for t in good]
    host_c = np.asfortranarray(args[0])
    assert raw([host_c.ctypes.data] + ptrs[1:]) == -1
    print("host address ->", hprlp.last_error())
    assert "C" in hprlp.last_error() and ("device memory" in hprlp.last_error() or "runtime" in hprlp.last_error())
    still_fine("after a host address", ref)
    hip = _loaded_hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), 8 * (m * B - 1)) == 0
    try:
        assert raw([ptrs[0], short.value] + ptrs[2:]) == -1
        print("short buffer ->", hprlp.last_error())
        assert "AL" in hprlp.last_error() and "short" in hprlp.last_error()
    finally:
        assert hip.hipFree(short) == 0
    still_fine("after a short buffer", ref)
    assert raw(ptrs) == 0, hprlp.last_error()  # (the raw call itself works)
    assert np.array_equal(outs[0].T.cpu().numpy(), ref["x"])

    # a non-finite start: found by the kernel that maps the starts, refused before the loop; a carry still works afterwards
    bad = ref["x"].copy()
    bad[7, 3] = np.nan
    solves = h.info()["solves"]
    assert "non-finite" in refused("NaN in X0", RuntimeError, *targs, X0=T(bad), Y0=T(ref["y"]))
    assert h.info()["solves"] == solves
    args2 = (args[0] * 1.001,) + tuple(args[1:])
    carried = on_host(h.solve_tensors(*[T(a) for a in args2], carry=True))
    assert_same(carried, h.solve(*args2, X0=ref["x"], Y0=ref["y"]), "carry after the refused start")
    still_fine("after a NaN start", ref)

    # in Python, before the C call
    assert "float64" in refused("float32", ValueError, targs[0].float(), *targs[1:])
    assert "device" in refused("a CPU tensor", ValueError, targs[0], targs[1].cpu(), *targs[2:])
    assert "shape" in refused("a wrong shape", ValueError, *targs[:4], targs[4][:, :B - 1])
    assert "shape" in refused("a wrong start", ValueError, *targs, X0=targs[1])
    assert "torch tensor" in refused("numpy", ValueError, targs[0], args[1], *targs[2:])
    still_fine("after the Python refusals", ref)
    assert {k: v for k, v in h.info().items() if k != "solves"} == {k: v for k, v in before.items() if k != "solves"}
    h.close(); model.free()


def test_the_host_entry_without_set_norms_keeps_its_bits(gpu):
    """A handle that never called set_norms: its host entry is the fresh solve_batched_warm before and after a device-entry call."""
    model, prm = model_of(planted()), hprlp.Parameters(**PLANTED_PRM)
    B = 8
    args = planted_batch(B)
    ref = fresh(model, args, None, prm)
    h = hprlp.BatchedSolver(model, prm)
    assert_same(h.solve(*args), ref, "before")
    dev = on_host(h.solve_tensors(*[T(a) for a in args]))
    assert len(dev["status"]) == B and dev["x"].shape == ref["x"].shape  # (another norm rule: close, not the same bits)
    assert_same(h.solve(*args), ref, "after")
    assert_same(h.solve(*args, carry=True), fresh(model, args, None, prm, ref["x"], ref["y"]), "host carry after host")
    h.close(); model.free()
