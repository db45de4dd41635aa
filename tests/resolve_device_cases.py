"""The cases of tests/test_gpu_resolve_device.py (DESIGN.md "Device-resident re-solve"), one function each.  The kernel form is
chosen by environment switches that the library reads as a solver is set up, so the cases that name a form run in a process of
their own: `python resolve_device_cases.py <case> [form]`.  The others are called in the test process.

The reference of every comparison is the HOST entry (set_data / resolve / set_matrix) on a second solver prepared the same way.
Equality is status, iter, every scalar of Results but the wall-clock times, every trace row and array_equal on x, y, z: no
tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import hprlp, lpgen  # noqa: E402
from test_gpu_detect import model_of  # noqa: E402
from test_resolve import base_lp, changed  # noqa: E402
import test_gpu_resolve as T  # noqa: E402

ALL = T.VECS + T.B_SIDE + T.C_SIDE
SCALARS = ("residuals", "primal_obj", "gap", "iter4", "iter6", "iter8", "iter")   # (time, time4 .. time8: wall clock)
EXPECT = {"small": "single-workgroup kernel", "stream": "A: stream kernel", "tiled": "tiled, fused (k_tiled_fused",
          "reordered": "locality ordering applied"}


def torch_():
    import torch
    return torch


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def six_t(lp):
    return dict(c=dev(lp["c"]), obj_constant=0.0, AL=dev(lp["AL"]), AU=dev(lp["AU"]), l=dev(lp["l"]), u=dev(lp["u"]))


def to_host(r):
    """x, y, z of a resolve_tensors() result as numpy arrays, in place."""
    for f in ("x", "y", "z"):
        v = getattr(r, f)
        assert v.is_cuda and v.dtype == torch_().float64
        setattr(r, f, v.cpu().numpy())
    return r


def same_results(a, b):
    bad = T.same_run(a, b)
    bad += [(k, getattr(a, k), getattr(b, k)) for k in SCALARS
            if not np.array_equal(np.float64(getattr(a, k)), np.float64(getattr(b, k)), equal_nan=True)]
    return bad


def check_equal(tag, a, b):
    bad = same_results(a, b)
    print(tag, a.status, a.iter, "| host", b.status, b.iter, "| differs:", bad[:3])
    assert not bad, (tag, bad[:3])


def pair(lp, prm, form=None):
    S, H = T.prepared(lp, prm), T.prepared(lp, prm)
    if form:
        assert EXPECT[form] in S.describe(), S.describe()
    return S, H


def words(S):
    t = S.transfer()
    return t["h2d_bytes"], t["d2h_bytes"], t["device_entry"]


def raw_resolve(S, x0, y0, xo, yo, zo, sigma=-1.0, max_trace=4096):
    """hprlp_solver_resolve_device itself: tensors or None for every device argument.  Returns (rc, Results or None)."""
    torch = torch_()
    res = hprlp.CResults()
    trace = (hprlp.CTraceRow * max_trace)()
    nt = C.c_int(0)
    ptr = [None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in (x0, y0, xo, yo, zo)]
    rc = hprlp.lib().hprlp_solver_resolve_device(S.h, float(sigma), ptr[0], ptr[1], torch.cuda.current_stream().cuda_stream, ptr[2], ptr[3],
                                                 ptr[4], C.byref(res), trace, max_trace, C.byref(nt))
    if rc != 0:
        return rc, None
    assert not res.x and not res.y and not res.z   # (NULL: nothing for the caller to free)
    r = hprlp.Results(res, S.model.m, S.model.n)
    r.trace = [{f: getattr(trace[i], f) for f, _ in hprlp.CTraceRow._fields_} for i in range(nt.value)]
    r.x, r.y, r.z = xo, yo, zo
    return rc, r


# ---- 1. set_data_tensors against set_data -------------------------------------------------------------------------------------------
def case_set_data(form):
    lp = base_lp(11)
    m, n = lp["m"], lp["n"]
    for use_bc in (True, False):
        prm = T.params(max_iter=3000, use_bc_scaling=use_bc)
        S, H = pair(lp, prm, form)
        for change in ("c1e-3", "rows1e-3", "kinds"):
            lp2 = changed(lp, change)
            S.set_data_tensors(**six_t(lp2))
            H.set_data(**T.six(lp2))
            assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL), (change, T.same_bits(T.snapshot(S), T.snapshot(H), ALL))
            assert words(S) == (0, 0, 1) and words(H) == ((2 * m + 3 * n) * 8, 0, 0), (words(S), words(H))
            check_equal("%s bc=%s %s" % (form, use_bc, change), to_host(S.resolve_tensors()), H.resolve())
        lp2, lp3 = changed(lp, "c1e-3"), changed(changed(lp, "rows1e-3"), "kinds")
        for kw, bytes_in in ((dict(c=lp2["c"]), n * 8), (dict(AL=lp3["AL"], AU=lp3["AU"], l=lp3["l"], u=lp3["u"]), (2 * m + 2 * n) * 8),
                             (dict(obj_constant=3.5), 0)):
            S.set_data_tensors(**{k: (v if k == "obj_constant" else dev(v)) for k, v in kw.items()})
            H.set_data(**kw)
            assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL), sorted(kw)
            assert words(S) == (0, 0, 1) and words(H) == (bytes_in, 0, 0), (sorted(kw), words(S), words(H))
            check_equal("%s bc=%s partial %s" % (form, use_bc, sorted(kw)), to_host(S.resolve_tensors()), H.resolve())
        assert S.transfer()["device_calls"] == 12 and H.transfer()["device_calls"] == 0
        T.close(S, H)


# ---- 2. resolve_tensors against resolve ---------------------------------------------------------------------------------------------
def case_resolve():
    torch = torch_()
    lp = base_lp(11)
    m, n = lp["m"], lp["n"]
    S, H = pair(lp, T.params(max_iter=100000))
    cold, hc = to_host(S.resolve_tensors()), H.resolve()
    check_equal("cold", cold, hc)
    assert hc.status == "OPTIMAL"
    assert words(S) == (0, 0, 1) and words(H) == (0, (2 * n + m) * 8, 0), (words(S), words(H))
    rng = np.random.default_rng(3)
    x0, y0 = hc.x + rng.normal(scale=0.1, size=n), hc.y + rng.normal(scale=0.1, size=m)
    hw = H.resolve(x0, y0)
    assert words(H) == ((n + m) * 8, (2 * n + m) * 8, 0), words(H)
    check_equal("from a start", to_host(S.resolve_tensors(dev(x0), dev(y0))), hw)
    # the start and the results are the same tensors
    xt, yt, zt = dev(x0), dev(y0), torch.empty(n, dtype=torch.float64, device="cuda")
    rc, r = raw_resolve(S, xt, yt, xt, yt, zt)
    assert rc == 0, hprlp.last_error()
    check_equal("start and results in the same tensors", to_host(r), hw)
    assert words(S) == (0, 0, 1)
    sig = hc.trace[-1]["sigma"]
    hs = H.resolve(x0, y0, sigma=sig)
    assert hs.trace[0]["sigma"] == sig
    check_equal("a caller's sigma", to_host(S.resolve_tensors(dev(x0), dev(y0), sigma=sig)), hs)
    # z not wanted
    xo, yo = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
    rc, r = raw_resolve(S, dev(x0), dev(y0), xo, yo, None)
    assert rc == 0, hprlp.last_error()
    assert np.array_equal(xo.cpu().numpy(), hw.x) and np.array_equal(yo.cpu().numpy(), hw.y) and (r.status, r.iter) == (hw.status, hw.iter)
    # detection on seed 11's `kinds` data (unbounded below), and back
    lp2 = changed(lp, "kinds")
    for s in (S, H):
        s.set_detection(1e-8, 1e-8)
    S.set_data_tensors(**six_t(lp2))
    H.set_data(**T.six(lp2))
    rd, hd = to_host(S.resolve_tensors()), H.resolve()
    ks, kh = S.certificate(), H.certificate()
    print("kinds, seed 11:", rd.status, rd.iter, "certificate kind", ks.kind, "| host", hd.status, hd.iter, kh.kind)
    check_equal("detection", rd, hd)
    assert (ks.kind, ks.iter, ks.objective, ks.violation) == (kh.kind, kh.iter, kh.objective, kh.violation)
    for f in ("y", "z", "d"):
        a, b = getattr(ks, f), getattr(kh, f)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f
    S.set_data_tensors(**six_t(lp))
    H.set_data(**T.six(lp))
    back, hb = to_host(S.resolve_tensors()), H.resolve()
    check_equal("back on the base data", back, hb)
    assert hb.status == "OPTIMAL" and S.certificate().kind == 0
    T.close(S, H)


# ---- 3. / 4. the large forms: one set_data_tensors + resolve_tensors from a start ---------------------------------------------------
def planted_on(A, seed):
    from scipy import sparse
    A = sparse.csr_matrix(A); A.sum_duplicates(); A.sort_indices()
    lp = lpgen._plant(np.random.default_rng(seed), A)
    lp.update(m=A.shape[0], n=A.shape[1], A=A, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy())
    return lp


def case_large(form):
    from scipy import sparse
    if form == "reordered":   # (the shape of tests/test_gpu_warm.py / test_gpu_resolve.py: the ordering is applied to large matrices only)
        m = n = 1_600_000
        rp, ci, v = lpgen.banded_csr(m, n, 10, 16000, 5)
        A = sparse.csr_matrix((v, ci, rp), shape=(m, n)); A.sum_duplicates()
        rng = np.random.default_rng(8)
        pr, pc = rng.permutation(m), rng.permutation(n)
        inv = np.empty(n, np.int64); inv[pc] = np.arange(n)
        B = A[pr]; B = sparse.csr_matrix((B.data, inv[B.indices], B.indptr), shape=(m, n))
        lp, iters = planted_on(B, 32), 2 * 150
    else:
        m, n = 8000, 10000
        rp, ci, v = lpgen.banded_csr(m, n, 8, 1500, 6)
        lp, iters = planted_on(sparse.csr_matrix((v, ci, rp), shape=(m, n)), 33), 3 * 150
    prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-9, max_iter=iters, check_iter=150)
    S, H = pair(lp, prm, form)
    assert S.info()["reordered"] == (form == "reordered")
    f = 1 + 1e-3 * np.random.default_rng(8).normal(size=lp["m"])
    lp2 = dict(lp, c=lp["c"] * (1 + 1e-3 * np.random.default_rng(7).normal(size=lp["n"])), AL=lp["AL"] * f, AU=lp["AU"] * f)
    rng = np.random.default_rng(3)
    x0, y0 = lp["x_star"] + rng.normal(scale=0.1, size=lp["n"]), lp["y_star"] + rng.normal(scale=0.1, size=lp["m"])
    S.set_data_tensors(**six_t(lp2))
    H.set_data(**T.six(lp2))
    assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL)
    r, h = to_host(S.resolve_tensors(dev(x0), dev(y0))), H.resolve(x0, y0)
    check_equal(form, r, h)
    assert h.iter == iters and np.isfinite(h.x).all() and np.abs(h.x).max() > 0 and np.abs(h.y).max() > 0 and np.abs(h.z).max() > 0
    assert words(S) == (0, 0, 1)
    T.close(S, H)


# ---- 5. set_matrix_tensors against set_matrix -----------------------------------------------------------------------------------------
def case_matrix(form):
    lp = base_lp(12)
    S, H = pair(lp, T.params(max_iter=3000), form)
    vals = lp["values"] * (1 + 1e-3 * np.random.default_rng(5).normal(size=lp["values"].shape[0]))
    lp2 = changed(changed(lp, "rows1e-3"), "kinds")
    vec = [lp2[k] for k in ("c", "AL", "AU", "l", "u")]
    for rnd in range(2):   # (the first call builds the value maps, the second finds them)
        ps = S.set_matrix_tensors(dev(vals), *[dev(a) for a in vec])
        ph = H.set_matrix(vals, *vec)
        for k in ("A_val", "AT_val", "row_norm", "col_norm"):
            assert np.array_equal(S.get(k), H.get(k)), k
        assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL)
        assert ps == ph and S.scalars()["lambda_max"] == H.scalars()["lambda_max"], (ps, ph)
        nnz = lp["values"].shape[0]
        assert words(S) == (0, 0, 1) and words(H) == ((nnz + 2 * lp["m"] + 3 * lp["n"]) * 8, 0, 0), (words(S), words(H))
        check_equal("%s matrix values, call %d" % (form, rnd), to_host(S.resolve_tensors()), H.resolve())
        vals = vals * (1 + 1e-3 * np.random.default_rng(6).normal(size=vals.shape[0]))
    T.close(S, H)


# ---- 6. entries alternate on one handle -----------------------------------------------------------------------------------------------
def case_alternate():
    lp = base_lp(12)
    lp1, lp2 = changed(lp, "c1e-3"), changed(lp, "rows1e-3")
    S, H = pair(lp, T.params())
    S.set_data(**T.six(lp1))
    H.set_data(**T.six(lp1))
    assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL)
    r1, h1 = to_host(S.resolve_tensors()), H.resolve()
    check_equal("host set_data, tensor resolve", r1, h1)
    S.set_data_tensors(**six_t(lp2))
    H.set_data(**T.six(lp2))
    assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL)
    check_equal("tensor set_data, host resolve", S.resolve(h1.x, h1.y), H.resolve(h1.x, h1.y))
    assert S.transfer()["device_calls"] == 2 and words(S)[2] == 0
    T.close(S, H)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def loaded_hip_runtime():
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64.so" in path:
            return C.CDLL(path)
    raise AssertionError("no HIP runtime loaded")


def case_refusals():
    import pytest
    torch = torch_()
    L = hprlp.lib()
    lp = base_lp(11)
    m, n = lp["m"], lp["n"]
    lp2 = changed(lp, "c1e-3")
    S, H = pair(lp, T.params(max_iter=600))
    S.set_data_tensors(**six_t(lp2))
    H.set_data(**T.six(lp2))
    ref = H.resolve()
    before = T.snapshot(S)
    stream = torch.cuda.current_stream().cuda_stream

    def still_fine(tag):
        assert not T.same_bits(before, T.snapshot(S), ALL), tag
        check_equal("after " + tag, to_host(S.resolve_tensors()), ref)

    still_fine("nothing")
    good = dev(lp["c"])
    host = np.ascontiguousarray(lp["c"])
    assert L.hprlp_solver_set_data_device(S.h, host.ctypes.data, None, None, None, None, None, stream) == -1
    print("host address ->", hprlp.last_error())
    assert "c" in hprlp.last_error() and ("device memory" in hprlp.last_error() or "runtime" in hprlp.last_error())
    still_fine("a host address")
    hip = loaded_hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    short = C.c_void_p()   # (an allocation of its own: a tensor of n - 1 is a piece of torch's larger block, whose range is what the runtime reports)
    assert hip.hipMalloc(C.byref(short), 8 * (n - 1)) == 0
    try:
        assert L.hprlp_solver_set_data_device(S.h, short.value, None, None, None, None, None, stream) == -1
        print("short buffer ->", hprlp.last_error())
        assert "c " in hprlp.last_error() and "short" in hprlp.last_error()
        still_fine("a short buffer")
        xo, yo = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(m, dtype=torch.float64, device="cuda")
        rc, _ = raw_resolve(S, None, None, xo, yo, short.value)
        assert rc == -1
        print("short output ->", hprlp.last_error())
        assert "z " in hprlp.last_error() and "short" in hprlp.last_error()
        still_fine("an output buffer one short")
    finally:
        assert hip.hipFree(short) == 0
    for tag, bad in (("a numpy array", lp["c"]), ("a CPU tensor", torch.from_numpy(lp["c"].copy())), ("float32", good.float()),
                     ("a wrong length", good[:-1])):
        with pytest.raises(ValueError):
            S.set_data_tensors(c=bad)
        with pytest.raises(ValueError):
            S.resolve_tensors(x=bad)
        with pytest.raises(ValueError):
            S.set_matrix_tensors(dev(lp["values"]), bad, *[dev(lp[k]) for k in ("AL", "AU", "l", "u")])
        still_fine(tag)
    nan_c = lp["c"].copy(); nan_c[7] = np.nan
    with pytest.raises(RuntimeError, match=r"c\[7\] is NaN"):
        S.set_data_tensors(c=dev(nan_c))
    still_fine("a NaN in c[7]")
    nan_u = lp["u"].copy(); nan_u[-1] = np.nan
    with pytest.raises(RuntimeError, match=r"u\[%d\] is NaN" % (n - 1)):
        S.set_data_tensors(c=dev(lp["c"]), AL=dev(lp["AL"]), AU=dev(lp["AU"]), l=dev(lp["l"]), u=dev(nan_u))
    still_fine("a NaN in the last entry of u")
    with pytest.raises(RuntimeError, match="together"):
        S.set_data_tensors(AL=dev(lp["AL"]), AU=dev(lp["AU"]))
    still_fine("an incomplete bounds group")
    inf_x = ref.x.copy(); inf_x[13] = np.inf
    with pytest.raises(RuntimeError, match=r"x0\[13\] is not finite"):
        S.resolve_tensors(dev(inf_x), dev(ref.y))
    still_fine("inf in x0")
    nan_v = lp["values"].copy(); nan_v[41] = np.nan
    with pytest.raises(RuntimeError, match=r"val\[41\] is not finite"):
        S.set_matrix_tensors(dev(nan_v), *[dev(lp2[k]) for k in ("c", "AL", "AU", "l", "u")])
    still_fine("a NaN in values")
    with pytest.raises(RuntimeError, match=r"AL\[0\] is NaN"):
        S.set_matrix_tensors(dev(lp["values"]), dev(lp2["c"]), dev(np.full(m, np.nan)), *[dev(lp2[k]) for k in ("AU", "l", "u")])
    still_fine("a NaN vector with the matrix values")
    T.close(S, H)


# ---- 8. a non-default stream ------------------------------------------------------------------------------------------------------------
def case_stream():
    torch = torch_()
    lp = base_lp(12)
    S, H = pair(lp, T.params())
    base, f = dev(lp["c"]), dev(1 + 1e-3 * np.random.default_rng(7).normal(size=lp["n"]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c2 = base * f   # (produced on the side stream, which set_data_tensors is handed as the inputs' stream)
        S.set_data_tensors(c=c2)
        r = S.resolve_tensors()
    side.synchronize()
    H.set_data(c=c2.cpu().numpy())
    assert not T.same_bits(T.snapshot(S), T.snapshot(H), ALL)
    check_equal("side stream", to_host(r), H.resolve())
    T.close(S, H)


if __name__ == "__main__":
    case, args = sys.argv[1], sys.argv[2:]
    {"set_data": case_set_data, "large": case_large, "matrix": case_matrix}[case](*args)
    print("OK", case, *args)
