"""New matrix values for a resident solver, the part that needs no GPU (include/hprlp_amd.h hprlp_solver_set_matrix_values and
its companions, DESIGN.md "Matrix values"): the rule of the value maps (hprlp_value_maps_host) against a numpy restatement, the
entry points with the header's signatures, NULL handles refused with a message, and the Python wrappers' length checks.
tests/test_gpu_matrix_values.py imports the changed models and the numpy maps from here."""
import ctypes as C

import numpy as np
import pytest
from scipy import sparse

from conftest import hprlp, lpgen
from test_resolve import base_lp, header_prototypes

KINDS = ("rel1e-3", "rows", "signs+zeros")


def changed_matrix(lp, kind, seed):
    """The pattern of `lp` with new values, and the vectors planted anew on the new matrix (lpgen._plant), so that the changed LP
    has a known optimum.  rel1e-3: every value x (1 + 1e-3 xi); rows: rows rescaled by 10^U(-3, 3), which moves every scaling
    factor; signs+zeros: about 1 % of the signs flipped and two stored zeros, in rows and columns that keep other entries."""
    rng = np.random.default_rng(seed)
    m, n = lp["m"], lp["n"]
    rp, ci, v = lp["rowptr"], lp["colind"], lp["values"].copy()
    row_of = np.repeat(np.arange(m), np.diff(rp))
    if kind == "rel1e-3":
        v *= 1 + 1e-3 * rng.normal(size=len(v))
    elif kind == "rows":
        v *= (10.0 ** rng.uniform(-3, 3, size=m))[row_of]
    elif kind == "signs+zeros":
        v[rng.random(len(v)) < 0.01] *= -1.0
        rows_n, cols_n = np.diff(rp), np.bincount(ci, minlength=n)
        ok = np.flatnonzero((rows_n[row_of] >= 3) & (cols_n[ci] >= 3))
        zr = [int(ok[0])]   # two entries in different rows and columns: every row and column keeps a nonzero
        zr.append(int(next(k for k in ok[::-1] if row_of[k] != row_of[zr[0]] and ci[k] != ci[zr[0]])))
        v[zr] = 0.0
    else:
        raise ValueError(kind)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))   # (stored zeros stay stored)
    out = lpgen._plant(rng, A)
    out.update(m=m, n=n, A=A, rowptr=rp, colind=ci, values=v)
    return out


def numpy_maps(m, n, rowptr, colind, pr=None, pc=None):
    """The rule restated: mapA = argsort of the entries by (new row, new column), stable; mapAT = that order sorted by the new
    column, stable (the row-stable transpose).  No ordering: the given order and its stable transpose."""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colind, np.int64)
    row_of = np.repeat(np.arange(m), np.diff(rp))
    if pr is None:
        mapA, icol = np.arange(len(ci)), ci
    else:
        r_old2new = np.empty(m, np.int64); r_old2new[pr] = np.arange(m)
        c_old2new = np.empty(n, np.int64); c_old2new[pc] = np.arange(n)
        key = r_old2new[row_of] * n + c_old2new[ci]
        mapA = np.argsort(key, kind="stable")
        icol = c_old2new[ci][mapA]
    mapAT = mapA[np.argsort(icol, kind="stable")]
    return mapA.astype(np.int32), mapAT.astype(np.int32)


def hand_made():
    """7 x 5, row 3 and column 2 empty, row 5 with its columns not ascending."""
    rows = [[0, 1, 4], [3], [0, 4], [], [1, 3, 4], [4, 0, 1], [3]]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return 7, 5, rp, np.array([j for r in rows for j in r], np.int32)


def patterns():
    lp = base_lp(11)
    yield ("hand-made",) + hand_made()
    yield "base_lp(11)", lp["m"], lp["n"], lp["rowptr"], lp["colind"]


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_value_maps_against_numpy(which, ordered):
    name, m, n, rp, ci = list(patterns())[which]
    pr = pc = None
    if ordered:
        rng = np.random.default_rng(5)
        pr, pc = rng.permutation(m).astype(np.int32), rng.permutation(n).astype(np.int32)
    a, t = hprlp.value_maps_host(m, n, rp, ci, pr, pc)
    wa, wt = numpy_maps(m, n, rp, ci, pr, pc)
    assert np.array_equal(a, wa) and np.array_equal(t, wt), name
    nnz = len(ci)
    assert np.array_equal(np.sort(a), np.arange(nnz)) and np.array_equal(np.sort(t), np.arange(nnz))
    if not ordered:
        assert np.array_equal(a, np.arange(nnz))
    # what the maps are for: values scattered through them are the matrix P A Q and its transpose
    v = np.arange(1.0, nnz + 1)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))
    B = A if pr is None else A[pr][:, pc]
    B = sparse.csr_matrix(B)
    if ordered:
        B.sort_indices()
        assert np.array_equal(B.data, v[a]), name
    assert np.array_equal(sparse.csr_matrix(B.T).toarray(), sparse.csr_matrix((v[t], *transposed_index(m, n, rp, ci, pr, pc)), shape=(n, m)).toarray())


def transposed_index(m, n, rp, ci, pr, pc):
    """(column indices, row pointers) of the transpose of the internal matrix, from scipy."""
    A = sparse.csr_matrix((np.ones(len(ci)), ci, rp), shape=(m, n))
    if pr is not None:
        A = sparse.csr_matrix(A[pr][:, pc])
    T = sparse.csc_matrix(A)   # CSC of A = CSR of A^T, stable in row order
    T.sort_indices()
    return T.indices, T.indptr


def test_value_maps_host_refuses_bad_input():
    m, n, rp, ci = hand_made()
    L = hprlp.lib()
    ip = lambda a: a.ctypes.data_as(hprlp.c_int_p)
    a, t = np.zeros(len(ci), np.int32), np.zeros(len(ci), np.int32)
    bad_perm = np.zeros(m, np.int32)
    pc = np.arange(n, dtype=np.int32)
    assert L.hprlp_value_maps_host(m, n, ip(rp), ip(ci), ip(bad_perm), ip(pc), ip(a), ip(t)) == -1
    assert "permutation" in hprlp.last_error()
    bad_ci = ci.copy(); bad_ci[0] = n
    assert L.hprlp_value_maps_host(m, n, ip(rp), ip(bad_ci), None, None, ip(a), ip(t)) == -1
    assert "out of range" in hprlp.last_error()
    assert L.hprlp_value_maps_host(m, n, ip(rp), ip(ci), None, None, None, ip(t)) == -1


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
CTYPE_OF = {"hprlp_solver *": C.c_void_p, "hprlp_batched_solver *": C.c_void_p, "const double *": hprlp.c_dbl_p, "double *": hprlp.c_dbl_p,
            "long": C.c_long, "int": C.c_int, "int *": hprlp.c_int_p, "const int *": hprlp.c_int_p}
WANT = {
    "hprlp_solver_set_matrix_values": ("int", ["hprlp_solver *", "const double *", "long"] + ["const double *"] * 6),
    "hprlp_solver_matrix_seconds": ("int", ["hprlp_solver *", "double *"]),
    "hprlp_solver_value_maps": ("long", ["hprlp_solver *", "int *", "int *", "long"]),
    "hprlp_value_maps_host": ("int", ["int", "int"] + ["const int *"] * 4 + ["int *", "int *"]),
    "hprlp_batched_solver_set_matrix_values": ("int", ["hprlp_batched_solver *", "const double *", "long"]),
}


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    assert protos[name] == WANT[name], protos[name]
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in WANT[name][1]], fn.argtypes
    assert fn.restype is (C.c_long if WANT[name][0] == "long" else C.c_int)


def test_null_handles_are_refused_with_a_message():
    L = hprlp.lib()
    v = np.zeros(4)
    p = v.ctypes.data_as(hprlp.c_dbl_p)
    assert L.hprlp_solver_set_matrix_values(None, p, 4, p, None, p, p, p, p) == -1
    assert "null solver" in hprlp.last_error()
    assert L.hprlp_solver_matrix_seconds(None, np.zeros(6).ctypes.data_as(hprlp.c_dbl_p)) == -1
    assert "null solver" in hprlp.last_error()
    i = np.zeros(4, np.int32).ctypes.data_as(hprlp.c_int_p)
    assert L.hprlp_solver_value_maps(None, i, i, 4) == -1
    assert "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_set_matrix_values(None, p, 4) == -1
    assert "null solver" in hprlp.last_error()


class _Model:
    m, n, nnz = 3, 4, 5


def _unborn(cls, **attrs):
    """A wrapper object without a library handle behind it: the length checks come before the library is called."""
    s = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def test_python_wrappers_refuse_wrong_lengths():
    s = _unborn(hprlp.Solver, model=_Model(), h=None)
    good = dict(values=np.ones(5), c=np.ones(4), AL=np.ones(3), AU=np.ones(3), l=np.ones(4), u=np.ones(4))
    for k, bad in (("values", np.ones(4)), ("c", np.ones(3)), ("AL", np.ones(4)), ("AU", np.ones((3, 1))), ("l", np.ones(5)),
                   ("u", np.ones(0)), ("c", None)):
        with pytest.raises(ValueError, match="length"):
            s.set_matrix(**dict(good, **{k: bad}))
    b = _unborn(hprlp.BatchedSolver, model=_Model(), _h=1)
    for bad in (np.ones(4), np.ones((5, 1))):
        with pytest.raises(ValueError, match="length"):
            b.set_matrix(bad)
    with pytest.raises(ValueError, match="length"):
        hprlp.value_maps_host(3, 4, np.zeros(3, np.int32), np.zeros(0, np.int32))
    for f in ("set_matrix", "matrix_seconds", "value_maps"):
        assert callable(getattr(hprlp.Solver, f)), f


def test_changed_matrices_are_the_issues():
    lp = base_lp(11)
    for kind in KINDS:
        lp2 = changed_matrix(lp, kind, 3)
        assert np.array_equal(lp2["rowptr"], lp["rowptr"]) and np.array_equal(lp2["colind"], lp["colind"])
        assert len(lp2["values"]) == len(lp["values"]) and not np.array_equal(lp2["values"], lp["values"])
        assert np.all(np.isfinite(lp2["values"])) and np.isfinite(lp2["obj_star"])
    z = changed_matrix(lp, "signs+zeros", 3)
    assert int(np.sum(z["values"] == 0.0)) == 2
    flipped = np.sum(np.sign(z["values"]) == -np.sign(lp["values"]))
    assert 0.003 * len(lp["values"]) < flipped < 0.03 * len(lp["values"])
    A = sparse.csr_matrix((np.abs(z["values"]), z["colind"], z["rowptr"]), shape=(z["m"], z["n"]))
    was = sparse.csr_matrix((np.abs(lp["values"]), lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    assert np.array_equal(np.asarray(A.sum(1) > 0), np.asarray(was.sum(1) > 0))
    assert np.array_equal(np.asarray(A.sum(0) > 0), np.asarray(was.sum(0) > 0))
    r = changed_matrix(lp, "rows", 3)
    ratio = np.abs(r["values"] / lp["values"])
    assert ratio.min() < 1e-2 and ratio.max() > 1e2
