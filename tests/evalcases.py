"""The LPs the evaluation tests run on (tests/test_evalref.py, tests/test_gpu_evaluation.py): every column and row bound kind
cycled by index over a feasible planted point, on the smallest shape at which existing tests show each kernel form selected.
A plain module: no fixtures."""
import numpy as np
from scipy import sparse

COL_KINDS = 8   # (0, inf), (-0.0, inf), (-inf, inf), (-inf, f), (f != 0, inf), (f, g), (f, f), (0, g)
ROW_KINDS = 5   # equality, (-inf, b), (b, inf), (a, b), (-inf, inf)


def all_bounds_lp(A, seed):
    """An LP on the CSR matrix A that carries every bound kind, cycled by index over a feasible planted point x*, with a cost made
    of sign-consistent multipliers (y > 0 on a row at AL, z > 0 on a column at l), so the LP is bounded."""
    A = sparse.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    m, n = A.shape
    rng = np.random.default_rng(seed)
    jk, ik = np.arange(n) % COL_KINDS, np.arange(m) % ROW_KINDS
    f = rng.uniform(0.5, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    width = rng.uniform(0.5, 2.0, size=n)
    at_l = rng.random(n) < 0.4
    at_u = ~at_l & (rng.random(n) < 0.4)
    inside = rng.uniform(0.1, 0.9, size=n)
    l, u, x, z = np.zeros(n), np.full(n, np.inf), np.zeros(n), np.zeros(n)
    zl, zu = rng.uniform(0.1, 1.0, size=n), -rng.uniform(0.1, 1.0, size=n)
    for kind in range(COL_KINDS):
        k = jk == kind
        lo = {0: 0.0, 1: -0.0, 2: -np.inf, 3: -np.inf, 4: f, 5: f, 6: f, 7: 0.0}[kind]
        hi = {0: np.inf, 1: np.inf, 2: np.inf, 3: f, 4: np.inf, 5: f + width, 6: f, 7: width}[kind]
        lo, hi = np.broadcast_to(lo, n)[k], np.broadcast_to(hi, n)[k]
        l[k], u[k] = lo, hi
        base = np.where(np.isfinite(lo), lo, np.where(np.isfinite(hi), hi - 2.0, -1.0))
        top = np.where(np.isfinite(hi), hi, base + 2.0)
        xi = base + inside[k] * (top - base)
        lo_hit, hi_hit = at_l[k] & np.isfinite(lo), at_u[k] & np.isfinite(hi)
        xi = np.where(lo_hit, lo, np.where(hi_hit, hi, xi))
        x[k] = xi + 0.0   # (-0.0 + 0.0 = +0.0: the planted point itself carries no negative zero)
        z[k] = np.where(lo_hit, zl[k], np.where(hi_hit, zu[k], 0.0))
    b = A @ x
    slack_lo, slack_hi = rng.uniform(0.5, 2.0, size=m), rng.uniform(0.5, 2.0, size=m)
    act = rng.random(m) < 0.5
    AL, AU, y = np.full(m, -np.inf), np.full(m, np.inf), np.zeros(m)
    k = ik == 0
    AL[k], AU[k], y[k] = b[k], b[k], rng.normal(size=int(k.sum()))
    k = ik == 1
    AU[k] = np.where(act[k], b[k], b[k] + slack_hi[k])
    y[k] = np.where(act[k], -rng.uniform(0.1, 1.0, size=int(k.sum())), 0.0)
    k = ik == 2
    AL[k] = np.where(act[k], b[k], b[k] - slack_lo[k])
    y[k] = np.where(act[k], rng.uniform(0.1, 1.0, size=int(k.sum())), 0.0)
    k = ik == 3
    AL[k], AU[k] = b[k] - np.where(act[k], 0.0, slack_lo[k]), b[k] + slack_hi[k]
    y[k] = np.where(act[k], rng.uniform(0.1, 1.0, size=int(k.sum())), 0.0)
    c = A.T @ y + z
    return dict(m=m, n=n, A=A, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy(), AL=AL, AU=AU,
                l=l, u=u, c=c, x_star=x, y_star=y, z_star=z, obj_star=float(c @ x))


def _banded(lpgen, m, n, per_row, band, seed):
    rp, ci, v = lpgen.banded_csr(m, n, per_row, band, seed)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n))
    A.sum_duplicates()
    return A


def _with_lines(A, row_lens, col_lens, seed, empty_rows=(), empty_cols=()):
    """A plus rows / columns of the given entry counts (replacing what the line held) and emptied rows / columns."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    A = sparse.lil_matrix(A)
    lines = rng.choice(min(m, n) - 1, size=len(row_lens) + len(col_lens) + len(empty_rows) + len(empty_cols), replace=False)
    rows_at = lines[:len(row_lens)]
    cols_at = lines[len(row_lens):len(row_lens) + len(col_lens)]
    er = lines[len(row_lens) + len(col_lens):len(row_lens) + len(col_lens) + len(empty_rows)]
    ec = lines[len(lines) - len(empty_cols):] if len(empty_cols) else []
    rows_left = np.setdiff1d(np.arange(m), np.asarray(er, dtype=np.int64))
    for j, L in zip(cols_at, col_lens):
        A[:, j] = 0
        A[np.sort(rng.choice(rows_left, size=L, replace=False)), j] = (rng.normal(size=L) * 0.3 + np.sign(rng.normal(size=L))).reshape(-1, 1)
    for i, L in zip(rows_at, row_lens):
        keep = np.asarray(cols_at, dtype=np.int64)
        held = np.asarray(A[i, keep].todense()).ravel()
        A[i, :] = 0
        free = np.setdiff1d(np.arange(n), np.concatenate([keep, np.asarray(ec, dtype=np.int64)]))
        L_new = L - int((held != 0).sum())
        A[i, np.sort(rng.choice(free, size=L_new, replace=False))] = rng.normal(size=L_new) * 0.3 + np.sign(rng.normal(size=L_new))
        A[i, keep] = held
    for i in er:
        A[i, :] = 0
    for j in ec:
        A[:, j] = 0
    A = sparse.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    lens_r, lens_c = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    return A, dict(rows={int(i): int(lens_r[i]) for i in rows_at}, cols={int(j): int(lens_c[j]) for j in cols_at},
                   empty_rows=[int(i) for i in er], empty_cols=[int(j) for j in ec])


# case -> (the hook set's name in tests/test_gpu_detect.py: FORM_ENV, further hooks, iterate tolerance (rtol, atol) or None = bits)
CASES = {
    "small": ("small", {}, None),
    "stream-short": ("stream", {}, None),
    "stream-rows": ("stream", {}, (1e-10, 1e-12)),
    "tiled": ("tiled", {}, (1e-11, 1e-13)),
    "tiled-rounds": ("tiled", {"HPRLP_TILE_ROWS": "64"}, (1e-11, 1e-13)),
    "pieces": ("pieces", {}, (1e-11, 1e-13)),
    "all-remainder": ("all-remainder", {}, (1e-11, 1e-13)),
    "tiled-aside": ("tiled", {}, (1e-10, 1e-12)),
}
_lp_cache = {}


def case_lp(name, lpgen):
    """The LP of a case (built once per process; callers leave it unchanged)."""
    if name in _lp_cache:
        return _lp_cache[name]
    facts = {}
    if name == "small":
        A = lpgen.planted_lp(400, 600, 2400, 41)["A"]
    elif name == "stream-short":
        A = lpgen.planted_lp(3000, 4000, 18000, 42, dense_col_frac=0.0)["A"]
        assert np.diff(A.indptr).max() <= 64 and np.diff(A.tocsc().indptr).max() <= 64
    elif name == "stream-rows":
        A0 = lpgen.planted_lp(4200, 6000, 25000, 43, dense_col_frac=0.0)["A"]
        A, facts = _with_lines(A0, (64, 65, 350, 4097, 5000), (4097, 65), 44, empty_rows=(0, 0), empty_cols=(0,))
        assert sorted(facts["rows"].values()) == [64, 65, 350, 4097, 5000] and sorted(facts["cols"].values()) == [65, 4097], facts
        lr, lc = np.diff(A.indptr), np.diff(A.tocsc().indptr)
        assert (lr[facts["empty_rows"]] == 0).all() and (lc[facts["empty_cols"]] == 0).all()
    elif name in ("tiled", "pieces"):
        A = _banded(lpgen, 8000, 10000, 8, 1500, 6)
    elif name == "tiled-rounds":
        A = _banded(lpgen, 40000, 40000, 12, 1500, 7)
    elif name == "all-remainder":
        A = lpgen.planted_lp(3000, 4000, 18000, 31, values="network")["A"]
    elif name == "tiled-aside":
        A, facts = _with_lines(_banded(lpgen, 8000, 10000, 8, 1500, 6), (1100, 4200), (1100, 4100), 45)
        assert sorted(facts["rows"].values()) == [1100, 4200] and sorted(facts["cols"].values()) == [1100, 4100], facts
    else:
        raise KeyError(name)
    lp = all_bounds_lp(A, 100 + list(CASES).index(name))
    lp["facts"] = facts
    _lp_cache[name] = lp
    return lp
