"""Matrix values (DESIGN.md "Matrix values"): a fresh solver on a model whose coefficients changed against set_matrix on a
resident one.

  python tools/matrix_values_ab.py [small|c5|c5perm|batched|all]
      small:   config 2, config 3 and the banded 8000 x 10000 shape of the tiled tests (HPRLP_TEST_HOOKS=1 with
               HPRLP_TILED_MIN_ROWS=1 HPRLP_TILED_MIN_DENSE=0.0 HPRLP_NO_REORDER=1 in the environment gives it the tiled form);
      c5:      config 5; c5perm: its randomly permuted variant (locality ordering at set-up);
      batched: the resident batched handle at config 4, B = 64 (create against set_matrix; one solve after each, bits compared).
  Per model, every value times (1 + 1e-3 N), the vectors kept:
      A  hprlp_solver_create + scale + power iteration on the changed model (wall seconds, with the solver's own set-up,
         scaling and power-iteration seconds);
      B1 the FIRST set_matrix of a solver prepared on the base model (it builds the value maps) + its power iteration;
      B2 a LATER set_matrix + power iteration (a second change), hprlp_solver_matrix_seconds itemised for both;
  and whether B2's state equals a fresh solver's bit for bit.  One line per measurement on stdout ("[matrix_values_ab] ...");
  the library's own log goes to stderr.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from warm_ab import _model, _quiet, _timed  # noqa: E402

STATE = ("A_val", "AT_val", "row_norm", "col_norm", "c", "AL", "AU", "l", "u")


def new_values(lp, seed):
    return lp["values"] * (1 + 1e-3 * np.random.default_rng(seed).normal(size=len(lp["values"])))


def mat(lp, values):
    return dict(values=values, c=lp["c"], AL=lp["AL"], AU=lp["AU"], l=lp["l"], u=lp["u"])


def fresh(H, lp, values, prm):
    model = _model(H, dict(lp, values=values))
    t0 = time.perf_counter()
    s = H.Solver(model, prm)
    H.lib().hprlp_solver_set_verbose(s.h, 0)
    s.scale()
    lam, its = s.power_iteration()
    wall = time.perf_counter() - t0
    return s, model, lam, its, wall


def one(H, out, name, lp):
    prm = H.Parameters(use_presolve=False)
    v1, v2 = new_values(lp, 1), new_values(lp, 2)
    s, model, _, _, t_base = fresh(H, lp, lp["values"], prm)
    s.init(-1.0, 1.0)
    desc = s.describe()
    print(f"[matrix_values_ab] {name} ({lp['m']} x {lp['n']}, {len(lp['values'])} nnz): {desc}", file=out)
    rows = []
    for tag, v in (("B1 first set_matrix", v1), ("B2 later set_matrix", v2)):
        (lam, its), wall = _timed(lambda: s.set_matrix(**mat(lp, v)))
        ms, sc = s.matrix_seconds(), s.scalars()
        rows.append((tag, wall, lam, its))
        print(f"[matrix_values_ab] {name} {tag} + power iteration: wall {wall:.4f} s (maps {ms['maps']:.4f}, upload + check "
              f"{ms['upload']:.4f}, kernels {ms['kernels']:.4f}, scale {ms['scale']:.4f}, call {ms['total']:.4f}; power iteration "
              f"{sc['power_time']:.4f}, {its} it)", file=out)
    f, fm, lamF, itsF, t_fresh = fresh(H, lp, v2, prm)
    sc = f.scalars()
    same = (lamF, itsF) == rows[1][2:] and all(np.array_equal(s.get(k), f.get(k)) for k in STATE)
    print(f"[matrix_values_ab] {name} A fresh create + scale + power iteration: wall {t_fresh:.4f} s (set-up {sc['setup_time']:.4f}, "
          f"scaling {sc['scaling_time']:.4f}, power iteration {sc['power_time']:.4f}, {itsF} it; the base solver took {t_base:.4f}); "
          f"B1 / A {rows[0][1] / t_fresh:.3f}, B2 / A {rows[1][1] / t_fresh:.3f}; bits {'equal' if same else 'DIFFER'}", file=out)
    for x, y in ((s, model), (f, fm)):
        x.close()
        y.free()


def small(out):
    from conftest import hprlp as H, lpgen
    from scipy import sparse
    one(H, out, "config 2", lpgen.c2_25fv47_like())
    one(H, out, "config 3", lpgen.c3_pds20_like())
    rp, ci, v = lpgen.banded_csr(8000, 10000, 8, 1500, 6)
    A = sparse.csr_matrix((v, ci, rp), shape=(8000, 10000))
    A.sum_duplicates()
    A.sort_indices()
    lp = lpgen._plant(np.random.default_rng(33), A)
    lp.update(m=8000, n=10000, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy())
    one(H, out, "banded 8000 x 10000", lp)


def c5(out, permuted):
    import bench as B
    m, n, per_row, band = B.WORKLOADS["c5"]
    lp = B.banded_lp(m, n, per_row, band)
    if permuted:
        lp = B.permute_lp(lp)
    one(B.H, out, "config 5, randomly permuted" if permuted else "config 5", lp)


def batched(out):
    from conftest import hprlp as H, lpgen
    from test_gpu_warm import make_batch
    lp, B = lpgen.c3_pds20_like(), 64
    prm = H.Parameters(stop_tol=1e-4, max_iter=3000, use_presolve=False)   # (the batch keeps the base model's sides: no member need converge)
    args = make_batch(lp, B, 2)
    v1, v2 = new_values(lp, 1), new_values(lp, 2)
    model = _model(H, lp)
    h, t_base = _timed(lambda: H.BatchedSolver(model, prm))
    h.solve(*args)
    for tag, v in (("B1 first set_matrix", v1), ("B2 later set_matrix", v2)):
        before = h.seconds()
        _, wall = _timed(lambda: h.set_matrix(v))
        after = h.seconds()
        print(f"[matrix_values_ab] config 4 batched (B = {B}) {tag}: wall {wall:.4f} s (values + scaling "
              f"{after['create_setup'] - before['create_setup']:.4f}, power iteration {after['create_power'] - before['create_power']:.4f})", file=out)
    got = h.solve(*args)
    m2 = _model(H, dict(lp, values=v2))
    f, t_fresh = _timed(lambda: H.BatchedSolver(m2, prm))
    ref = f.solve(*args)
    sec = f.seconds()
    same = got["status"] == ref["status"] and all(np.array_equal(got[k], ref[k]) for k in ("iter", "x", "y", "z"))
    print(f"[matrix_values_ab] config 4 batched (B = {B}) A fresh create: wall {t_fresh:.4f} s (set-up + scaling {sec['create_setup']:.4f}, "
          f"power iteration {sec['create_power']:.4f}; the base handle took {t_base:.4f}); panels {h.info()['panel_allocations']} allocation(s); "
          f"the next solve's bits {'equal' if same else 'DIFFER'}", file=out)
    h.close(); f.close(); model.free(); m2.free()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "small"
    out = _quiet()
    if what in ("small", "all"):
        small(out)
    if what in ("batched", "all"):
        batched(out)
    if what in ("c5", "all"):
        c5(out, False)
    if what in ("c5perm", "all"):
        c5(out, True)
