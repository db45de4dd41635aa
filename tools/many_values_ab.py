"""Group matrix values of many small LPs (DESIGN.md "Many small LPs", group matrix values): K resident solvers get new matrix
values and new vectors, over and over --
  (a) member by member: hprlp_solver_set_matrix_values for every member (the single entry: what a caller does without the group
      entry), against
  (b) hprlp_solver_set_matrix_values_many for all of them,
both on the SAME handles in ONE process, alternating a / b / a / b, after one warm-up call each (the value maps exist from then on).

  python tools/many_values_ab.py [--k 64] [--repeats 5] [--out profiles/many_values_ab.txt]

K planted 300 x 500 LPs (lpgen.planted_lp(300, 500, 2500, seed)), one model each.  A repeat gives every member new values
val * (1 + 1e-3 normal) and new vectors (c moved by 1e-3 relative, the row sides outwards), the same on both sides; the table has
the best of the repeats per side, first for the entry alone, then for the entry followed by what a caller needs before the next
resolve (a: power_iteration + init per member, which is Solver.set_matrix; b: power_iteration_many + init per member), the ratio
a / b, and both count vectors of hprlp_last_values_many_counts: b's from its last call, a's the sum over K calls of the group entry
with one member each, which issues that member's own hprlp_solver_set_matrix_values and counts it (nominal where the solver keeps
no count).  After the last repeat the two sides' scaled matrices and vectors must be equal bit for bit (side b ran last on the
handles, side a on a second set of handles kept in step).  One GPU process; any failing step ends the run with its message and a
non-zero exit status.  A host without a GPU fails.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def round_values(lp, rnd, k):
    rng = np.random.default_rng(1000 * rnd + k)
    m, n = lp["m"], lp["n"]
    AL, AU = np.asarray(lp["AL"], float), np.asarray(lp["AU"], float)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    return dict(values=f(lp["values"] * (1 + 1e-3 * rng.normal(size=len(lp["values"])))), c=f(lp["c"] * (1 + 1e-3 * rng.normal(size=n))),
                AL=f(AL - 1e-3 * rng.uniform(size=m) * (1 + np.abs(AL))), AU=f(AU + 1e-3 * rng.uniform(size=m) * (1 + np.abs(AU))),
                l=f(lp["l"]), u=f(lp["u"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from many_ab import quiet
    from conftest import hprlp as H, lpgen
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_values_ab] no GPU: " + H.last_error())
    if not hasattr(L, "hprlp_solver_set_matrix_values_many"):
        sys.exit("[many_values_ab] the library has no hprlp_solver_set_matrix_values_many: " + H.LIB_PATH)
    K = a.k
    prm = H.Parameters(use_presolve=False)
    lps = [lpgen.planted_lp(300, 500, 2500, seed) for seed in range(100, 100 + K)]
    models = [H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"]) for lp in lps]
    with quiet():
        both = [H.Solver(m, prm) for m in models]    # the handles both sides run on
        twin = [H.Solver(m, prm) for m in models]    # side a once more, for the comparison of the bits at the end
        for s in both + twin:
            s.prepare()
    p = lambda v: v.ctypes.data_as(H.c_dbl_p)

    def single(s, d):
        if L.hprlp_solver_set_matrix_values(s.h, p(d["values"]), len(d["values"]), p(d["c"]), None, p(d["AL"]), p(d["AU"]), p(d["l"]), p(d["u"])) != 0:
            sys.exit("[many_values_ab] hprlp_solver_set_matrix_values: " + H.last_error())

    def side_a(solvers, data, further):
        t0 = time.perf_counter()
        for s, d in zip(solvers, data):
            single(s, d)
            if further:
                lam, _ = s.power_iteration()
                s.init(-1.0, 1.01 * lam)
        return time.perf_counter() - t0

    def side_b(solvers, data, further):
        t0 = time.perf_counter()
        H.Solver.set_matrix_many(solvers, data)   # (raises with hprlp_last_error() on a non-zero return)
        if further:
            for s, (lam, _) in zip(solvers, H.Solver.power_iteration_many(solvers)):
                s.init(-1.0, 1.01 * lam)
        return time.perf_counter() - t0

    best = {}
    rnd = 0
    with quiet():
        for further in (False, True):
            for rep in range(a.repeats + 1):   # (repeat 0: the warm-up call of each side)
                for label, run in (("a member by member", side_a), ("b group", side_b)):
                    data = [round_values(lps[k], rnd, k) for k in range(K)]
                    t = run(both, data, further)
                    if label[0] == "b":
                        counts_b = H.last_values_many_counts()
                        side_a(twin, data, further)   # (the twins follow side b's data: the bits compared at the end)
                    if rep > 0:
                        key = (label, further)
                        best[key] = min(best.get(key, t), t)
                    rnd += 1
        # side a's count vector: the group entry with one member each issues the member's own call and counts it
        counts_a = dict.fromkeys(H.VALUES_MANY_KEYS, 0)
        data = [round_values(lps[k], rnd, k) for k in range(K)]
        for s, t, d in zip(both, twin, data):
            H.Solver.set_matrix_many([s], [d])
            for key, v in H.last_values_many_counts().items():
                counts_a[key] += v
            single(t, d)
        same = all(np.array_equal(s.get(v), t.get(v)) for s, t in zip(both, twin) for v in ("A_val", "AT_val", "AL", "AU", "l", "u", "c", "row_norm", "col_norm"))
        for s in both + twin:
            s.close()
    for m in models:
        m.free()
    if not same:
        sys.exit("[many_values_ab] the two sides' scaled matrices and vectors differ")
    lines = [f"# tools/many_values_ab.py: new matrix values and vectors for K = {K} resident planted 300 x 500 LPs, one process, the same handles,",
             f"# a / b alternating, best of {a.repeats} after one warm-up call each; seconds per call for all K members",
             "# side | the entry alone | the entry, power iteration and init"]
    for label in ("a member by member", "b group"):
        lines.append(f"{label} | {best[(label, False)]:.6f} | {best[(label, True)]:.6f}")
    lines.append(f"# a / b: the entry alone {best[('a member by member', False)] / best[('b group', False)]:.2f}, with power iteration and init "
                 f"{best[('a member by member', True)] / best[('b group', True)]:.2f}")
    lines.append("# counts (" + ", ".join(H.VALUES_MANY_KEYS) + ")")
    lines.append("a member by member (K calls of one member, summed) | " + " ".join(str(counts_a[k]) for k in H.VALUES_MANY_KEYS))
    lines.append("b group (one call) | " + " ".join(str(counts_b[k]) for k in H.VALUES_MANY_KEYS))
    lines.append("# scaled matrices and vectors equal bit for bit on both sides after the last repeat: True")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
