"""Group detection of many small LPs (DESIGN.md "Many small LPs", group detection): K small LPs, half of them planted infeasible
or unbounded, detection on for every member.

  python tools/many_detect_ab.py [--k 64] [--repeats 3] [--max-iter 50000] [--out profiles/many_detect_ab.txt]

One process measures ONE library (HPRLP_LIB names another build, as tools/ab_libs.sh: run the parent commit's library and this
tree's alternately, A/B/A/B, and compare the lines).  Three sides, each after one unmeasured warm-up run:
  run_many   K resident handles (created, scaled and power-iterated once); per run every handle is reset and initialised
             (unmeasured), the timed part is ONE Solver.run_many and the K certificate() calls -- what a caller of the parent commit
             does with detection on, and what every library has;
  steps      the whole way of such a caller: create_many, scale_many, power_iteration_many, init and set_detection per member,
             run_many, certificate() per member, close_many;
  detect     ONE solve_many_detect of the same models (where the library has the entry).
The table gives the median wall time with its spread, the eight counts of hprlp_last_run_many_counts (rounds waits group-launches copies
own served ray_served certs_served; a library without the last two reports 0) and a digest of statuses, iterations, x and the
certificates' arrays, which must be the same on every side and in every library.  A host without a GPU fails.
"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from many_ab import quiet  # noqa: E402


def digest(results, certs):
    h = hashlib.sha1()
    for r, k in zip(results, certs):
        h.update(f"{r.status} {r.iter} {k.kind} {k.iter} ".encode())
        for v in (r.x, k.y, k.z, k.d):
            if v is not None:
                h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()[:12]


def counts_text(H):
    c = H.last_run_many_detect_counts()
    return " ".join(str(c.get(k, 0)) for k in ("rounds", "waits", "group_launches", "copies", "own", "served", "ray_served", "certs_served"))


def arm(solvers, lams):
    for s, lam in zip(solvers, lams):
        s.init(-1.0, lam * 1.01)
        s.set_detection()


def side_run_many(H, solvers, lams):
    for s in solvers:
        s.reset()
    arm(solvers, lams)
    t0 = time.perf_counter()
    res = H.Solver.run_many(solvers)
    certs = [s.certificate() for s in solvers]
    return time.perf_counter() - t0, res, certs


def side_steps(H, models, prm):
    t0 = time.perf_counter()
    solvers = H.Solver.create_many(models, prm)
    H.Solver.scale_many(solvers)
    lams = [lam for lam, _ in H.Solver.power_iteration_many(solvers)]
    arm(solvers, lams)
    res = H.Solver.run_many(solvers)
    certs = [s.certificate() for s in solvers]
    H.Solver.close_many(solvers)
    return time.perf_counter() - t0, res, certs


def side_detect(H, models, prm):
    t0 = time.perf_counter()
    res, certs = H.solve_many_detect(models, prm)
    return time.perf_counter() - t0, res, certs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=50000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from conftest import hprlp as H, lpgen
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_detect_ab] no GPU: " + H.last_error())
    K = a.k
    prm = H.Parameters(stop_tol=1e-4, use_presolve=False, use_CR_scaling=False, max_iter=a.max_iter)
    lps = []
    for k in range(K):   # in turn: feasible, infeasible, feasible, unbounded
        seed = 200 + k
        lps.append(lpgen.planted_lp(300, 500, 2500, seed) if k % 2 == 0 else
                   lpgen.planted_infeasible_lp(400, 600, 2400, seed) if k % 4 == 1 else lpgen.planted_unbounded_lp(400, 600, 2400, seed))
    models = [H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
              for lp in lps]
    has_entry = hasattr(L, "hprlp_solve_many_detect")
    with quiet():
        resident = H.Solver.create_many(models, prm)
        H.Solver.scale_many(resident)
        lams = [lam for lam, _ in H.Solver.power_iteration_many(resident)]
    sides = [("run_many", lambda: side_run_many(H, resident, lams)), ("steps", lambda: side_steps(H, models, prm))]
    if has_entry:
        sides.append(("detect", lambda: side_detect(H, models, prm)))
    lines = [f"# tools/many_detect_ab.py: K = {K} small LPs (planted 300 x 500 feasible, 400 x 600 infeasible / unbounded in turn: {K // 2} with a",
             f"# verdict to find), detection on, stop_tol 1e-4, no Curtis-Reid scaling, max_iter {a.max_iter}, no presolve; {a.repeats} measured runs per side after one warm-up run",
             f"# library {H.LIB_PATH}  (hprlp_solve_many_detect: {'yes' if has_entry else 'no'})",
             "# side | wall seconds, median [min .. max] | counts (rounds waits group-launches copies own served ray_served certs_served) | "
             "statuses | iterations of the verdicts | digest"]
    for name, run in sides:
        walls = []
        for rep in range(a.repeats + 1):
            with quiet():
                wall, res, certs = run()
            if rep > 0:
                walls.append(wall)
        walls.sort()
        st = {}
        for r in res:
            st[r.status] = st.get(r.status, 0) + 1
        vit = sorted(r.iter for r in res if r.status.endswith("INFEASIBLE"))
        lines.append(f"{name} | {statistics.median_low(walls):.4f} [{walls[0]:.4f} .. {walls[-1]:.4f}] | {counts_text(H)} | "
                     f"{' '.join(f'{k}:{v}' for k, v in sorted(st.items()))} | {vit[0] if vit else '-'} .. {vit[-1] if vit else '-'} | {digest(res, certs)}")
        print(lines[-1], flush=True)
    H.Solver.close_many(resident)
    for m in models:
        m.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
