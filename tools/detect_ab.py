"""Infeasibility detection (DESIGN.md "Infeasibility and unboundedness"): what it costs and how early it decides.

  python tools/detect_ab.py cost [workload] [tol] [reps]   config-5 LP (bench.py WORKLOADS) solved with detection off (solve) and
                                                          on (hprlp_solve_detect), alternating: iterations, identical bits, loop time
  python tools/detect_ab.py corpus                        iterations and seconds to the verdict on the infeasible / unbounded corpus
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cost(name="c5", tol=1e-4, reps=2):
    import bench as B
    H = B.H
    os.dup2(2, 1)  # (the library's log goes to stderr with ours)
    m, n, per_row, band = B.WORKLOADS[name]
    lp = B.banded_lp(m, n, per_row, band)
    model = H.Model.from_csr(m, n, lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=tol, use_presolve=False, time_limit=900.0)
    runs = {"off": [], "on": []}
    ref = None
    for rep in range(reps):
        for mode in ("off", "on"):
            r = model.solve(prm) if mode == "off" else model.solve_detect(prm)
            loop = H.last_solve_phases()["loop"]
            same = None
            if ref is None:
                ref = r
            else:
                same = r.iter == ref.iter and all(np.array_equal(getattr(r, f), getattr(ref, f)) for f in ("x", "y", "z"))
            runs[mode].append(loop)
            print(f"[detect_ab] {name} rep {rep} detection {mode}: {r.status}, {r.iter} iterations, loop {loop:.4f} s, "
                  f"solver time {r.time:.4f} s, same bits as the first run: {same}", file=sys.stderr)
    off, on = min(runs["off"]), min(runs["on"])
    print(f"[detect_ab] {name} tol={tol:g}: best loop off {off:.4f} s, on {on:.4f} s, on/off {on / off:.4f}", file=sys.stderr)


def corpus():
    from conftest import hprlp as H, lpgen
    from test_gpu_detect import EDGE, as_lp, model_of
    from test_detect import dual_ray_test, primal_ray_test
    cases = {"edge infeasible": as_lp(EDGE["infeasible"]), "edge unbounded": as_lp(EDGE["unbounded"]),
             "transportation 30 < 36": lpgen.transportation_lp([10, 10, 10], [12, 12, 12], 3),
             "transportation 40 x 60": lpgen.transportation_lp(np.full(40, 10.0), np.full(60, 6.8), 4),
             "planted infeasible 3000 x 4000": lpgen.planted_infeasible_lp(3000, 4000, 18000, 21),
             "planted unbounded 3000 x 4000": lpgen.planted_unbounded_lp(3000, 4000, 18000, 21),
             "planted infeasible 200k x 250k": lpgen.planted_infeasible_lp(200_000, 250_000, 1_600_000, 31),
             "planted unbounded 200k x 250k": lpgen.planted_unbounded_lp(200_000, 250_000, 1_600_000, 31)}
    for name, lp in cases.items():
        model = model_of(lp)
        t0 = time.perf_counter()
        r = model.solve_detect(H.Parameters(max_iter=30000, use_presolve=False, time_limit=120.0))
        wall = time.perf_counter() - t0
        k = r.certificate
        if k.kind == 1:
            D, V = primal_ray_test(lp, k.y)
            ratio = V / D
        elif k.kind == 2:
            cd, W = dual_ray_test(lp, k.d)
            ratio = W / -cd
        else:
            ratio = float("nan")
        print(f"[detect_ab] {name}: {r.status} at iteration {r.iter}, solver time {r.time:.3f} s (wall {wall:.3f} s), "
              f"numpy ratio {ratio:.2e}", flush=True)
        model.free()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "corpus"
    if what == "cost":
        a = sys.argv[2:]
        cost(a[0] if a else "c5", float(a[1]) if len(a) > 1 else 1e-4, int(a[2]) if len(a) > 2 else 2)
    else:
        corpus()
