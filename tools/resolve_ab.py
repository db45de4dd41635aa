"""Re-solve (DESIGN.md "Re-solve"): a fresh solve() of a changed model against set_data + resolve on a prepared solver.

  python tools/resolve_ab.py [small|c5|all] [tol]
      small: config 2, config 3 and the four 300 x 400 planted LPs of tests/test_resolve.py; c5: config 5 (tol 1e-4); all: both.
      Per LP and change (c and the row sides, times 1 + 1e-3 N): whole-call seconds of solve(use_presolve=False) of the changed
      model; then, on a solver prepared and run on the base model, set_data (hprlp_solver_data_seconds itemised) + resolve cold,
      warm from the base answer, and warm with the base run's last sigma.
  python tools/resolve_ab.py once
      one prepared solver on a 300 x 400 planted LP and ONE set_data of all six: the process to put under
      rocprofv3 --kernel-trace --stats (profiles/resolve_set_data_kernels.txt).
One line per measurement on stdout ("[resolve_ab] ..."); the library's own log goes to stderr.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from warm_ab import _model, _quiet, _timed, perturb  # noqa: E402


def six(lp):
    return dict(c=lp["c"], obj_constant=0.0, AL=lp["AL"], AU=lp["AU"], l=lp["l"], u=lp["u"])


def one(H, out, name, lp, tol, time_limit=60.0):
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=500000, time_limit=time_limit)
    model = _model(H, lp)
    s = H.Solver(model, prm)
    H.lib().hprlp_solver_set_verbose(s.h, 0)
    _, t_prep = _timed(s.prepare)
    base, t_run = _timed(s.run)
    sc = s.scalars()
    print(f"[resolve_ab] {name} ({lp['m']} x {lp['n']}) tol {tol:g}: prepare {t_prep:.4f} s (set-up {sc['setup_time']:.4f}, scaling "
          f"{sc['scaling_time']:.4f}, power iteration {sc['power_time']:.4f}); base run {base.status} {base.iter} it {t_run:.4f} s", file=out)
    for what in ("c", "bounds"):
        lp2 = perturb(lp, what, 1e-3, 7)
        m2 = _model(H, lp2)
        fresh, t_fresh = _timed(lambda: m2.solve(prm))
        m2.free()
        rows = []
        for mode in ("cold", "warm", "warm+sigma"):
            t0 = time.perf_counter()
            s.set_data(**six(lp2))
            t_data = time.perf_counter() - t0
            ds = s.data_seconds()
            if mode == "cold":
                r = s.resolve()
            elif mode == "warm":
                r = s.resolve(base.x, base.y)
            else:
                r = s.resolve(base.x, base.y, sigma=base.trace[-1]["sigma"])
            t_all = time.perf_counter() - t0
            rows.append(f"{mode} {r.status} {r.iter} it, whole {t_all:.4f} s (set_data {t_data:.5f}: upload {ds['upload']:.5f}, kernels + fetch "
                        f"{ds['kernels']:.5f}; reported time {r.time:.4f})")
        print(f"[resolve_ab] {name} {what} x(1 + 1e-3 N): fresh solve() {fresh.status} {fresh.iter} it, whole call {t_fresh:.4f} s; "
              + "; ".join(rows), file=out)
    s.close()
    model.free()


def small(tol):
    from conftest import hprlp as H, lpgen
    from test_resolve import SEEDS, base_lp
    out = _quiet()
    cases = {"config 2": lpgen.c2_25fv47_like(), "config 3": lpgen.c3_pds20_like()}
    cases.update({f"planted seed {s}": base_lp(s) for s in SEEDS})
    for name, lp in cases.items():
        one(H, out, name, lp, tol)


def c5(tol=1e-4):
    import bench as B
    out = _quiet()
    m, n, per_row, band = B.WORKLOADS["c5"]
    one(B.H, out, "config 5", B.banded_lp(m, n, per_row, band), tol, time_limit=300.0)


def once():
    from conftest import hprlp as H
    from test_resolve import base_lp, changed
    out = _quiet()
    lp = base_lp(11)
    s = H.Solver(_model(H, lp), H.Parameters(use_presolve=False))
    s.prepare()
    s.set_data(**six(changed(lp, "rows1e-3")))
    print("[resolve_ab] one set_data:", s.data_seconds(), file=out)
    s.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "small"
    tol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-6
    if what in ("small", "all"):
        small(tol)
    if what in ("c5", "all"):
        c5(1e-4)
    if what == "once":
        once()
    if what not in ("small", "c5", "all", "once"):
        sys.exit(__doc__)
