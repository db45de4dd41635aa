"""Infeasibility detection in solve_batched (DESIGN.md "Batched detection"): what it costs and what it finds on config 4.

  python tools/detect_batched_ab.py cost [reps]        config-4 recipe as in bench.py (infinite upper bounds clamped to 50), 1500
                                                      batch iterations at stop_tol 1e-30, detection off and on alternating in one
                                                      process: batch iterations/s (best of `reps`, default 3) and identical bits
  python tools/detect_batched_ab.py unclamped [iters] [eps ..]
                                                      the same recipe with U = inf kept, detection on (eps_primal = eps_dual = eps,
                                                      default 1e-8; several: one run each), up to `iters` (60000) iterations:
                                                      per-member status and verdict iteration, batch seconds, every certificate
                                                      checked by the numpy ratio tests of tests/test_detect.py
  python tools/detect_batched_ab.py trace             one detection solve of the B = 64 mixed batch of tests/test_gpu_batched_detect.py
                                                      (run it under rocprofv3 --kernel-trace --stats with HPRLP_NO_GRAPH=1:
                                                      eager launches; the profiler faulted in hipGraphLaunch)
"""
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import hprlp as H, lpgen  # noqa: E402


def config4(clamp):
    """bench.py's config-4 members (seed 4, B = 64) on the config-3 matrix; clamp: infinite upper bounds -> 50 as bench.py does."""
    lp = lpgen.c3_pds20_like()
    B = 64
    rng = np.random.default_rng(4)
    m, n = lp["m"], lp["n"]
    Cm = lp["c"][:, None] * (1 + 0.1 * rng.normal(size=(n, B)))
    AU = lp["AU"][:, None] + np.abs(rng.normal(scale=0.1, size=(m, B)))
    AL = np.repeat(lp["AL"][:, None], B, axis=1)
    AL = np.where(np.isfinite(AL), np.minimum(AL, AU), AL)
    L = np.repeat(lp["l"][:, None], B, axis=1)
    U = np.repeat(lp["u"][:, None], B, axis=1)
    if clamp:
        U = np.where(np.isfinite(U), U, 50.0)
    model = H.Model.from_csr(m, n, lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    return lp, model, (Cm, AL, AU, L, U)


def cost(reps=3, iters=1500):
    lp, model, panels = config4(clamp=True)
    prm = H.Parameters(stop_tol=1e-30, max_iter=iters, use_presolve=False)
    rates = {"off": [], "on": []}
    ref = None
    for rep in range(reps):
        for mode in ("off", "on"):
            r = H.solve_batched(model, *panels, None, prm) if mode == "off" else H.solve_batched_detect(model, *panels, None, prm)
            rate = iters / r["solve_time"]
            rates[mode].append(rate)
            same = None
            if ref is None:
                ref = r
            else:
                same = r["status"] == ref["status"] and all(np.array_equal(r[f], ref[f]) for f in ("x", "y", "z", "iter", "primal_obj"))
            print(f"[detect_batched_ab] cost rep {rep} detection {mode}: {iters} batch iterations in {r['solve_time']:.4f} s = "
                  f"{rate:.1f} it/s, statuses {dict(collections.Counter(r['status']))}, same bits as the first run: {same}", flush=True)
    off, on = max(rates["off"]), max(rates["on"])
    print(f"[detect_batched_ab] cost: best of {reps}: off {off:.1f} it/s, on {on:.1f} it/s, on/off {on / off:.4f}; "
          f"all off {[round(x, 1) for x in rates['off']]}, all on {[round(x, 1) for x in rates['on']]}", flush=True)
    model.free()


def unclamped(iters=60000, eps_list=(1e-8,)):
    lp, model, (Cm, AL, AU, L, U) = config4(clamp=False)
    print(f"[detect_batched_ab] unclamped: {int(np.isinf(U[:, 0]).sum())} of {lp['n']} columns without an upper bound", flush=True)
    for eps in eps_list:
        unclamped_run(lp, model, (Cm, AL, AU, L, U), iters, eps)
    model.free()


def unclamped_run(lp, model, panels, iters, eps):
    from test_detect import dual_ray_test, primal_ray_test
    Cm, AL, AU, L, U = panels
    B = Cm.shape[1]
    prm = H.Parameters(stop_tol=1e-4, max_iter=iters, time_limit=900.0, use_presolve=False)
    t0 = time.perf_counter()
    r = H.solve_batched_detect(model, Cm, AL, AU, L, U, None, prm, eps_primal=eps, eps_dual=eps)
    wall = time.perf_counter() - t0
    cert = r["certificates"]
    print(f"[detect_batched_ab] unclamped eps {eps:g}: statuses {dict(collections.Counter(r['status']))}, batch solve time {r['solve_time']:.3f} s "
          f"(setup {r['setup_time']:.3f} s, wall {wall:.3f} s), last iteration {int(np.max(r['iter']))}", flush=True)
    worst = 0.0
    for k in range(B):
        mk = dict(m=lp["m"], n=lp["n"], rowptr=lp["rowptr"], colind=lp["colind"], values=lp["values"], AL=AL[:, k], AU=AU[:, k],
                  l=L[:, k], u=U[:, k], c=Cm[:, k])
        ratio, ok = float("nan"), None
        if cert["kind"][k] == 1:
            D, V = primal_ray_test(mk, cert["y"][:, k])
            ratio, ok = V / D, D > 0 and V <= eps * D
        elif cert["kind"][k] == 2:
            cd, W = dual_ray_test(mk, cert["d"][:, k])
            ratio, ok = W / -cd, cd < 0 and W <= eps * -cd
        if ok is not None:
            worst = max(worst, ratio)
        print(f"[detect_batched_ab] member {k:2d}: {r['status'][k]:17s} iteration {int(r['iter'][k]):6d}  kkt {r['residuals'][k]:.2e}  "
              f"numpy ratio {ratio:.2e} passes {ok}", flush=True)
    print(f"[detect_batched_ab] unclamped eps {eps:g}: worst numpy ratio of the certificates {worst:.2e}", flush=True)


def trace():
    from test_gpu_batched_detect import MIXED_PRM, _mixed
    members, model, panels = _mixed(64)
    r = H.solve_batched_detect(model, *panels, None, H.Parameters(**MIXED_PRM))
    print(f"[detect_batched_ab] trace: statuses {dict(collections.Counter(r['status']))}, last iteration {int(np.max(r['iter']))}, "
          f"evaluations {int(np.max(r['iter'])) // 150}", flush=True)
    model.free()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    a = sys.argv[2:]
    if what == "cost":
        cost(int(a[0]) if a else 3)
    elif what == "unclamped":
        unclamped(int(a[0]) if a else 60000, tuple(float(e) for e in a[1:]) or (1e-8,))
    else:
        trace()
