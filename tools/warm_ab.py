"""Warm start (DESIGN.md "Warm start"): cold against warm re-solves, by iterations and wall time.

  python tools/warm_ab.py resolve [tol]      configs 2 and 3 and two lpgen families: c, and AL / AU, perturbed by a relative 1e-3 and
                                             1e-2; the perturbed LP solved cold and warm from the unperturbed answer
  python tools/warm_ab.py batched [tol]      config 4 (B = 64): C perturbed by a relative 1e-3, re-solved cold and warm from the previous
                                             batch's X / Y
  python tools/warm_ab.py c5 [reps]          config 5: what the start adds (upload, projection, the two SpMVs of the iteration-0
                                             evaluation), hprlp_last_solve_phases()[7], on a solve capped at a few iterations
  python tools/warm_ab.py probe [tol]        planted LPs (the shapes tests/test_gpu_warm.py may use): c perturbed by 1e-3, cold and warm
One line per measurement on stdout ("[warm_ab] ..."); the library's own log goes to stderr.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _quiet():
    """The library prints its log on fd 1: send it to stderr, keep our lines on a private copy of stdout."""
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)
    return out


def _model(H, lp):
    return H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])


def perturb(lp, what, eps, seed):
    rng = np.random.default_rng(seed)
    out = dict(lp)
    if what == "c":
        out["c"] = lp["c"] * (1 + eps * rng.normal(size=lp["n"]))
    else:  # the same positive factor on both sides of a row keeps AL <= AU
        f = 1 + eps * rng.normal(size=lp["m"])
        f = np.maximum(f, 0.5)
        out["AL"] = np.where(np.isfinite(lp["AL"]), lp["AL"] * f, lp["AL"])
        out["AU"] = np.where(np.isfinite(lp["AU"]), lp["AU"] * f, lp["AU"])
    return out


def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def resolve_one(H, out, name, lp, tol, whats=("c", "bounds"), epss=(1e-3, 1e-2)):
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=500000, time_limit=30.0)
    model = _model(H, lp)
    base = model.solve(prm)
    model.free()
    for what in whats:
        for eps in epss:
            lp2 = perturb(lp, what, eps, 7)
            m2 = _model(H, lp2)
            cold, tc = _timed(lambda: m2.solve(prm))
            warm, tw = _timed(lambda: m2.solve_warm(base.x, base.y, prm))
            print(f"[warm_ab] {name} ({lp['m']} x {lp['n']}) {what} x(1 + {eps:g} N) tol {tol:g}: base {base.status} {base.iter}; "
                  f"cold {cold.status} {cold.iter} it {tc:.3f} s; warm {warm.status} {warm.iter} it {tw:.3f} s; "
                  f"iterations warm/cold {warm.iter / max(cold.iter, 1):.3f}", file=out)
            m2.free()


def resolve(tol=1e-6):
    from conftest import hprlp as H, lpgen
    out = _quiet()
    cases = {"config 2": lpgen.c2_25fv47_like(), "config 3": lpgen.c3_pds20_like(),
             "pds_like": lpgen.FAMILIES_SMALL["pds_like"](), "staircase": lpgen.FAMILIES_SMALL["staircase"]()}
    for name, lp in cases.items():
        resolve_one(H, out, name, lp, tol)


def probe(tol=1e-6):
    from conftest import hprlp as H, lpgen
    out = _quiet()
    for shape in ((300, 400, 2400), (1000, 1500, 6000), (2000, 3000, 16000)):
        for values in ("network", "general"):
            for seed in (11, 12, 13, 14):
                lp = lpgen.planted_lp(*shape, seed, values=values)
                resolve_one(H, out, f"planted {values} seed {seed}", lp, tol, whats=("c",), epss=(1e-3,))


def batched(tol=1e-4):
    from conftest import hprlp as H, lpgen
    from test_gpu_warm import make_batch
    out = _quiet()
    lp = lpgen.c3_pds20_like()
    B = 64
    Cm, AL, AU, L, U = make_batch(lp, B, 4)
    model = _model(H, lp)
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=200000, time_limit=300.0)
    r0, t0 = _timed(lambda: H.solve_batched(model, Cm, AL, AU, L, U, None, prm))
    for eps in (1e-3, 1e-2):
        C2 = Cm * (1 + eps * np.random.default_rng(40).normal(size=Cm.shape))
        cold, tc = _timed(lambda: H.solve_batched(model, C2, AL, AU, L, U, None, prm))
        warm, tw = _timed(lambda: H.solve_batched_warm(model, C2, AL, AU, L, U, r0["x"], r0["y"], None, prm))
        it = lambda r: (int(np.max(r["iter"])), float(np.mean(r["iter"])))
        opt = lambda r: sum(s == "OPTIMAL" for s in r["status"])
        print(f"[warm_ab] config 4 (B = {B}) C x(1 + {eps:g} N) tol {tol:g}: first solve {t0:.3f} s; cold {opt(cold)} OPTIMAL, "
              f"iterations max/mean {it(cold)[0]}/{it(cold)[1]:.0f}, {tc:.3f} s; warm {opt(warm)} OPTIMAL, iterations max/mean "
              f"{it(warm)[0]}/{it(warm)[1]:.0f}, {tw:.3f} s", file=out)
    model.free()


def c5(reps=3):
    import bench as B
    H = B.H
    out = _quiet()
    m, n, per_row, band = B.WORKLOADS["c5"]
    lp = B.banded_lp(m, n, per_row, band)
    model = _model(H, lp)
    prm = H.Parameters(stop_tol=1e-4, use_presolve=False, max_iter=10, time_limit=300.0)
    rng = np.random.default_rng(1)
    x0, y0 = rng.random(n), rng.normal(size=m)
    for rep in range(reps):
        for mode in ("cold", "warm"):
            r = model.solve(prm) if mode == "cold" else model.solve_warm(x0, y0, prm)
            ph = H.last_solve_phases()
            L = H.lib()
            import ctypes as C
            raw = (C.c_double * 8)()
            L.hprlp_last_solve_phases(raw)
            print(f"[warm_ab] config 5 ({m} x {n}) rep {rep} {mode}: {r.status} {r.iter} it; set-up {ph['device_setup']:.4f} s, "
                  f"loop {ph['loop']:.4f} s, whole call {ph['whole_call']:.4f} s, start {raw[7]:.4f} s", file=out)
    model.free()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "resolve"
    a = sys.argv[2:]
    if what == "resolve":
        resolve(float(a[0]) if a else 1e-6)
    elif what == "probe":
        probe(float(a[0]) if a else 1e-6)
    elif what == "batched":
        batched(float(a[0]) if a else 1e-4)
    elif what == "c5":
        c5(int(a[0]) if a else 3)
    else:
        sys.exit(__doc__)
