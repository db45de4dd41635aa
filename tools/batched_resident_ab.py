"""Resident batches (DESIGN.md "Resident batches"): a sequence of batches over one matrix, call by call against one handle.

  python tools/batched_resident_ab.py [c4|planted|all] [--out FILE]
      c4: config 4's recipe (lpgen.c3_pds20_like(), B = 64, make_batch), tol 1e-4; planted: the 300 x 400 planted network LP of
      tests/test_gpu_warm.py at B = 8, tol 1e-6.  A base batch, then six more, C multiplied by 1 + 1e-3 N at every step.
      Path A: solve_batched_warm from path A's previous result (the base: solve_batched).  Path B: one BatchedSolver, carry=True
      (the base: a cold solve on the fresh handle).  The paths alternate in one process, A then B at every step; the base pair is
      the warm-up and is listed apart.  Per path: median, minimum and maximum over the six steps of the whole-call wall time and
      of the phases each path reports (A: setup_time / solve_time of the results; B: hprlp_batched_solver_seconds).  Every step's
      results are compared bit for bit (status, iter, x, y, z, primal_obj, residuals, gap).
The table goes to stdout and to FILE (default profiles/batched_resident_ab.txt); the library's own log goes to stderr.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = 6


def make_batch(lp, B, seed):  # (tests/test_gpu_batched.py's recipe)
    rng = np.random.default_rng(seed)
    m, n = lp["m"], lp["n"]
    Cm = lp["c"][:, None] * (1 + 0.1 * rng.normal(size=(n, B)))
    AU = lp["AU"][:, None] + np.abs(rng.normal(scale=0.1, size=(m, B)))
    AL = np.repeat(lp["AL"][:, None], B, axis=1)
    AL = np.where(np.isfinite(AL), np.minimum(AL, AU), AL)
    L = np.repeat(lp["l"][:, None], B, axis=1)
    U = np.repeat(lp["u"][:, None], B, axis=1)
    U = np.where(np.isfinite(U), U, 50.0)
    return Cm, AL, AU, L, U


def same(a, b):
    return (a["status"] == b["status"] and list(a["iter"]) == list(b["iter"])
            and all(np.array_equal(a[f], b[f]) for f in ("x", "y", "z", "primal_obj", "residuals", "gap")))


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def one(H, name, lp, B, seed, tol, lines):
    say = lambda s: (lines.append(s), print(s, flush=True))
    Cm, AL, AU, L, U = make_batch(lp, B, seed)
    model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=tol, max_iter=200000, use_presolve=False)
    rng = np.random.default_rng(40)
    # the base pair: warm-up of both paths (code objects, allocator cache), and what step 1 starts from
    t0 = time.perf_counter()
    ra = H.solve_batched(model, Cm, AL, AU, L, U, None, prm)
    ta = time.perf_counter() - t0
    t0 = time.perf_counter()
    h = H.BatchedSolver(model, prm)
    t_create = time.perf_counter() - t0
    rb = h.solve(Cm, AL, AU, L, U)
    tb = time.perf_counter() - t0
    sec = h.seconds()
    say(f"[batched_resident_ab] {name} ({lp['m']} x {lp['n']}, B = {B}, tol {tol:g}); base batch (cold, the warm-up pair): A solve_batched "
        f"{ta:.4f} s (set-up {ra['setup_time']:.4f}, loop {ra['solve_time']:.4f}), B create {t_create:.4f} s (set-up + scaling "
        f"{sec['create_setup']:.4f}, power iteration {sec['create_power']:.4f}) + solve {tb - t_create:.4f} s (prep {sec['prep']:.4f}, upload + "
        f"panels + start {sec['upload']:.4f}, loop {sec['loop']:.4f}, results {sec['results']:.4f}); iterations max {int(max(ra['iter']))}; "
        f"bits {'equal' if same(ra, rb) else 'DIFFER'}")
    A = dict(call=[], setup=[], loop=[])
    Bt = dict(call=[], prep=[], upload=[], loop=[], results=[])
    equal = True
    for step in range(1, STEPS + 1):
        Cm = Cm * (1 + 1e-3 * rng.normal(size=Cm.shape))
        t0 = time.perf_counter()
        ra = H.solve_batched_warm(model, Cm, AL, AU, L, U, ra["x"], ra["y"], None, prm)
        A["call"].append(time.perf_counter() - t0)
        A["setup"].append(ra["setup_time"]); A["loop"].append(ra["solve_time"])
        t0 = time.perf_counter()
        rb = h.solve(Cm, AL, AU, L, U, carry=True)
        Bt["call"].append(time.perf_counter() - t0)
        sec = h.seconds()
        for k in ("prep", "upload", "loop", "results"):
            Bt[k].append(sec[k])
        ok = same(ra, rb)
        equal = equal and ok
        say(f"[batched_resident_ab] {name} step {step}: iterations max {int(max(ra['iter']))} mean {float(np.mean(ra['iter'])):.0f}; "
            f"A {A['call'][-1]:.4f} s, B {Bt['call'][-1]:.4f} s; bits {'equal' if ok else 'DIFFER'}")
    info = h.info()
    say(f"[batched_resident_ab] {name} over {STEPS} steps, seconds, median (min .. max):")
    say(f"[batched_resident_ab]   A solve_batched_warm from the previous result: whole call {spread(A['call'])}; set-up {spread(A['setup'])}; "
        f"loop {spread(A['loop'])}")
    say(f"[batched_resident_ab]   B one handle, carry: whole call {spread(Bt['call'])}; host prep {spread(Bt['prep'])}; upload + panels + start "
        f"{spread(Bt['upload'])}; loop {spread(Bt['loop'])}; results {spread(Bt['results'])}")
    say(f"[batched_resident_ab]   B / A median whole call {statistics.median(Bt['call']) / statistics.median(A['call']):.3f}; all steps' bits "
        f"{'equal' if equal else 'DIFFER'}; handle: {info}")
    h.close()
    model.free()


def main(argv):
    what = argv[1] if len(argv) > 1 and not argv[1].startswith("--") else "all"
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "batched_resident_ab.txt")
    if what not in ("c4", "planted", "all"):
        sys.exit(__doc__)
    from conftest import hprlp as H, lpgen
    lines = []
    if what in ("planted", "all"):
        one(H, "planted 300 x 400", lpgen.planted_lp(300, 400, 2400, 7, values="network"), 8, 2, 1e-6, lines)
    if what in ("c4", "all"):
        one(H, "config 4", lpgen.c3_pds20_like(), 64, 4, 1e-4, lines)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
