"""Device-resident batches (DESIGN.md "Device-resident batches"): the host entry against the device entry of one resident solver.

  python tools/batched_device_ab.py [c4|planted|all] [--out FILE]
      c4: config 4's recipe (lpgen.c3_pds20_like(), B = 64, make_batch), tol 1e-4; planted: the 300 x 400 planted network LP of
      tests/test_gpu_warm.py at B = 8, tol 1e-6.  A base batch, then six more, C multiplied by 1 + 1e-3 N at every step, every
      step carried from the one before (the sequence of tools/batched_resident_ab.py).
      Path H: BatchedSolver.solve, numpy in, numpy out, on a handle with set_norms(1).  Path D: BatchedSolver.solve_tensors on a
      second handle, the step's tensors on the GPU before the clock starts, x / y / z left there.  The paths alternate in one
      process, H then D at every step; the base pair is the warm-up and is listed apart.  Per path: median, minimum and maximum
      over the six steps of the whole-call wall time and of the phases of hprlp_batched_solver_seconds (create: set-up and power
      iteration, once per handle; per call: prep, upload, loop, results), and the staging bytes of hprlp_batched_solver_transfer.
      Every step's results are compared bit for bit (status, iter, x, y, z, primal_obj, residuals, gap, the seven scalars).
The table goes to stdout and to FILE (default profiles/batched_device_ab.txt); the library's own log goes to stderr.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS = 6
PHASES = ("prep", "upload", "loop", "results")


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def same(H, rh, rd, sh, sd):
    return (rh["status"] == rd["status"] and list(rh["iter"]) == list(rd["iter"])
            and all(np.array_equal(rh[f], rd[f].cpu().numpy()) for f in ("x", "y", "z"))
            and all(np.array_equal(rh[f], rd[f]) for f in ("primal_obj", "residuals", "gap"))
            and all(np.array_equal(sh[k], sd[k]) for k in H.BATCH_SCALARS))


def one(H, name, lp, B, seed, tol, lines):
    import torch
    from batched_resident_ab import make_batch
    say = lambda s: (lines.append(s), print(s, flush=True))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda().T  # strides (1, rows): passed without a copy
    Cm, AL, AU, L, U = make_batch(lp, B, seed)
    model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=tol, max_iter=200000, use_presolve=False)
    rng = np.random.default_rng(40)
    hh, hd = H.BatchedSolver(model, prm), H.BatchedSolver(model, prm)
    hh.set_norms(1)
    tAL, tAU, tL, tU = dev(AL), dev(AU), dev(L), dev(U)

    def pair(Cm, carry):
        tC = dev(Cm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rh = hh.solve(Cm, AL, AU, L, U, carry=carry)
        th = time.perf_counter() - t0
        t0 = time.perf_counter()
        rd = hd.solve_tensors(tC, tAL, tAU, tL, tU, carry=carry)
        td = time.perf_counter() - t0
        return rh, th, rd, td, same(H, rh, rd, hh.scalars(), hd.scalars())

    rh, th, rd, td, ok = pair(Cm, False)
    sh, sd = hh.seconds(), hd.seconds()
    fmt = lambda s: ", ".join(f"{k} {s[k]:.4f}" for k in PHASES)
    say(f"[batched_device_ab] {name} ({lp['m']} x {lp['n']}, B = {B}, tol {tol:g}); base batch (cold, the warm-up pair): H {th:.4f} s "
        f"({fmt(sh)}), D {td:.4f} s ({fmt(sd)}); create H set-up {sh['create_setup']:.4f} power {sh['create_power']:.4f}, D set-up "
        f"{sd['create_setup']:.4f} power {sd['create_power']:.4f}; iterations max {int(max(rh['iter']))}; bits {'equal' if ok else 'DIFFER'}")
    Ht, Dt = dict(call=[], **{k: [] for k in PHASES}), dict(call=[], **{k: [] for k in PHASES})
    equal = ok
    for step in range(1, STEPS + 1):
        Cm = Cm * (1 + 1e-3 * rng.normal(size=Cm.shape))
        rh, th, rd, td, ok = pair(Cm, True)
        equal = equal and ok
        for acc, t, h in ((Ht, th, hh), (Dt, td, hd)):
            acc["call"].append(t)
            sec = h.seconds()
            for k in PHASES:
                acc[k].append(sec[k])
        say(f"[batched_device_ab] {name} step {step}: iterations max {int(max(rh['iter']))} mean {float(np.mean(rh['iter'])):.0f}; "
            f"H {th:.4f} s, D {td:.4f} s; bits {'equal' if ok else 'DIFFER'}")
    say(f"[batched_device_ab] {name} over {STEPS} steps, seconds, median (min .. max):")
    for tag, acc, h in (("H host entry, numpy in / out, tree rule", Ht, hh), ("D device entry, tensors in / out", Dt, hd)):
        say(f"[batched_device_ab]   {tag}: whole call {spread(acc['call'])}; " + "; ".join(f"{k} {spread(acc[k])}" for k in PHASES)
            + f"; outside the phases {spread([c - sum(acc[k][i] for k in PHASES) for i, c in enumerate(acc['call'])])}; staging {h.transfer()}")
    say(f"[batched_device_ab]   D / H median whole call {statistics.median(Dt['call']) / statistics.median(Ht['call']):.3f}; all steps' bits "
        f"{'equal' if equal else 'DIFFER'}")
    hh.close(); hd.close()
    model.free()


def main(argv):
    what = argv[1] if len(argv) > 1 and not argv[1].startswith("--") else "all"
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "batched_device_ab.txt")
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
