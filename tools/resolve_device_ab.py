"""Device-resident re-solve (DESIGN.md "Device-resident re-solve"): the host entry against the tensor entry of a resident solver.

  python tools/resolve_device_ab.py [small|c5|all] [--out FILE]
      small: config 2 and config 3 (lpgen.c2_25fv47_like(), lpgen.c3_pds20_like(), tol 1e-6); c5: config 5 (bench.py's workload,
      tol 1e-4); all: the three.  Two solvers are prepared on the model and run once.  Then a sequence of STEPS steps: c multiplied
      by 1 + 1e-3 N, set_data of the new c, resolve from the previous step's solution.
      Path H: Solver.set_data + Solver.resolve, numpy in, numpy out.  Path D: Solver.set_data_tensors + Solver.resolve_tensors on
      the second solver, the step's c and the previous x, y on the GPU before the clock starts, x / y / z left there.  The paths
      alternate in one process, H then D at every step; the first pair is the warm-up and is listed apart.  Per path: median,
      minimum and maximum over the steps of the whole step's wall time (both calls, ending in the call's own wait for the solver's
      stream), of the slots of hprlp_solver_data_seconds, of set_data and resolve apart, and the bytes of hprlp_solver_transfer
      for both calls.  Every step's status, iter and the bits of x, y, z are compared.  A step's results are released after both
      windows have closed (see the comment in one()).
The table goes to stdout and to FILE (default profiles/resolve_device_ab.txt); the library's own log goes to stderr.
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

from warm_ab import _model, _quiet  # noqa: E402

STEPS = 5
SLOTS = ("upload", "kernels", "total")


def spread(v):
    return "%.5f (%.5f .. %.5f)" % (statistics.median(v), min(v), max(v))


def one(H, say, name, lp, tol, time_limit):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=500000, time_limit=time_limit)
    model = _model(H, lp)
    solvers = []
    for _ in range(2):
        s = H.Solver(model, prm)
        H.lib().hprlp_solver_set_verbose(s.h, 0)
        s.prepare()
        solvers.append(s)
    sh, sd = solvers
    bh, bd = sh.run(), sd.run()
    x, y = bh.x, bh.y
    tx, ty = dev(bd.x), dev(bd.y)
    say(f"[resolve_device_ab] {name} ({lp['m']} x {lp['n']}, {len(lp['values'])} entries) tol {tol:g}: base run {bh.status} {bh.iter} it; "
        f"kernel forms: {sh.describe()}")
    rng = np.random.default_rng(40)
    c = lp["c"]
    acc = {p: dict(step=[], set_data=[], resolve=[], **{k: [] for k in SLOTS}) for p in "HD"}
    bytes_ = {}
    equal = True
    rh, rd = bh, bd
    for step in range(STEPS + 1):   # (step 0: the warm-up pair)
        # The previous step's results stay alive until both windows are closed: giving a host entry's malloc'ed x / y / z back to
        # the system (munmap of memory the runtime had pinned for the download) stalls the process's next GPU work for
        # milliseconds, and that belongs to neither window.  It happens at the end of the step, before the synchronize below.
        keep = (rh, rd)
        c = c * (1 + 1e-3 * rng.normal(size=lp["n"]))
        tc = dev(c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sh.set_data(c=c)
        t1 = time.perf_counter()
        trh = sh.transfer()
        rh = sh.resolve(x, y)
        t2 = time.perf_counter()
        th = (t2 - t0, t1 - t0, t2 - t1)
        bytes_["H"] = (trh["h2d_bytes"], trh["d2h_bytes"], sh.transfer()["h2d_bytes"], sh.transfer()["d2h_bytes"])
        dsh = sh.data_seconds()
        t0 = time.perf_counter()
        sd.set_data_tensors(c=tc)
        t1 = time.perf_counter()
        trd = sd.transfer()
        rd = sd.resolve_tensors(tx, ty)
        t2 = time.perf_counter()
        td = (t2 - t0, t1 - t0, t2 - t1)
        bytes_["D"] = (trd["h2d_bytes"], trd["d2h_bytes"], sd.transfer()["h2d_bytes"], sd.transfer()["d2h_bytes"])
        dsd = sd.data_seconds()
        ok = ((rh.status, rh.iter) == (rd.status, rd.iter)
              and all(np.array_equal(getattr(rh, f), getattr(rd, f).cpu().numpy()) for f in ("x", "y", "z")))
        equal = equal and ok
        say(f"[resolve_device_ab] {name} step {step}{' (warm-up pair)' if step == 0 else ''}: {rh.status} {rh.iter} it; H {th[0]:.5f} s "
            f"(set_data {th[1]:.5f}, resolve {th[2]:.5f}), D {td[0]:.5f} s (set_data {td[1]:.5f}, resolve {td[2]:.5f}); "
            f"status, iter, bits {'equal' if ok else 'DIFFER'}")
        if step > 0:
            for p, t, ds in (("H", th, dsh), ("D", td, dsd)):
                acc[p]["step"].append(t[0]); acc[p]["set_data"].append(t[1]); acc[p]["resolve"].append(t[2])
                for k in SLOTS:
                    acc[p][k].append(ds[k])
        x, y, tx, ty = rh.x, rh.y, rd.x, rd.y
        del keep
    say(f"[resolve_device_ab] {name} over {STEPS} steps, seconds, median (min .. max):")
    for p, tag in (("H", "H host entry, numpy in / out"), ("D", "D tensor entry, tensors in / out")):
        a = acc[p]
        say(f"[resolve_device_ab]   {tag}: whole step {spread(a['step'])}; set_data {spread(a['set_data'])}; resolve {spread(a['resolve'])}; "
            + "data_seconds " + "; ".join(f"{k} {spread(a[k])}" for k in SLOTS)
            + "; transfer bytes set_data in / out %d / %d, resolve in / out %d / %d" % bytes_[p])
    say(f"[resolve_device_ab]   D / H median whole step {statistics.median(acc['D']['step']) / statistics.median(acc['H']['step']):.3f}; "
        f"D - H median {statistics.median(acc['D']['step']) - statistics.median(acc['H']['step']):+.5f} s; all steps' status, iter and bits "
        f"{'equal' if equal else 'DIFFER'}")
    for s in solvers:
        s.close()
    model.free()


def main(argv):
    what = argv[1] if len(argv) > 1 and not argv[1].startswith("--") else "all"
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "resolve_device_ab.txt")
    if what not in ("small", "c5", "all"):
        sys.exit(__doc__)
    from conftest import hprlp as H, lpgen
    stdout = _quiet()
    lines = []
    say = lambda s: (lines.append(s), print(s, file=stdout, flush=True))
    if what in ("small", "all"):
        one(H, say, "config 2", lpgen.c2_25fv47_like(), 1e-6, 60.0)
        one(H, say, "config 3", lpgen.c3_pds20_like(), 1e-6, 60.0)
    if what in ("c5", "all"):
        import bench as B
        m, n, per_row, band = B.WORKLOADS["c5"]
        one(B.H, say, "config 5", B.banded_lp(m, n, per_row, band), 1e-4, 300.0)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv)
