"""Many small LPs at once (DESIGN.md "Many small LPs"): K sequential HPRLP_main_solve calls -- what a caller with K different
small LPs does without the group path -- against one hprlp_solve_many of the same K models.

  python tools/many_ab.py [--ks 1,16,64,256] [--repeats 3] [--tol 1e-4] [--out profiles/many_ab.txt]

Cases: (a) the 25fv47-like LP of BASELINE config 2 (821 x 1571, 10 700 nonzeros, kernel class <12, 2>) with K value seeds,
(b) the (300, 500, 2500) planted shape (class <4, 1>) with K seeds.  Same process, same box, order A/B/A/B...: per K one
unmeasured warm-up pair, then `repeats` measured pairs; the table gives the median whole-call wall time (host clock around calls
that end in a device wait) with the spread, and the phases of the median run: set-up + scaling, power iteration, loop + collect,
teardown (sequential: sums of hprlp_last_solve_phases over the K calls; group: hprlp_last_solve_many_phases).  The results of the
two sides are compared member by member (status, iterations, x): they must be the same bits.  A host without a GPU fails.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class quiet:
    """The library's banner and summary (stdout of the C side) go to /dev/null for the duration."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        self.null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(self.null, 1)

    def __exit__(self, *a):
        os.dup2(self.saved, 1)
        os.close(self.saved)
        os.close(self.null)


def sequential(H, models, prm):
    """K HPRLP_main_solve calls one after another; phases summed."""
    L = H.lib()
    cp = prm.to_c()
    ph = np.zeros(8)
    tot = np.zeros(8)
    res = []
    t0 = time.perf_counter()
    for m in models:
        r = L.HPRLP_main_solve(m._ptr, C.byref(cp))
        L.hprlp_last_solve_phases(ph.ctypes.data_as(H.c_dbl_p))
        tot += ph
        res.append(H.Results(r, m.m, m.n))
    wall = time.perf_counter() - t0
    return res, wall, {"setup+scaling": tot[0] + tot[1], "power": tot[2], "loop+collect": tot[3] + tot[4], "teardown": tot[5]}


def grouped(H, models, prm):
    t0 = time.perf_counter()
    res = H.solve_many(models, prm)
    wall = time.perf_counter() - t0
    p = H.last_solve_many_phases()
    rest = p["call"] - p["setup"] - p["scaling"] - p["power"] - p["loop"]
    return res, wall, {"setup+scaling": p["setup"] + p["scaling"], "power": p["power"], "loop+collect": p["loop"], "teardown": rest,
                       "rounds": p["rounds"], "waits": p["waits"], "launches": p["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from conftest import hprlp as H, lpgen
    L = H.lib()
    L.hprlp_last_solve_phases.argtypes = [H.c_dbl_p]
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_ab] no GPU: " + H.last_error())
    ks = [int(k) for k in a.ks.split(",")]
    prm = H.Parameters(stop_tol=a.tol, use_presolve=False)
    cases = {"c2_25fv47_like <12,2>": lambda seed: lpgen.c2_25fv47_like(seed=seed),
             "planted 300x500x2500 <4,1>": lambda seed: lpgen.planted_lp(300, 500, 2500, seed)}
    lines = [f"# tools/many_ab.py: K sequential HPRLP_main_solve calls (seq) against one hprlp_solve_many (many); stop_tol {a.tol:g}, no presolve,",
             f"# one process, A/B/A/B, {a.repeats} measured pairs after one warm-up pair; seconds, median [min .. max]; phases of the median run",
             "# case | K | side | whole call | set-up + scaling | power iteration | loop + collect | teardown | rounds waits launches"]
    for name, gen in cases.items():
        models = []
        for seed in range(100, 100 + max(ks)):
            lp = gen(seed)
            models.append(H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"],
                                           lp["c"]))
        for K in ks:
            runs = {"seq": [], "many": []}
            same = True
            for rep in range(a.repeats + 1):
                with quiet():
                    rs, ws, ps = sequential(H, models[:K], prm)
                    rm, wm, pm = grouped(H, models[:K], prm)
                same = same and all(x.status == y.status and x.iter == y.iter and np.array_equal(x.x, y.x) for x, y in zip(rs, rm))
                if rep > 0:
                    runs["seq"].append((ws, ps))
                    runs["many"].append((wm, pm))
            iters = [r.iter for r in rm]
            for side in ("seq", "many"):
                walls = sorted(w for w, _ in runs[side])
                med = statistics.median_low(walls)
                p = next(pp for w, pp in runs[side] if w == med)
                extra = f"{int(p['rounds'])} {int(p['waits'])} {int(p['launches'])}" if side == "many" else "-"
                lines.append(f"{name} | {K} | {side} | {med:.4f} [{walls[0]:.4f} .. {walls[-1]:.4f}] | {p['setup+scaling']:.4f} | {p['power']:.4f} | "
                             f"{p['loop+collect']:.4f} | {p['teardown']:.4f} | {extra}")
            ms, mm = statistics.median_low(sorted(w for w, _ in runs["seq"])), statistics.median_low(sorted(w for w, _ in runs["many"]))
            lines.append(f"#   K = {K}: seq / many = {ms / mm:.2f}; iterations {min(iters)} .. {max(iters)}; results bit-identical: {same}")
            print("\n".join(lines[-3:]), flush=True)
        for m in models:
            m.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
