"""Many small LPs at once (DESIGN.md "Many small LPs"): K sequential HPRLP_main_solve calls -- what a caller with K different
small LPs does without the group path -- against one hprlp_solve_many of the same K models.

  python tools/many_ab.py [--ks 1,16,64,256] [--repeats 3] [--tol 1e-4] [--modes solve,prepared] [--sides both|many]
                          [--out profiles/many_ab.txt]

Cases: (a) the 25fv47-like LP of BASELINE config 2 (821 x 1571, 10 700 nonzeros, kernel class <12, 2>) with K value seeds,
(b) the (300, 500, 2500) planted shape (class <4, 1>) with K seeds.  Same process, same box, order A/B/A/B...: per K one
unmeasured warm-up pair, then `repeats` measured pairs; the table gives the median whole-call wall time (host clock around calls
that end in a device wait) with the spread, and the phases of the median run: set-up + scaling, power iteration, loop + collect,
teardown (sequential: sums of hprlp_last_solve_phases over the K calls; group: hprlp_last_solve_many_phases).  The results of the
two sides are compared member by member (status, iterations, x): they must be the same bits.  A host without a GPU fails.

Mode `prepared` is the resident use: K handles prepared once (Solver.prepare), then per run every handle is reset and initialised
(unmeasured) and the timed part is K Solver.run calls (seq) against ONE Solver.run_many (many) -- no set-up, no teardown: the
rounds are the whole cost.  The last column gives the counts of hprlp_last_run_many_counts (rounds waits group-launches copies
own served; "-" where the library has no such entry) and a digest of the group side's results (status, iterations, x of every
member), so that two libraries -- HPRLP_LIB, as tools/ab_libs.sh -- can be compared run by run: one process per library, order
A/B/A/B.  --sides many leaves the sequential side out (nothing to compare the bits with inside the process: the digest stands in).
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
                       "rounds": p["rounds"], "waits": p["waits"], "launches": p["launches"], "counts": counts_text(H), "digest": digest(res)}


def digest(results):
    h = hashlib.sha1()
    for r in results:
        h.update(f"{r.status} {r.iter} ".encode())
        h.update(np.ascontiguousarray(r.x).tobytes())
    return h.hexdigest()[:12]


def counts_text(H):
    if not hasattr(H, "last_run_many_counts") or not hasattr(H.lib(), "hprlp_last_run_many_counts"):
        return "-"
    c = H.last_run_many_counts()
    return " ".join(str(c[k]) for k in ("rounds", "waits", "group_launches", "copies", "own", "served"))


def rearm(solvers):
    """Every prepared handle back to its start: iterates to zero, sigma and lambda as after prepare()."""
    for s in solvers:
        lam = s.scalars()["lambda_max"]
        s.reset()
        s.init(-1.0, lam)


def prepared_sequential(H, solvers):
    rearm(solvers)
    t0 = time.perf_counter()
    res = [s.run(max_trace=1) for s in solvers]
    wall = time.perf_counter() - t0
    return res, wall, {"setup+scaling": 0.0, "power": 0.0, "loop+collect": wall, "teardown": 0.0}


def prepared_grouped(H, solvers):
    rearm(solvers)
    t0 = time.perf_counter()
    res = H.Solver.run_many(solvers)
    wall = time.perf_counter() - t0
    return res, wall, {"setup+scaling": 0.0, "power": 0.0, "loop+collect": wall, "teardown": 0.0, "counts": counts_text(H), "digest": digest(res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--modes", default="solve,prepared")
    ap.add_argument("--sides", default="both", choices=("both", "many"))
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
             f"# library {H.LIB_PATH}",
             "# mode | case | K | side | whole call | set-up + scaling | power iteration | loop + collect | teardown | rounds waits launches | "
             "counts (rounds waits group-launches copies own served) | digest"]
    both = a.sides == "both"
    for mode, (name, gen) in [(mo, c) for mo in a.modes.split(",") for c in cases.items()]:
        models = []
        for seed in range(100, 100 + max(ks)):
            lp = gen(seed)
            models.append(H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"],
                                           lp["c"]))
        solvers = []
        if mode == "prepared":
            with quiet():
                for m in models:
                    solvers.append(H.Solver(m, prm))
                    solvers[-1].prepare()
        for K in ks:
            runs = {"seq": [], "many": []}
            same = True
            for rep in range(a.repeats + 1):
                with quiet():
                    if both:
                        rs, ws, ps = sequential(H, models[:K], prm) if mode == "solve" else prepared_sequential(H, solvers[:K])
                    rm, wm, pm = grouped(H, models[:K], prm) if mode == "solve" else prepared_grouped(H, solvers[:K])
                if both:
                    same = same and all(x.status == y.status and x.iter == y.iter and np.array_equal(x.x, y.x) for x, y in zip(rs, rm))
                if rep > 0:
                    if both:
                        runs["seq"].append((ws, ps))
                    runs["many"].append((wm, pm))
            iters = [r.iter for r in rm]
            for side in ("seq", "many") if both else ("many",):
                walls = sorted(w for w, _ in runs[side])
                med = statistics.median_low(walls)
                p = next(pp for w, pp in runs[side] if w == med)
                loops = sorted(pp["loop+collect"] for _, pp in runs[side])
                extra = f"{int(p['rounds'])} {int(p['waits'])} {int(p['launches'])}" if "rounds" in p else "-"
                lines.append(f"{mode} | {name} | {K} | {side} | {med:.4f} [{walls[0]:.4f} .. {walls[-1]:.4f}] | {p['setup+scaling']:.4f} | {p['power']:.4f} | "
                             f"{p['loop+collect']:.4f} [{loops[0]:.4f} .. {loops[-1]:.4f}] | {p['teardown']:.4f} | {extra} | {p.get('counts', '-')} | "
                             f"{p.get('digest', '-')}")
            mm = statistics.median_low(sorted(w for w, _ in runs["many"]))
            if both:
                ms = statistics.median_low(sorted(w for w, _ in runs["seq"]))
                lines.append(f"#   K = {K}: seq / many = {ms / mm:.2f}; iterations {min(iters)} .. {max(iters)}; results bit-identical: {same}")
            else:
                lines.append(f"#   K = {K}: iterations {min(iters)} .. {max(iters)}")
            print("\n".join(lines[-3:]), flush=True)
        for s_ in solvers:
            s_.close()
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
