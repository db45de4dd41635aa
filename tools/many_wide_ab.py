"""Wide members of a group of LPs (DESIGN.md "Many small LPs", wide members): K resident solvers past the single-workgroup size,
run three ways in one process.

  python tools/many_wide_ab.py [--shapes mid,large,c3] [--rounds 3] [--tol 1e-4] [--max-iter 2000] [--out profiles/many_wide_ab.txt]

Mode `prepared` of tools/many_ab.py: K handles are prepared once (Solver.prepare); before every timed call each handle is reset and
initialised, unmeasured.  The three sides alternate A B C A B C ...:
  (A) K Solver.run calls, one after another -- each member alone, its normal iterations as graph replays;
  (B) one Solver.run_many with the setting off -- the members issue their own launches inside the lock-step;
  (C) one Solver.run_many with Solver.set_group_wide() on every member -- the normal iterations in group launches.
One unmeasured warm-up round, then `rounds` measured ones; the table gives the median wall time of the call with its spread (a host
clock around calls that end in a device wait).  The results of the three sides are compared member by member -- status,
iterations and x, bit for bit -- in every round.  The last columns time Solver.power_iteration_many on the same handles with the
setting off and on (lambda and the iteration count compared as well).  max_iter bounds every solve: the quantity of interest is
the cost of an iteration, and a member that reaches the tolerance earlier leaves its group as it would anyway.
A host without a GPU fails."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from many_ab import quiet, rearm  # noqa: E402

SHAPES = {
    "mid": ("planted_lp(2500, 4000, 15000)", lambda g, seed: g.planted_lp(2500, 4000, 15000, seed), (1, 4, 16, 64)),
    "large": ("planted_lp(20000, 30000, 150000)", lambda g, seed: g.planted_lp(20000, 30000, 150000, seed), (1, 4, 16)),
    "c3": ("lpgen.c3_pds20_like() 33874 x 105728", lambda g, seed: g.c3_pds20_like(seed=seed), (1, 2, 4, 8)),
}


def same(a, b):
    return all(x.status == y.status and x.iter == y.iter and np.array_equal(x.x, y.x) for x, y in zip(a, b))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def spread(walls):
    walls = sorted(walls)
    return statistics.median_low(walls), f"{statistics.median_low(walls):.4f} [{walls[0]:.4f} .. {walls[-1]:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mid,large,c3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from conftest import hprlp as H, lpgen
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_wide_ab] no GPU: " + H.last_error())
    prm = H.Parameters(stop_tol=a.tol, use_presolve=False, max_iter=a.max_iter)
    lines = [f"# tools/many_wide_ab.py: K prepared solvers; (A) K Solver.run, (B) run_many, setting off, (C) run_many, every member wide;",
             f"# stop_tol {a.tol:g}, max_iter {a.max_iter}, no presolve; one process, A B C alternating, {a.rounds} measured rounds after one warm-up round;",
             "# seconds, median [min .. max], host clock around calls that end in a device wait; power: power_iteration_many, setting off / on",
             "# shape | K | joined | iterations | A | B | C | A / C | B / C | bits A = B = C | wide counts of C (normal launches, segments, member-iterations) | "
             "power off | power on | off / on | power bits equal"]
    for key in a.shapes.split(","):
        name, gen, ks = SHAPES[key]
        models, solvers = [], []
        with quiet():
            for seed in range(100, 100 + max(ks)):
                lp = gen(lpgen, seed)
                models.append(H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"],
                                               lp["c"]))
                solvers.append(H.Solver(models[-1], prm))
                solvers[-1].prepare()
        print(f"[many_wide_ab] {name}: {solvers[0].describe()}", flush=True)
        lines.append(f"# {name}: {solvers[0].describe()}")
        for K in ks:
            group = solvers[:K]
            walls = {"A": [], "B": [], "C": [], "P0": [], "P1": []}
            bits = power_bits = True
            joined = 0
            for rnd in range(a.rounds + 1):
                with quiet():
                    for s in group:
                        s.set_group_wide(False)
                    rearm(group)
                    ra, wa = timed(lambda: [s.run(max_trace=1) for s in group])
                    rearm(group)
                    rb, wb = timed(lambda: H.Solver.run_many(group))
                    p0, wp0 = timed(lambda: H.Solver.power_iteration_many(group))
                    joined = sum(bool(s.set_group_wide(True)) for s in group)
                    rearm(group)
                    rc, wc = timed(lambda: H.Solver.run_many(group))
                    counts = H.last_many_wide_counts()
                    p1, wp1 = timed(lambda: H.Solver.power_iteration_many(group))
                bits = bits and same(ra, rb) and same(ra, rc)
                power_bits = power_bits and p0 == p1
                if rnd > 0:
                    for k, w in zip(("A", "B", "C", "P0", "P1"), (wa, wb, wc, wp0, wp1)):
                        walls[k].append(w)
            med = {k: spread(v) for k, v in walls.items()}
            iters = [r.iter for r in rc]
            lines.append(f"{name} | {K} | {joined} | {min(iters)} .. {max(iters)} | {med['A'][1]} | {med['B'][1]} | {med['C'][1]} | "
                         f"{med['A'][0] / med['C'][0]:.2f} | {med['B'][0] / med['C'][0]:.2f} | {bits} | "
                         f"{counts['normal_launches']} {counts['segments']} {counts['member_iterations']} | {med['P0'][1]} | {med['P1'][1]} | "
                         f"{med['P0'][0] / med['P1'][0]:.2f} | {power_bits}")
            print(lines[-1], flush=True)
        for s in solvers:
            s.close()
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
