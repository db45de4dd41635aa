"""Group re-solve of many small LPs (DESIGN.md "Many small LPs", group re-solve): K resident solvers, R rounds of new c and new row
sides for every member, each round started from the previous round's solution --
  (a) member by member: set_data, reset, init, set_start for every member, then ONE run_many (what a caller does without the
      group entries), against
  (b) set_data_many + resolve_many.

  python tools/many_resolve_ab.py --lib-a PARENT/libhprlp.so [--lib-b lib/libhprlp.so] [--ks 1,16,64,256] [--rounds 20]
                                  [--passes 3] [--tol 1e-4] [--max-iter 20000] [--out profiles/many_resolve_ab.txt]

Protocol of tools/many_ab.py: side (a) runs on the library of --lib-a (the parent commit's build: the yardstick), side (b) on
--lib-b (this tree's), each through HPRLP_LIB in a process of its own -- one process per library and pass, order A/B/A/B, one
unmeasured warm-up pair, then `passes` measured pairs.  Per case and K a pass prepares the K solvers once (unmeasured), runs one
cold solve, then times the R rounds; the table gives the median over the passes [min .. max] of a round's mean seconds: the whole
round, the loop only and the rest (outside the loop = whole - loop), then the counts of hprlp_last_resolve_many_counts of the last
round and a digest of status, iterations and x of every member in every round -- it must be the same on both sides in every pass.
A host without a GPU fails.

The loop only is the group loop's wall time up to its last member's last event, read from out.time, which starts from a
different base on the two sides: side (a) ends in run_many, whose out.time = the member's power-iteration seconds (prepare() ran
one) + the loop, so the loop is the largest out.time - scalars()["power_time"]; side (b) ends in resolve_many, whose out.time =
the member's set_data seconds since its previous loop + the loop, so the loop is the largest out.time - data_seconds()["total"].
One bias remains and goes AGAINST side (b): its zeroing, bound codes, ctrl and start kernels are recorded and run in front of
the loop's first evaluation, after the loop's clock has started, so their GPU time is booked under "loop only", while side (a)
runs them before the clock starts and has them under "outside the loop".  The whole round has no such bias.

  python tools/many_resolve_ab.py --child member|group ...   is one pass (what the parent starts; prints one line per case and K).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def cases(lpgen):
    return {"c2_25fv47_like <12,2>": lambda seed: lpgen.c2_25fv47_like(seed=seed),
            "planted 300x500x2500 <4,1>": lambda seed: lpgen.planted_lp(300, 500, 2500, seed)}


def round_data(lp, rnd, k):
    """New c and new row sides of member k in round rnd: c moved by 1e-3 relative, the row sides moved OUTWARDS by at most
    1e-3 (1 + |side|), infinite sides stay -- the planted point stays feasible, so every round has a solution (sides moved at
    random make some members infeasible, and such a member iterates to its limits); l and u as they are."""
    rng = np.random.default_rng(1000 * rnd + k)
    m = lp["m"]
    AL, AU = np.asarray(lp["AL"], float), np.asarray(lp["AU"], float)
    return dict(c=lp["c"] * (1 + 1e-3 * rng.normal(size=lp["n"])), AL=AL - 1e-3 * rng.uniform(size=m) * (1 + np.abs(AL)),
                AU=AU + 1e-3 * rng.uniform(size=m) * (1 + np.abs(AU)), l=lp["l"], u=lp["u"])


def one_pass(side, ks, rounds, tol, max_iter):
    from many_ab import quiet
    from conftest import hprlp as H, lpgen
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_resolve_ab] no GPU: " + H.last_error())
    if side == "group" and not hasattr(L, "hprlp_solver_resolve_many"):
        sys.exit("[many_resolve_ab] the library of the group side has no hprlp_solver_resolve_many: " + H.LIB_PATH)
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=max_iter)   # (the limit bounds a round whatever the data does)
    for name, gen in cases(lpgen).items():
        lps = [gen(seed) for seed in range(100, 100 + max(ks))]
        models = [H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
                  for lp in lps]
        for K in ks:
            with quiet():
                solvers = [H.Solver(m, prm) for m in models[:K]]
                for s in solvers:
                    s.prepare()
                prev = H.Solver.run_many(solvers)   # the cold solve the rounds start from
            h = hashlib.sha1()
            whole, loop = [], []
            iters = []
            for rnd in range(rounds):
                data = [round_data(lps[k], rnd, k) for k in range(K)]
                xs, ys = [r.x for r in prev], [r.y for r in prev]
                with quiet():
                    t0 = time.perf_counter()
                    if side == "member":
                        for k, s in enumerate(solvers):
                            s.set_data(**data[k])
                            lam = s.scalars()["lambda_max"]
                            s.reset()
                            s.init(-1.0, lam)
                            s.set_start(xs[k], ys[k])
                        prev = H.Solver.run_many(solvers)
                    else:
                        H.Solver.set_data_many(solvers, data)
                        prev = H.Solver.resolve_many(solvers, xs, ys)
                    w = time.perf_counter() - t0
                whole.append(w)
                if side == "member":   # out.time of run_many starts from the power iteration's seconds (see the docstring)
                    loop.append(max(r.time - s.scalars()["power_time"] for r, s in zip(prev, solvers)))
                else:                  # ... of resolve_many from the set_data seconds since the previous loop
                    loop.append(max(r.time - s.data_seconds()["total"] for r, s in zip(prev, solvers)))
                iters += [r.iter for r in prev]
                for r in prev:
                    h.update(f"{r.status} {r.iter} ".encode())
                    h.update(np.ascontiguousarray(r.x).tobytes())
            counts = "-"
            if side == "group":
                c = H.last_resolve_many_counts()
                counts = " ".join(str(c[k]) for k in H.RESOLVE_MANY_KEYS)
            for s in solvers:
                s.close()
            print("PASS " + json.dumps(dict(case=name, K=K, whole=statistics.mean(whole), loop=statistics.mean(loop),
                                            outside=statistics.mean(whole) - statistics.mean(loop), counts=counts, digest=h.hexdigest()[:12],
                                            iters=[min(iters), max(iters)])), flush=True)
        for m in models:
            m.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("member", "group"))
    ap.add_argument("--lib-a", help="the yardstick: the parent commit's libhprlp.so (side a, member by member)")
    ap.add_argument("--lib-b", default=os.path.join(ROOT, "lib", "libhprlp.so"))
    ap.add_argument("--ks", default="1,16,64,256")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    if a.child:
        one_pass(a.child, ks, a.rounds, a.tol, a.max_iter)
        return
    if not a.lib_a:
        sys.exit("[many_resolve_ab] --lib-a (the parent commit's library) is required")
    sides = {"a member-by-member": ("member", a.lib_a), "b group": ("group", a.lib_b)}
    runs = {}
    for p in range(a.passes + 1):   # (pass 0: the warm-up pair)
        for label, (child, lib) in sides.items():
            env = dict(os.environ, HPRLP_LIB=os.path.abspath(lib))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", child, "--ks", a.ks, "--rounds", str(a.rounds), "--tol", str(a.tol), "--max-iter",
                   str(a.max_iter)]
            with subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as proc:
                tail = []
                for ln in proc.stdout:   # (line by line as they come: a long run is seen to make progress)
                    tail = (tail + [ln])[-40:]
                    if ln.startswith("PASS "):
                        d = json.loads(ln[5:])
                        print(f"pass {p} side {label}: {d['case']} K = {d['K']} whole {d['whole']:.5f} s", flush=True)
                        if p > 0:
                            runs.setdefault((d["case"], d["K"]), {}).setdefault(label, []).append(d)
            if proc.returncode != 0:
                sys.exit(f"[many_resolve_ab] pass {p}, side {label}: exit {proc.returncode}\n{''.join(tail)}")
    lines = [f"# tools/many_resolve_ab.py: {a.rounds} rounds of new c and row sides on K resident solvers, each started from the previous solution;",
             "# a: set_data, reset, init, set_start member by member + run_many; b: set_data_many + resolve_many; stop_tol " + f"{a.tol:g}, max_iter {a.max_iter}",
             f"# one process per library and pass, A/B/A/B, {a.passes} measured pairs after one warm-up pair; seconds per round, median [min .. max]",
             f"# a: {a.lib_a}", f"# b: {a.lib_b}",
             "# loop only: the largest out.time of a member less its base (a: power-iteration seconds, b: set_data seconds); b's zeroing, code, ctrl",
             "# and start kernels run after the loop's clock has started and are booked under its loop, a's run before it: a bias against b",
             "# case | K | side | whole round | loop only | outside the loop | counts (" + ", ".join(
                 ("h2d", "d2h", "waits", "launches", "memsets", "served", "own", "loop own")) + ") | digest(s)"]
    for (name, K), by_side in runs.items():
        med = {}
        for label, ds in by_side.items():
            def col(key):
                v = sorted(d[key] for d in ds)
                return statistics.median_low(v), v[0], v[-1]
            w, l, o = col("whole"), col("loop"), col("outside")
            med[label] = (w, o)
            digests = sorted({d["digest"] for d in ds})
            lines.append(f"{name} | {K} | {label} | {w[0]:.5f} [{w[1]:.5f} .. {w[2]:.5f}] | {l[0]:.5f} [{l[1]:.5f} .. {l[2]:.5f}] | "
                         f"{o[0]:.5f} [{o[1]:.5f} .. {o[2]:.5f}] | {ds[-1]['counts']} | {' '.join(digests)}")
        if len(med) == 2:
            (wa, oa), (wb, ob) = med["a member-by-member"], med["b group"]
            same = len({d["digest"] for ds in by_side.values() for d in ds}) == 1
            spreads = (oa[2] - oa[1]) + (ob[2] - ob[1])
            lines.append(f"#   K = {K}: outside the loop a - b = {oa[0] - ob[0]:.5f} s (the two spreads together {spreads:.5f}); whole round a / b = "
                         f"{wa[0] / wb[0]:.2f}; digest identical on both sides in every pass: {same}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
