"""Set-up, scaling and teardown of hprlp_solve_many (DESIGN.md "Many small LPs", group set-up): two builds of the library against
each other, e.g. the parent commit's (member-by-member set-up) and this one's (hprlp_solver_create_many / _scale_many /
_destroy_many inside hprlp_solve_many).

  python tools/many_setup_ab.py --libs A=/path/to/parent/libhprlp.so,B=lib/libhprlp.so [--ks 1,16,64,256] [--passes 3]
                                [--tol 1e-4] [--out profiles/many_setup_ab.txt]

One process per library and pass (HPRLP_LIB names the build), order A/B/A/B after one unmeasured warm-up pair.  A process builds
the K models of a case -- (a) the 25fv47-like LP (821 x 1571, 10 700 nonzeros), (b) the planted (300, 500, 2500) LP, K seeds each --
and for every K calls solve_many once unmeasured and once measured.  Reported per library, case and K, over the passes, as median
[min .. max] in seconds: `setup` and `scaling` of hprlp_last_solve_many_phases, `teardown` (the call minus its four other phases:
the wall time of destroying the group), their sum, and the whole `call`; then the set-up counts where the library has them and a
digest of the results (status, iterations, x of every member) -- the two libraries must print the same digest.  With HPRLP_TEST_HOOKS=1
HPRLP_NO_GROUP_SETUP=1 in the environment the B side can also be held against itself.  A host without a GPU fails.

  python tools/many_setup_ab.py --child      (what the driver starts: one pass of one library, JSON lines on stdout)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = ("c2_25fv47_like", "planted 300x500x2500")


def child(ks, tol):
    from conftest import hprlp as H, lpgen
    from many_ab import digest, quiet
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0:
        sys.exit("[many_setup_ab] no GPU: " + H.last_error())
    prm = H.Parameters(stop_tol=tol, use_presolve=False)
    gens = {CASES[0]: lambda seed: lpgen.c2_25fv47_like(seed=seed), CASES[1]: lambda seed: lpgen.planted_lp(300, 500, 2500, seed)}
    for name in CASES:
        models = []
        for seed in range(100, 100 + max(ks)):
            lp = gens[name](seed)
            models.append(H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"]))
        for K in ks:
            for measured in (False, True):
                with quiet():
                    res = H.solve_many(models[:K], prm)
                p = H.last_solve_many_phases()
            counts = H.last_setup_many_counts() if hasattr(L, "hprlp_last_setup_many_counts") else None
            row = {"case": name, "K": K, "setup": p["setup"], "scaling": p["scaling"], "call": p["call"],
                   "teardown": p["call"] - p["setup"] - p["scaling"] - p["power"] - p["loop"], "loop": p["loop"], "power": p["power"],
                   "digest": digest(res), "counts": list(counts.values()) if counts else None}
            print("ROW " + json.dumps(row), flush=True)
        for m in models:
            m.free()


def spread(v):
    v = sorted(v)
    return f"{statistics.median_low(v):.4f} [{v[0]:.4f} .. {v[-1]:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default=None, help="A=path,B=path")
    ap.add_argument("--ks", default="1,16,64,256")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    if a.child:
        return child(ks, a.tol)
    if not a.libs:
        sys.exit("--libs A=path,B=path")
    libs = [kv.split("=", 1) for kv in a.libs.split(",")]
    rows = {name: [] for name, _ in libs}
    for p in range(a.passes + 1):
        for name, path in libs:
            env = dict(os.environ, HPRLP_LIB=os.path.abspath(path))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--ks", a.ks, "--tol", str(a.tol)], env=env, capture_output=True,
                                 text=True, timeout=900)
            if out.returncode != 0:
                sys.exit(f"[many_setup_ab] pass {p} of {name} failed: {out.stderr[-2000:]}")
            got = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if p > 0:  # (pass 0: the warm-up pair)
                rows[name].append(got)
            print(f"pass {p} {name}: {len(got)} rows", flush=True)
    lines = [f"# tools/many_setup_ab.py: hprlp_solve_many, stop_tol {a.tol:g}, no presolve; one process per library and pass, "
             f"{'/'.join(n for n, _ in libs)} alternating, {a.passes} measured passes after one warm-up pair;",
             "# in a process one unmeasured and one measured call per case and K; seconds, median [min .. max] over the passes",
             *[f"# library {n} = {p}" for n, p in libs],
             "# case | K | library | set-up | scaling | teardown | set-up + scaling + teardown | loop | whole call | set-up counts | digest"]
    for case in CASES:
        for K in ks:
            for name, _ in libs:
                sel = [r for got in rows[name] for r in got if r["case"] == case and r["K"] == K]
                if not sel:
                    continue
                outside = [r["setup"] + r["scaling"] + r["teardown"] for r in sel]
                digests = sorted({r["digest"] for r in sel})
                counts = sel[-1]["counts"]
                lines.append(f"{case} | {K} | {name} | {spread([r['setup'] for r in sel])} | {spread([r['scaling'] for r in sel])} | "
                             f"{spread([r['teardown'] for r in sel])} | {spread(outside)} | {spread([r['loop'] for r in sel])} | "
                             f"{spread([r['call'] for r in sel])} | {' '.join(str(c) for c in counts) if counts else '-'} | {' '.join(digests)}")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
