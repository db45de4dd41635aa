"""Group device re-solve of many small LPs (DESIGN.md "Many small LPs", group device re-solve): K resident solvers, rounds of new
c and new row sides for every member, produced ON THE GPU, each round started from the previous round's x, y, which are wanted on
the GPU again --
  (a) the host group entries: the caller brings the packed inputs to the host (one copy per kind), calls set_data_many +
      resolve_many, and puts x, y, z back on the GPU (one copy per kind), against
  (b) the device group entries: set_data_many_tensors + resolve_many_tensors on slices of the same packed tensors, the solution
      written over the start.

  python tools/many_device_ab.py [--ks 8,64,512] [--rounds 5] [--tol 1e-4] [--max-iter 2000] [--out profiles/many_device_ab.txt]

Same box, same process, same library: this commit leaves the host group entries as they were, so side (a) is the yardstick as it
stands.  Two identically prepared groups (create_many, scale_many, power_iteration_many, init) of the class shapes of
tests/test_gpu_many.py, member k on shape k mod 4 with data of its own; one unmeasured warm-up round, then `rounds` measured rounds
in which the sides alternate (a, b, a, b ...) on the same numbers.  Every timed window ends in a wait for the device (the entries
return after their stream has drained; side (a)'s last copy is followed by a synchronise).  The table gives the median
[min .. max] of a round's seconds: (a) whole = transfers + entries, (a) entries alone, (b) whole; then the loop only (the largest
out.time of a member less its set_data seconds), which both sides share, and the counts of the last round.  x, y, z of every member
must be the same bits on both sides in every round.  A host without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("c", "AL", "AU", "l", "u")


def round_data(lp, rnd, k):
    """tools/many_resolve_ab.py's: c moved by 1e-3 relative, the row sides moved outwards (the planted point stays feasible)."""
    rng = np.random.default_rng(1000 * rnd + k)
    m = lp["m"]
    AL, AU = np.asarray(lp["AL"], float), np.asarray(lp["AU"], float)
    return dict(c=lp["c"] * (1 + 1e-3 * rng.normal(size=lp["n"])), AL=AL - 1e-3 * rng.uniform(size=m) * (1 + np.abs(AL)),
                AU=AU + 1e-3 * rng.uniform(size=m) * (1 + np.abs(AU)), l=np.asarray(lp["l"], float), u=np.asarray(lp["u"], float))


def group_of(H, models, prm):
    s = H.Solver.create_many(models, prm)
    H.Solver.scale_many(s)
    for sv, (lam, _) in zip(s, H.Solver.power_iteration_many(s)):
        sv.init(-1.0, 1.01 * lam)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="8,64,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from many_ab import quiet
    from conftest import hprlp as H
    from test_gpu_many import CLASS_SHAPES, planted
    import ctypes as C
    L = H.lib()
    L.hprlp_warmup.restype = C.c_int
    if L.hprlp_warmup(0) != 0 or not torch.cuda.is_available():
        sys.exit("[many_device_ab] no GPU: " + H.last_error())
    prm = H.Parameters(stop_tol=a.tol, use_presolve=False, max_iter=a.max_iter)
    shapes = [planted(s) for s in CLASS_SHAPES]
    shape_models = [H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
                    for lp in shapes]
    lines = [f"# tools/many_device_ab.py: {a.rounds} rounds of new c and row sides on K resident solvers (the class shapes of tests/test_gpu_many.py, member k",
             "# on shape k mod 4), inputs produced on the GPU, each round started from the previous x, y, the solution wanted on the GPU;",
             "# a: packed inputs to the host + set_data_many + resolve_many + x, y, z back to the GPU; b: set_data_many_tensors + resolve_many_tensors;",
             f"# one process, one library, two identically prepared groups, sides alternating on the same numbers; stop_tol {a.tol:g}, max_iter {a.max_iter};",
             "# seconds per round, median [min .. max]; counts: h2d, d2h, waits, launches, memsets, served, own (set_data / resolve, outside the loop)",
             "# K | a whole | a entries alone | b whole | loop only (a / b) | a / b whole | counts a | counts b | device counts b (resolve) | same bits"]
    for K in [int(k) for k in a.ks.split(",")]:
        lps = [shapes[k % 4] for k in range(K)]
        models = [shape_models[k % 4] for k in range(K)]
        with quiet():
            ga, gb = group_of(H, models, prm), group_of(H, models, prm)
        ns, ms = [lp["n"] for lp in lps], [lp["m"] for lp in lps]
        offs_n, offs_m = np.concatenate(([0], np.cumsum(ns))), np.concatenate(([0], np.cumsum(ms)))
        length = {"c": offs_n[-1], "l": offs_n[-1], "u": offs_n[-1], "AL": offs_m[-1], "AU": offs_m[-1]}
        offs = {"c": offs_n, "l": offs_n, "u": offs_n, "AL": offs_m, "AU": offs_m}

        def cut(t, o, k):
            return t[int(o[k]):int(o[k + 1])]

        # the carried x, y (and z) of both sides, packed: the cold solve of the warm-up round fills them
        Xb, Zb = (torch.zeros(int(offs_n[-1]), dtype=torch.float64, device="cuda") for _ in range(2))
        Yb = torch.zeros(int(offs_m[-1]), dtype=torch.float64, device="cuda")
        Xa, Ya, Za = Xb.clone(), Yb.clone(), Zb.clone()
        out_b = [(cut(Xb, offs_n, k), cut(Yb, offs_m, k), cut(Zb, offs_n, k)) for k in range(K)]
        whole_a, inner_a, whole_b, loop_a, loop_b = [], [], [], [], []
        same = True
        for rnd in range(a.rounds + 1):   # (round 0: the warm-up, from a cold start)
            data = [round_data(lps[k], rnd, k) for k in range(K)]
            packed = {v: torch.from_numpy(np.concatenate([d[v] for d in data])).cuda() for v in KINDS}   # (the caller's GPU data)
            assert all(packed[v].shape[0] == length[v] for v in KINDS)
            tdata = [{v: cut(packed[v], offs[v], k) for v in KINDS} for k in range(K)]
            warm = rnd > 0
            torch.cuda.synchronize()
            for side in ("a", "b"):
                with quiet():
                    t0 = time.perf_counter()
                    if side == "a":
                        host = {v: packed[v].cpu().numpy() for v in KINDS}
                        xs_h, ys_h = Xa.cpu().numpy(), Ya.cpu().numpy()
                        hd = [{v: cut(host[v], offs[v], k) for v in KINDS} for k in range(K)]
                        xs = [cut(xs_h, offs_n, k) for k in range(K)] if warm else None
                        ys = [cut(ys_h, offs_m, k) for k in range(K)] if warm else None
                        t1 = time.perf_counter()
                        H.Solver.set_data_many(ga, hd)
                        ca_data = H.last_resolve_many_counts()
                        ra = H.Solver.resolve_many(ga, xs, ys)
                        ca = H.last_resolve_many_counts()
                        t2 = time.perf_counter()
                        Xa.copy_(torch.from_numpy(np.concatenate([r.x for r in ra])))
                        Ya.copy_(torch.from_numpy(np.concatenate([r.y for r in ra])))
                        Za.copy_(torch.from_numpy(np.concatenate([r.z for r in ra])))
                        torch.cuda.synchronize()
                        t3 = time.perf_counter()
                        if warm:
                            whole_a.append(t3 - t0), inner_a.append(t2 - t1)
                            loop_a.append(max(r.time - s.data_seconds()["total"] for r, s in zip(ra, ga)))
                    else:
                        H.Solver.set_data_many_tensors(gb, tdata)
                        cb_data = H.last_resolve_many_counts()
                        xs = [o[0] for o in out_b] if warm else None
                        ys = [o[1] for o in out_b] if warm else None
                        rb = H.Solver.resolve_many_tensors(gb, xs, ys, out=out_b)
                        cb, db = H.last_resolve_many_counts(), H.last_many_device_counts()
                        t3 = time.perf_counter()
                        if warm:
                            whole_b.append(t3 - t0)
                            loop_b.append(max(r.time - s.data_seconds()["total"] for r, s in zip(rb, gb)))
            same = same and torch.equal(Xa, Xb) and torch.equal(Ya, Yb) and torch.equal(Za, Zb)
            same = same and all((p.status, p.iter) == (q.status, q.iter) for p, q in zip(ra, rb))
            print(f"K = {K} round {rnd}: b {t3 - t0:.5f} s, same bits so far: {same}", flush=True)

        def col(v):
            v = sorted(v)
            return f"{statistics.median_low(v):.5f} [{v[0]:.5f} .. {v[-1]:.5f}]"

        def cnt(c):
            return " ".join(str(c[k]) for k in H.RESOLVE_MANY_KEYS[:7])

        ratio = statistics.median_low(sorted(whole_a)) / statistics.median_low(sorted(whole_b))
        lines.append(f"{K} | {col(whole_a)} | {col(inner_a)} | {col(whole_b)} | {col(loop_a)} / {col(loop_b)} | {ratio:.2f} | {cnt(ca_data)} / {cnt(ca)} | "
                     f"{cnt(cb_data)} / {cnt(cb)} | {' '.join(str(db[k]) for k in H.MANY_DEVICE_KEYS)} | {same}")
        lines.append(f"#   K = {K}: outside the loop a = {statistics.median_low(sorted(whole_a)) - statistics.median_low(sorted(loop_a)):.5f} s, "
                     f"b = {statistics.median_low(sorted(whole_b)) - statistics.median_low(sorted(loop_b)):.5f} s; the device entries are "
                     f"{'faster' if ratio > 1 else 'NOT faster'} on the whole round at this K")
        H.Solver.close_many(ga)
        H.Solver.close_many(gb)
    for m in shape_models:
        m.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
