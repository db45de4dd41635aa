"""Streams with parents (DESIGN.md "Streamed batches", "Parents"): a rolling horizon level by level against one call with parents.

  python tools/batched_stream_parents_ab.py [config4|planted] [chains] [periods] [width] [tol] [rounds]

config4 (the default): BASELINE config 4's matrix (33 874 x 105 728), 64 chains x 4 periods by the recipe of
tools/batched_stream_ab.py (make_batch, seed 4), period t + 1 of a chain being period t with C perturbed by 1e-3; width 64,
tolerance 1e-4.  planted: the 300 x 400 LP of the tests, for a rehearsal.  The queue is numbered period by period and lies on the
GPU as torch tensors before the clock starts.
A: what the stream offers without parents -- one solve_stream_tensors call per period, each fed the previous call's x, y as X0, Y0
   (period 0 cold): every level waits for its slowest member.
B: one solve_stream_tensors call with parent[p] = p - chains.
The two alternate on one handle: one warm-up round, then `rounds` measured ones.  Reported per side: loop iterations, loop seconds
and refill-pass seconds (stream_info(), stream_seconds(); host clocks around work that ends in a device synchronise; median
[min .. max]), occupancy = sum of iter / (width x loop iterations), and the bytes over the bus (transfer()).  Checked in the tool:
B's loop iterations EQUAL the makespan of hprlp.stream_schedule(iter // check_iter, width, parent) of B's own iteration counts, and
A's equal the sum of its calls' longest members (exit 1 otherwise).  Per problem the sides' status and iter are compared, and all
bits where the problem sat in the same slot on both sides.
One line per measurement on stdout ("[batched_stream_parents_ab] ..."), also appended to profiles/batched_stream_parents_ab.txt;
the library's own log goes to stderr.
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BITS = ("x", "y", "z", "primal_obj", "residuals", "gap")


def _quiet():
    """The library prints its log on fd 1: send it to stderr, keep our lines on a private copy of stdout."""
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)
    return out


def spread(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]"


def main(which="config4", chains=64, periods=4, width=64, tol=1e-4, rounds=2):
    import torch
    from conftest import hprlp as H, lpgen
    from test_gpu_warm import make_batch
    out = _quiet()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "batched_stream_parents_ab.txt"), "a")

    def say(text):
        for f in (out, log):
            print("[batched_stream_parents_ab] " + text, file=f, flush=True)

    if which == "config4":
        lp, name, seed = lpgen.c3_pds20_like(), "config 4", 4
    else:
        lp, name, seed = lpgen.planted_lp(300, 400, 2400, 7, values="network"), "planted 300 x 400", 2
    Cm, AL, AU, L, U = make_batch(lp, chains, seed)
    rng = np.random.default_rng(40)
    Cs = [Cm]
    for _ in range(periods - 1):
        Cs.append(Cs[-1] * (1 + 1e-3 * rng.normal(size=Cm.shape)))
    rep = lambda a: np.concatenate([a] * periods, axis=1)
    args = (np.concatenate(Cs, axis=1), rep(AL), rep(AU), rep(L), rep(U))
    count = chains * periods
    parent = np.array([-1 if p < chains else p - chains for p in range(count)])
    model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=199950, time_limit=600.0)
    check = prm.to_c().check_iter
    h = H.BatchedSolver(model, prm)
    targs = [torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).cuda().T for a in args]
    level = [[t[:, g * chains:(g + 1) * chains] for t in targs] for g in range(periods)]
    torch.cuda.synchronize()
    say(f"{name} ({lp['m']} x {lp['n']}), {chains} chains x {periods} periods, C perturbed by 1e-3 from period to period, width {width}, "
        f"tol {tol:g}; A = one solve_stream_tensors call per period from the previous call's x, y, B = one call with parents; "
        f"alternating, one warm-up round, {rounds} measured")
    acc = {e: {k: [] for k in ("loop", "refill_passes")} for e in "AB"}
    ok = True
    for rnd in range(rounds + 1):
        # -- A: level by level
        a = dict(status=[], iter=[], slot=[], **{f: [] for f in BITS})
        a_loop = a_sec = a_refill = 0.0
        a_bytes = [0, 0]
        longest, bumps = [], 0
        X0 = Y0 = None
        for g in range(periods):
            r = h.solve_stream_tensors(*level[g], width=width, X0=X0, Y0=Y0)
            info, ssec, tr = h.stream_info(), h.stream_seconds(), h.transfer()
            X0, Y0 = r["x"], r["y"]
            a_loop += info["loop_iterations"]
            a_sec += ssec["refill_passes"] + ssec["rest"]
            a_refill += ssec["refill_passes"]
            a_bytes = [a_bytes[0] + tr["staged_h2d_bytes"], a_bytes[1] + tr["staged_d2h_bytes"]]
            bumps += info["lambda_bumps"]
            longest.append(int(r["iter"].max()))
            a["status"] += r["status"]
            for f in ("iter", "slot", "primal_obj", "residuals", "gap"):
                a[f].append(np.asarray(r[f]))
            for f in ("x", "y", "z"):
                a[f].append(r[f].cpu().numpy())
        for f in ("iter", "slot", "primal_obj", "residuals", "gap"):
            a[f] = np.concatenate(a[f])
        for f in ("x", "y", "z"):
            a[f] = np.concatenate(a[f], axis=1)
        a_sum = int(a["iter"].sum())
        if a_loop != sum(longest):
            ok = False
        say(f"round {rnd}{' (warm-up)' if rnd == 0 else ''} A: loop iterations {int(a_loop)} = sum of the calls' longest members {longest} "
            f"({'yes' if a_loop == sum(longest) else 'NO'}); loop {a_sec:.4f} s (refill passes {a_refill:.4f} s); occupancy "
            f"{a_sum / (width * a_loop):.3f}; bytes in / back {a_bytes[0]} / {a_bytes[1]}; lambda bumps {bumps}")
        # -- B: one call with parents
        r = h.solve_stream_tensors(*targs, width=width, parent=parent)
        info, ssec, tr, pinfo = h.stream_info(), h.stream_seconds(), h.transfer(), h.stream_parents_info()
        b = dict(r, **{f: r[f].cpu().numpy() for f in ("x", "y", "z")})
        slot, ein, eout = H.stream_schedule(b["iter"] // check, width, parent)
        makespan = int(eout.max()) * check
        exact = info["loop_iterations"] == makespan and all(np.array_equal(b[f], w) for f, w in (("slot", slot), ("event_in", ein), ("event_out", eout)))
        ok = ok and exact
        b_sum = int(b["iter"].sum())
        say(f"round {rnd}{' (warm-up)' if rnd == 0 else ''} B: loop iterations {info['loop_iterations']} = the parents schedule's makespan "
            f"{makespan} and the record is that schedule ({'yes' if exact else 'NO'}); loop {ssec['refill_passes'] + ssec['rest']:.4f} s "
            f"(refill passes {ssec['refill_passes']:.4f} s); occupancy {b_sum / (width * info['loop_iterations']):.3f}; bytes in / back "
            f"{tr['staged_h2d_bytes']} / {tr['staged_d2h_bytes']}; lambda bumps {info['lambda_bumps']}; refills {info['refills']} in "
            f"{info['refill_evaluations']} evaluations; {pinfo}")
        if rnd:
            acc["A"]["loop"].append(a_sec); acc["A"]["refill_passes"].append(a_refill)
            acc["B"]["loop"].append(ssec["refill_passes"] + ssec["rest"]); acc["B"]["refill_passes"].append(ssec["refill_passes"])
        same_status = sum(a["status"][p] == b["status"][p] and a["iter"][p] == b["iter"][p] for p in range(count))
        same_slot = [p for p in range(count) if a["slot"][p] == b["slot"][p]]
        same_bits = sum(a["status"][p] == b["status"][p] and a["iter"][p] == b["iter"][p] and
                        all(np.array_equal(a[f][..., p], b[f][..., p]) for f in BITS) for p in same_slot)
        say(f"round {rnd}: status and iter agree for {same_status} of {count} problems; {len(same_slot)} sat in the same slot on both sides, "
            f"{same_bits} of them agree bit for bit; loop iterations A - B = {int(a_loop) - info['loop_iterations']} "
            f"({info['loop_iterations'] / a_loop:.3f} x)")
    for e in "AB":
        say(f"{e} seconds, median [min .. max] of {rounds}: loop {spread(acc[e]['loop'])}; refill passes {spread(acc[e]['refill_passes'])}")
    say(f"the exact checks hold in every round: {ok}")
    h.close()
    model.free()
    return 0 if ok else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    sys.exit(main(a[0] if a else "config4", int(a[1]) if len(a) > 1 else 64, int(a[2]) if len(a) > 2 else 4, int(a[3]) if len(a) > 3 else 64,
                  float(a[4]) if len(a) > 4 else 1e-4, int(a[5]) if len(a) > 5 else 2))
