"""Streamed batches (DESIGN.md "Streamed batches"): plain batches one after the other against one stream, on one handle.

  python tools/batched_stream_ab.py [config4|planted] [count] [width] [tol] [reps]

config4 (the default): BASELINE config 4's matrix (33 874 x 105 728), 256 problems by the config-4 recipe of tools/warm_ab.py
(make_batch, then C perturbed by a relative 1e-3), width 64, tolerance 1e-4.  planted: the 300 x 400 LP of the tests, for a
rehearsal.  A: count / width plain solves of `width` members, in the problems' order.  B: one solve_stream of width `width`.
The two alternate, `reps` times, after one plain solve as warm-up (code objects, graph captures).  For both: loop iterations
(deterministic), wall seconds of the loops (BatchedSolver.seconds()["loop"]: a host clock around work that ends in a device
synchronise), occupancy = sum of the members' iterations / (width x loop iterations); for B also the mean wall time of an
evaluation's refill passes (harvest, refill, the new members' iteration-0 evaluation; stream_seconds()) beside the time of
check_iter iterations at that size.  Every problem's status and iteration count must agree between A and B wherever neither
side raised lambda_max; the tool says how many do.
One line per measurement on stdout ("[batched_stream_ab] ..."), also appended to profiles/batched_stream_ab.txt; the library's own
log goes to stderr.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHECK = 150


def _quiet():
    """The library prints its log on fd 1: send it to stderr, keep our lines on a private copy of stdout."""
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)
    return out


def main(which="config4", count=256, width=64, tol=1e-4, reps=2):
    from conftest import hprlp as H, lpgen
    from test_gpu_warm import make_batch
    out = _quiet()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "batched_stream_ab.txt"), "a")

    def say(text):
        for f in (out, log):
            print("[batched_stream_ab] " + text, file=f, flush=True)

    if which == "config4":
        lp, name = lpgen.c3_pds20_like(), "config 4"
        args = list(make_batch(lp, count, 4))
        args[0] = args[0] * (1 + 1e-3 * np.random.default_rng(40).normal(size=args[0].shape))
    else:
        lp, name = lpgen.planted_lp(300, 400, 2400, 7, values="network"), "planted 300 x 400"
        args = list(make_batch(lp, count, 2))
    model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=tol, use_presolve=False, max_iter=199950, time_limit=600.0)
    h = H.BatchedSolver(model, prm)
    groups = [np.arange(g, min(g + width, count)) for g in range(0, count, width)]
    say(f"{name} ({lp['m']} x {lp['n']}), {count} problems, width {width}, tol {tol:g}, check_iter {CHECK}; A = {len(groups)} plain "
        f"solves, B = one stream; {reps} repetitions, alternating, after one plain solve as warm-up")
    h.solve(*(a[:, groups[0]] for a in args))
    for rep in range(reps):
        it_a, st_a = np.zeros(count, dtype=np.int64), [None] * count
        loop_a, iters_a, bump_a = 0.0, 0, False
        for idx in groups:
            r = h.solve(*(a[:, idx] for a in args))
            it_a[idx] = r["iter"]
            for k, p in enumerate(idx):
                st_a[p] = r["status"][k]
            loop_a += h.seconds()["loop"]
            iters_a += int(np.max(r["iter"]))
            lam = h.lambda_max()
            bump_a = bump_a or lam[0] != lam[1]
        occ_a = it_a.sum() / (width * iters_a)
        say(f"rep {rep} A: loop iterations {iters_a} ({' + '.join(str(int(np.max(it_a[idx]))) for idx in groups)}), loops {loop_a:.4f} s, "
            f"occupancy {occ_a:.3f}, members' iterations max / mean {int(it_a.max())} / {it_a.mean():.0f}, "
            f"{sum(s == 'OPTIMAL' for s in st_a)} OPTIMAL, lambda raised: {bump_a}; {loop_a / (iters_a / CHECK) * 1e3:.3f} ms per {CHECK} iterations")
        r = h.solve_stream(*args, width=width)
        info, sec, loop_b = h.stream_info(), h.stream_seconds(), h.seconds()["loop"]
        it_b = np.asarray(r["iter"], dtype=np.int64)
        occ_b = it_b.sum() / (width * info["loop_iterations"])
        same = int(sum(a == b and x == y for a, b, x, y in zip(st_a, r["status"], it_a, it_b)))
        per_event = sec["rest"] / max(info["evaluations"] - 1, 1)
        per_refill = sec["refill_passes"] / max(info["refill_evaluations"], 1)
        say(f"rep {rep} B: loop iterations {info['loop_iterations']}, loop {loop_b:.4f} s, occupancy {occ_b:.3f}, "
            f"{sum(s == 'OPTIMAL' for s in r['status'])} OPTIMAL, lambda bumps {info['lambda_bumps']}; evaluations {info['evaluations']}, "
            f"of which with a refill {info['refill_evaluations']}, refills {info['refills']}, refill passes {info['refill_passes']}; "
            f"refill passes {sec['refill_passes']:.4f} s in all = {per_refill * 1e3:.3f} ms per evaluation with a refill, beside "
            f"{per_event * 1e3:.3f} ms per {CHECK} iterations with their evaluation ({per_refill / per_event * CHECK:.1f} iterations' worth)")
        say(f"rep {rep} B / A: loop iterations {info['loop_iterations'] / iters_a:.3f}, loop seconds {loop_b / loop_a:.3f}; "
            f"status and iter equal for {same} of {count} problems")
    say(f"handle: {h.info()}")
    h.close()
    model.free()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else "config4", int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 64,
         float(a[3]) if len(a) > 3 else 1e-4, int(a[4]) if len(a) > 4 else 2)
