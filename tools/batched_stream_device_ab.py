"""Device-resident streams (DESIGN.md "Device-resident streams"): the host stream against the device stream, on one handle.

  python tools/batched_stream_device_ab.py [config4|planted] [count] [width] [tol] [rounds]

config4 (the default): BASELINE config 4's matrix (33 874 x 105 728), the 256-problem recipe of tools/batched_stream_ab.py, width
64, tolerance 1e-4.  planted: the 300 x 400 LP of the tests, for a rehearsal.  H: solve_stream on numpy arrays with norm rule 1.
D: solve_stream_tensors on the same queue as torch tensors that are on the GPU before the clock starts.  The two alternate: one
warm-up round, then `rounds` measured ones.  Reported as median [min .. max] over the measured rounds: the preparation seconds
(BatchedSolver.seconds(): prep, upload, results -- seconds[2], [3], [5]), the loop and the refill passes (stream_seconds()), each a
host clock around work that ends in a device synchronise; stream_memory() and transfer() of either entry; and whether all problems
agree bit for bit (status, iter, x, y, z, primal_obj, residuals, gap, the record).
One line per measurement on stdout ("[batched_stream_device_ab] ..."), also appended to profiles/batched_stream_device_ab.txt; the
library's own log goes to stderr.
"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FIELDS = ("x", "y", "z", "iter", "primal_obj", "residuals", "gap", "slot", "event_in", "event_out")


def _quiet():
    """The library prints its log on fd 1: send it to stderr, keep our lines on a private copy of stdout."""
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)
    return out


def spread(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]"


def main(which="config4", count=256, width=64, tol=1e-4, rounds=3):
    import torch
    from conftest import hprlp as H, lpgen
    from test_gpu_warm import make_batch
    out = _quiet()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "batched_stream_device_ab.txt"), "a")

    def say(text):
        for f in (out, log):
            print("[batched_stream_device_ab] " + text, file=f, flush=True)

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
    h.set_norms(1)
    targs = [torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).cuda().T for a in args]
    torch.cuda.synchronize()
    say(f"{name} ({lp['m']} x {lp['n']}), {count} problems, width {width}, tol {tol:g}; H = solve_stream (numpy, norm rule 1), "
        f"D = solve_stream_tensors (tensors on the GPU); alternating, one warm-up round, {rounds} measured")
    acc = {e: {k: [] for k in ("prep", "upload", "results", "loop", "refill_passes")} for e in "HD"}
    report, equal = {}, True
    for rnd in range(rounds + 1):
        res = {}
        for e in "HD":
            r = h.solve_stream(*args, width=width) if e == "H" else h.solve_stream_tensors(*targs, width=width)
            sec, ssec, info = h.seconds(), h.stream_seconds(), h.stream_info()
            if e == "D":
                r = dict(r, **{f: r[f].cpu().numpy() for f in ("x", "y", "z")})
            res[e] = r
            report[e] = (h.stream_memory(), h.transfer(), info)
            if rnd:
                for k in ("prep", "upload", "results", "loop"):
                    acc[e][k].append(sec[k])
                acc[e]["refill_passes"].append(ssec["refill_passes"])
            say(f"round {rnd}{' (warm-up)' if rnd == 0 else ''} {e}: prep {sec['prep']:.4f} s, upload {sec['upload']:.4f} s, loop {sec['loop']:.4f} s "
                f"(refill passes {ssec['refill_passes']:.4f} s), results {sec['results']:.4f} s; loop iterations {info['loop_iterations']}, "
                f"refills {info['refills']}, lambda bumps {info['lambda_bumps']}")
        same = res["H"]["status"] == res["D"]["status"] and all(np.array_equal(res["H"][f], res["D"][f]) for f in FIELDS)
        differ = sum(res["H"]["status"][p] != res["D"]["status"][p] or any(not np.array_equal(res["H"][f][..., p], res["D"][f][..., p]) for f in FIELDS)
                     for p in range(count))
        equal = equal and same
        say(f"round {rnd}: {count - differ} of {count} problems agree bit for bit")
    for e in "HD":
        a = acc[e]
        say(f"{e} seconds, median [min .. max] of {rounds}: prep {spread(a['prep'])}; upload {spread(a['upload'])}; results {spread(a['results'])}; "
            f"loop {spread(a['loop'])}; refill passes {spread(a['refill_passes'])}")
        mem, tr, info = report[e]
        say(f"{e} stream_memory (queue vectors, result / ray block, scalars + partials + tables, pinned host; bytes): {mem}; transfer: {tr}; "
            f"evaluations with a refill {info['refill_evaluations']}, refill passes {info['refill_passes']}")
    say(f"all {count} problems agree bit for bit in every round: {equal}")
    h.close()
    model.free()
    return 0 if equal else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    sys.exit(main(a[0] if a else "config4", int(a[1]) if len(a) > 1 else 256, int(a[2]) if len(a) > 2 else 64,
                  float(a[3]) if len(a) > 3 else 1e-4, int(a[4]) if len(a) > 4 else 3))
