"""The resident batched solver's three entries by value: a fixed list of calls against whatever HPRLP_LIB names, one line each.

  HPRLP_LIB=lib/variants/libhprlp_<NAME>.so python tools/batched_calls_digest.py > a.txt    (and once per other library; diff)

Per call: a SHA-256 over status, iter, x, y, z, primal_obj, residuals, gap and, with detection, the certificates' arrays (for a
stream also slot, event_in, event_out), then info(), transfer() and, for a stream, stream_info().  Nothing timed is printed: two
libraries that compute the same print the same.  The calls: host entry cold, with X0 / Y0, carry, with detection on the mixed
batch of tests/test_gpu_batched_detect.py; device entry cold and with starts; streams of width 3, 12 and 64, with starts, with
detection; a plain solve after a stream.  All but the detection's on the planted 300 x 400 LP of the tests at 1e-4.
The library's own log goes to stderr.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FIELDS = ("iter", "x", "y", "z", "primal_obj", "residuals", "gap")
CERT_FIELDS = ("kind", "iter", "objective", "violation", "y", "z", "d")


def digest(r):
    h = hashlib.sha256("|".join(r["status"]).encode())
    arrays = [(f, r[f]) for f in FIELDS] + [(f, r[f]) for f in ("slot", "event_in", "event_out") if f in r]
    arrays += [("cert_" + f, r["certificates"][f]) for f in CERT_FIELDS] if "certificates" in r else []
    for name, a in arrays:
        h.update(name.encode())
        if a is not None:
            a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
            h.update(str((a.dtype, a.shape)).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    from conftest import hprlp as H, lpgen
    from test_gpu_batched_detect import MIXED_PRM, _mixed
    from test_gpu_batched_device import T
    from test_gpu_warm import make_batch
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)

    def say(name, h, r, streamed=False):
        counts = [h.info(), h.transfer()] + ([h.stream_info()] if streamed else [])
        statuses = {s: r["status"].count(s) for s in sorted(set(r["status"]))}
        print(f"{name}: {digest(r)} {statuses} iter {int(np.min(r['iter']))}..{int(np.max(r['iter']))} "
              + " ".join(str(c) for c in counts), file=out, flush=True)

    lp = lpgen.planted_lp(300, 400, 2400, 7, values="network")
    model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = H.Parameters(stop_tol=1e-4, max_iter=45000, use_presolve=False, use_CR_scaling=False)
    args = make_batch(lp, 160, 2)
    part = lambda N: tuple(a[:, :N] for a in args)
    h = H.BatchedSolver(model, prm)
    rough = h.solve(*part(10), param=H.Parameters(stop_tol=1e-2, max_iter=45000, use_presolve=False, use_CR_scaling=False))
    X0, Y0 = rough["x"], rough["y"]
    say("host cold", h, h.solve(*part(8)))
    say("host X0 Y0", h, h.solve(*part(8), X0=X0[:, :8], Y0=Y0[:, :8]))
    say("host carry", h, h.solve(*part(8), carry=True))
    say("device cold", h, h.solve_tensors(*[T(a) for a in part(8)]))
    say("device X0 Y0", h, h.solve_tensors(*[T(a) for a in part(8)], X0=T(X0[:, :8]), Y0=T(Y0[:, :8])))
    for width, N in ((3, 7), (12, 30), (64, 160)):
        say(f"stream width {width}", h, h.solve_stream(*part(N), width=width), streamed=True)
    say("stream X0 Y0", h, h.solve_stream(*part(10), width=4, X0=X0, Y0=Y0), streamed=True)
    say("plain after a stream", h, h.solve(*part(4)))
    say("carry after that", h, h.solve(*part(4), carry=True))
    h.close()
    model.free()

    members, model, margs = _mixed(20)
    mprm = H.Parameters(**MIXED_PRM)
    h = H.BatchedSolver(model, mprm)
    say("host detection", h, h.solve(*(a[:, :8] for a in margs), eps_primal=1e-8, eps_dual=1e-8))
    say("stream detection", h, h.solve_stream(*margs, width=8, eps_primal=1e-8, eps_dual=1e-8), streamed=True)
    say("device detection after a stream", h, h.solve_tensors(*[T(a[:, :8]) for a in margs], eps_primal=1e-8, eps_dual=1e-8))
    h.close()
    model.free()


if __name__ == "__main__":
    main()
