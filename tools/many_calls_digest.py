"""The group entries for new data, re-solve and new matrix values by value, host and device: a fixed list of calls against whatever
HPRLP_LIB names, one line each.

  HPRLP_LIB=lib/variants/libhprlp_<NAME>.so python tools/many_calls_digest.py > a.txt    (and once per other library; diff)

Per re-solve: a SHA-256 over every member's status, iter, x, y, z, primal_obj, residuals and gap.  Per set_data / set_matrix
call: a SHA-256 over every member's stored vectors (scaled data, matrix values, norms, iterates), its scalars but the wall times,
info(), describe() and transfer() -- a call that returns nothing is known by what it leaves.  Then the integers of
last_resolve_many_counts() or last_values_many_counts() and, for a device call, of last_many_device_counts().  A refused call
prints its message, then the digest of what it left.  Nothing timed is printed: two libraries that compute the same print the
same.

The calls, for the host entries and for the device entries each, on a group of its own: set_data with c only, with the bounds only,
with both and obj_constant alone for one member; re-solve cold, from x and y, with a sigma override; the device re-solve with
out given, with one member's triple None and with one output None; set_matrix, then power iteration, init and re-solve; a member
skipped (None and {}); per entry one refused call (a NaN in c, a non-finite start, a non-finite value) followed by a good one.
All of it on three groups: four members that join; three that join and one off the small path (the long-row LP); a group of
one.  Shapes, helpers and parameters are those of tests/test_gpu_many.py, test_gpu_many_resolve.py, test_gpu_many_values.py and
test_gpu_many_device.py (stop_tol 1e-4, max_iter 5000).  The library's own log goes to stderr.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FIELDS = ("iter", "x", "y", "z", "primal_obj", "residuals", "gap")


def update(h, name, a):
    h.update(name.encode())
    if a is None:
        return
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    h.update(str((a.dtype, a.shape)).encode() + np.ascontiguousarray(a).tobytes())


def results_digest(results):
    h = hashlib.sha256()
    for r in results:
        h.update(r.status.encode())
        for f in FIELDS:
            update(h, f, getattr(r, f))
    return h.hexdigest()


def main():
    from conftest import hprlp as H
    from resolve_device_cases import dev
    from test_gpu_many import SIX, long_row_lp, make, planted, prepared
    from test_gpu_many_device import tensors
    from test_gpu_many_resolve import close, new_data, params
    from test_gpu_many_values import new_values, state
    from test_resolve import base_lp
    out = os.fdopen(os.dup(1), "w", buffering=1)
    os.dup2(2, 1)

    def state_digest(group):
        h = hashlib.sha256()
        for s in group:
            st = state(s)
            for k in sorted(st):
                if isinstance(st[k], np.ndarray):
                    update(h, k, st[k])
                else:
                    h.update(f"{k} {st[k]!r}".encode())
            h.update(repr(s.transfer()).encode())
        return h.hexdigest()

    def ints(d):
        return "[" + " ".join(str(int(v)) for v in d.values()) + "]"

    def say(tag, digest, counts, device):
        print(f"{tag}: {digest} {ints(counts())}" + (" " + ints(H.last_many_device_counts()) if device else ""), file=out, flush=True)

    def run(tag, lps, device):
        K = len(lps)
        models = [make(lp) for lp in lps]
        group = prepared(models, [params()] * K)
        side = "device" if device else "host"
        t = tensors if device else (lambda d: d)
        tv = (lambda v: None if v is None else dev(v)) if device else (lambda v: v)
        set_data = H.Solver.set_data_many_tensors if device else H.Solver.set_data_many
        set_matrix = H.Solver.set_matrix_many_tensors if device else H.Solver.set_matrix_many
        resolve_fn = H.Solver.resolve_many_tensors if device else H.Solver.resolve_many

        def data_call(name, data):
            try:
                set_data(group, [t(d) for d in data])
            except RuntimeError as e:
                print(f"{tag} {side} {name} refused: {e}", file=out, flush=True)
            say(f"{tag} {side} {name}", state_digest(group), H.last_resolve_many_counts, device)

        def matrix_call(name, data):
            try:
                set_matrix(group, [t(d) for d in data])
            except RuntimeError as e:
                print(f"{tag} {side} {name} refused: {e}", file=out, flush=True)
            say(f"{tag} {side} {name}", state_digest(group), H.last_values_many_counts, device)

        def resolve(name, x=None, y=None, sigma=None, **kw):
            try:
                res = resolve_fn(group, None if x is None else [tv(v) for v in x], None if y is None else [tv(v) for v in y], sigma, **kw)
            except RuntimeError as e:
                print(f"{tag} {side} {name} refused: {e}", file=out, flush=True)
                say(f"{tag} {side} {name}", state_digest(group), H.last_resolve_many_counts, device)
                return None
            say(f"{tag} {side} {name}", results_digest(res), H.last_resolve_many_counts, device)
            return res

        def host(v):
            return v.cpu().numpy() if hasattr(v, "cpu") else v

        data_call("set_data c", [new_data(lp, 100 + k, "c") for k, lp in enumerate(lps)])
        cold = resolve("resolve cold")
        data_call("set_data bounds", [new_data(lp, 200 + k, "bounds") for k, lp in enumerate(lps)])
        resolve("resolve x y", [host(r.x) for r in cold], [host(r.y) for r in cold])
        data_call("set_data both, obj_constant alone for member 0",
                  [dict(obj_constant=1.5) if k == 0 else new_data(lp, 300 + k, "both") for k, lp in enumerate(lps)])
        resolve("resolve sigma", sigma=[0.7 if k % 2 == 0 else None for k in range(K)])
        if device:
            import torch
            empty = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
            triples = [(empty(lp["n"]), empty(lp["m"]), empty(lp["n"])) for lp in lps]
            resolve("resolve out given", out=triples)
            resolve("resolve a None triple", out=[None if k == K - 1 else tr for k, tr in enumerate(triples)])
            resolve("resolve one None output", out=[(tr[0], tr[1], None) if k == 0 else tr for k, tr in enumerate(triples)])
        for rnd in range(2):   # (the first call builds the value maps)
            matrix_call(f"set_matrix {rnd}", [new_values(lp, 400 + 40 * rnd + k) for k, lp in enumerate(lps)])
            lams = H.Solver.power_iteration_many(group)
            for g, (lam, _) in zip(group, lams):
                g.init(-1.0, 1.01 * lam)
            print(f"{tag} {side} power iteration {rnd}: {[(float(lam).hex(), int(it)) for lam, it in lams]}", file=out, flush=True)
            resolve(f"resolve after set_matrix {rnd}")
        # a member that is skipped
        skip = [None if k == 1 else {} if k == 2 else new_data(lp, 500 + k, "both") for k, lp in enumerate(lps)]
        data_call("set_data with None and {}", skip)
        matrix_call("set_matrix with None", [None if k == 1 else new_values(lp, 520 + k) for k, lp in enumerate(lps)])
        lams = H.Solver.power_iteration_many(group)
        for g, (lam, _) in zip(group, lams):
            g.init(-1.0, 1.01 * lam)
        resolve("resolve after the skips")
        # one refusal per entry, then a good call
        last = K - 1
        good = [new_data(lp, 600 + k, "both") for k, lp in enumerate(lps)]
        bad = [dict(d) for d in good]
        bad[last]["c"] = np.array(bad[last]["c"], dtype=np.float64)
        bad[last]["c"][2] = np.nan
        data_call("set_data NaN in c", bad)
        data_call("set_data after the refusal", good)
        inf_x = np.full(lps[last]["n"], 0.5)
        inf_x[3] = np.inf
        resolve("resolve inf in x0", [None] * last + [inf_x])
        resolve("resolve NaN sigma", sigma=[float("nan")] + [None] * last)
        resolve("resolve after the refusals")
        values = [new_values(lp, 700 + k) for k, lp in enumerate(lps)]
        badv = [dict(v) for v in values]
        badv[last]["values"] = badv[last]["values"].copy()
        badv[last]["values"][1] = np.inf
        matrix_call("set_matrix inf in values", badv)
        nanv = [dict(v) for v in values]
        nanv[0]["l"] = np.array(nanv[0]["l"], dtype=np.float64)
        nanv[0]["l"][0] = np.nan
        matrix_call("set_matrix NaN in l", nanv)
        matrix_call("set_matrix after the refusals", values)
        lams = H.Solver.power_iteration_many(group)
        for g, (lam, _) in zip(group, lams):
            g.init(-1.0, 1.01 * lam)
        resolve("resolve at the end")
        close(group, models)

    groups = {"four that join": [planted(SIX[0]), planted(SIX[1]), planted(SIX[4]), base_lp(11)],
              "three and one off the small path": [planted(SIX[0]), dict(long_row_lp(), x_star=np.full(600, 0.5)), planted(SIX[4]), base_lp(11)],
              "a group of one": [base_lp(12)]}
    for tag, lps in groups.items():
        for device in (False, True):
            run(tag, lps, device)


if __name__ == "__main__":
    main()
