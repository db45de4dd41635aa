#!/usr/bin/env python3
"""bench.py -- HPR iterations/sec (FP64) of the MI355X HPR-LP hot path.

    python bench.py --gpus N --steps K --warmup W            (N=1)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one HPR iteration (x-half + y-half, reference src/main_iterate.cu:434-481) on synthetic
data already resident in HBM.  Default workload: BASELINE.json config 5, the banded-random 10M x 10M,
~200M-nnz LP (the largest configuration; it fits one MI355X, so N=1 runs all of it and N>1
row-partitions the SAME problem: strong scaling).  Rank 0 prints one JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline figure, ms_per_step, the
timed steps' own half-step times).  --full adds everything else the benchmark measures or checks: the
bare SpMVs, the KKT check after the run, the whole solve to 1e-4, configs 2-4, the ladder, the predicted
scaling and the CPU baseline (each of them can still be left out with its --no-* switch).
--dump-outputs DIR writes the iterates x and y as the last timed step left them to DIR/x.npy, DIR/y.npy.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


H = _load("hprlp_amd", os.path.join("hpr-lp-c_amd", "hprlp.py"))
G = _load("hprlp_lpgen", os.path.join("hpr-lp-c_amd", "lpgen.py"))
SH = _load("hprlp_shard", os.path.join("hpr-lp-c_amd", "shard.py"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md, chip table)

WORKLOADS = {
    # name: (m, n, per_row, band)
    "c5": (10_000_000, 10_000_000, 20, 100_000),
    "c5_eighth": (1_250_000, 10_000_000, 20, 100_000),
    "c5_quarter": (2_500_000, 10_000_000, 20, 100_000),
    "c5_half": (5_000_000, 10_000_000, 20, 100_000),
    "c5_shard_like": (1_250_000, 1_250_000, 20, 100_000),  # rows and band of one of 8 shards of c5 (kernel-shape experiments)
    "c5_small": (1_000_000, 1_000_000, 20, 10_000),
    "band_6e7": (3_000_000, 3_000_000, 20, 30_000),   # the ladder's points as workloads of their own (kernel experiments)
    "band_6e6": (300_000, 300_000, 20, 3_000),
    "band_1.2e8": (6_000_000, 6_000_000, 20, 60_000),
    "band_1e8": (5_000_000, 5_000_000, 20, 50_000),
    "band_1.2e7": (600_000, 600_000, 20, 6_000),
    "band_1.6e7": (800_000, 800_000, 20, 8_000),
    "band_3e7": (1_500_000, 1_500_000, 20, 15_000),
    "band_4e7": (2_000_000, 2_000_000, 20, 20_000),
    "band_2e7_wide": (1_000_000, 1_000_000, 20, 100_000),   # same size as c5_small, config 5's band: the short form must decline
    "c5_tiny": (100_000, 100_000, 20, 1_000),
    # exactly 2 / 3 rounds of super-blocks over the 512 resident workgroups (config 5 has 1221 = 2.38 rounds): tail-balance experiments
    "c5_2rounds": (8_388_608, 8_388_608, 20, 100_000),
    "c5_3rounds": (12_582_912, 12_582_912, 20, 100_000),
    # config 5 handed over in a RANDOM row / column order: what the set-up time locality ordering (csrc/reorder.cpp) is for
    "c5_permuted": (10_000_000, 10_000_000, 20, 100_000),
    "c5_small_permuted": (2_000_000, 2_000_000, 20, 20_000),
}
PERMUTED = {"c5_permuted", "c5_small_permuted"}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def gen_banded(m, n, per_row, band, seed=5, row0=0, rows=None, threads=0):
    rows = m - row0 if rows is None else rows
    rp = np.zeros(rows + 1, np.int32)
    ci = np.zeros(rows * per_row, np.int32)
    v = np.zeros(rows * per_row, np.float64)
    L = H.lib()
    L.hprlp_gen_banded_csr.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, H.c_int_p,
                                       H.c_int_p, H.c_dbl_p, C.c_int]
    rc = L.hprlp_gen_banded_csr(m, n, per_row, band, seed, row0, rows, rp.ctypes.data_as(H.c_int_p),
                                ci.ctypes.data_as(H.c_int_p), v.ctypes.data_as(H.c_dbl_p), threads)
    if rc != 0:
        raise RuntimeError(H.last_error())
    return rp, ci, v


def permute_lp(lp, seed=99):
    """The same LP with rows and columns renumbered at random (the matrix through hprlp_permute_csr_host)."""
    m, n = lp["m"], lp["n"]
    rng = np.random.default_rng(seed)
    pr = rng.permutation(m).astype(np.int32)   # new -> old
    pc = rng.permutation(n).astype(np.int32)
    c_old2new = np.empty(n, np.int32); c_old2new[pc] = np.arange(n, dtype=np.int32)
    rp, ci, v = lp["rowptr"], lp["colind"], lp["values"]
    rp2 = np.zeros(m + 1, np.int32); ci2 = np.zeros(len(ci), np.int32); v2 = np.zeros(len(v), np.float64)
    L = H.lib()
    ip, dp = H.c_int_p, H.c_dbl_p
    rc = L.hprlp_permute_csr_host(m, n, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), v.ctypes.data_as(dp), pr.ctypes.data_as(ip),
                                  c_old2new.ctypes.data_as(ip), rp2.ctypes.data_as(ip), ci2.ctypes.data_as(ip), v2.ctypes.data_as(dp), 0)
    if rc != 0:
        raise RuntimeError(H.last_error())
    return dict(m=m, n=n, rowptr=rp2, colind=ci2, values=v2, AL=lp["AL"][pr], AU=lp["AU"][pr], l=lp["l"][pc], u=lp["u"][pc],
                c=lp["c"][pc], obj_star=lp["obj_star"])


def planted_vectors(m, n, seed=5):
    """The matrix-independent draws of the planted LP (full length; cheap next to the matrix), in banded_lp's order."""
    rng = np.random.default_rng(seed + 1)
    at_lower = rng.random(n) < 0.5
    x = np.where(at_lower, 0.0, rng.uniform(0.5, 2.0, size=n))
    z = np.where(at_lower, rng.uniform(0.0, 1.0, size=n), 0.0)
    l = np.zeros(n)
    u = np.where(rng.random(n) < 0.2, x + rng.uniform(0.5, 2.0, size=n), np.inf)
    is_eq = rng.random(m) < 0.5
    active = rng.random(m) < 0.6
    slack = rng.uniform(0.5, 2.0, size=m)
    y = np.where(is_eq, rng.normal(size=m), np.where(active, -rng.uniform(0.0, 1.0, size=m), 0.0))
    return dict(x=x, z=z, l=l, u=u, is_eq=is_eq, active=active, slack=slack, y=y)


def shard_rows_lp(name, parts, seed=5):
    """The (m / parts) x n matrix a MIDDLE rank of a `parts`-rank run of workload `name` really holds -- rows [rank m / parts,
    (rank + 1) m / parts) of the whole matrix, global column indices -- as an LP of its own (planted the same way): its y-half
    is that rank's y-half launch on the whole shard, and by the band's symmetry its rows of A^T (the x-half) have the same
    shape.  (The workloads `c5_half / c5_quarter / c5_eighth` of rounds 2-4 spread m / parts rows over ALL n columns instead:
    another matrix, with eight times the column window per super-block at parts = 8.)"""
    m, n, per_row, band = WORKLOADS[name]
    rank = parts // 2
    _, row_off, m_loc = SH.partition(m, parts, rank)
    rp, ci, v = gen_banded(m, n, per_row, band, seed, row0=row_off, rows=m_loc)
    return planted_on(m_loc, n, rp, ci, v, seed)


def banded_lp(m, n, per_row, band, seed=5):
    """Planted LP on the banded matrix: box 0<=x<=u, half equality rows, half active/inactive '<=' rows."""
    rp, ci, v = gen_banded(m, n, per_row, band, seed)
    return planted_on(m, n, rp, ci, v, seed)


def planted_on(m, n, rp, ci, v, seed=5):
    from scipy import sparse
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n), copy=False)
    p = planted_vectors(m, n, seed)
    b = A @ p["x"]
    AL = np.where(p["is_eq"], b, -np.inf)
    AU = np.where(p["is_eq"] | p["active"], b, b + p["slack"])
    c = A.T @ p["y"] + p["z"]
    return dict(m=m, n=n, rowptr=rp, colind=ci, values=v, AL=AL, AU=AU, l=p["l"], u=p["u"], c=c, obj_star=float(c @ p["x"]))


def banded_lp_shard(m, n, per_row, band, rank, world, dist, seed=5):
    """This rank's shard of the SAME planted LP without any rank generating or holding the whole matrix:
    its rows of A from the generator, its rows of A^T by sweeping the generator over ALL rows and keeping the columns it owns
    (hpr-lp-c_amd/shard.py: transposed_rows_generated -- the generator is a pure function of (seed, row); round 2's all-to-all of
    2e8 triples over gloo + argsort is kept in shard.py as the general form and as the test's cross-check).  Phase wall times go
    to stderr so that a time-limit kill names its phase."""
    from scipy import sparse
    t0 = time.time()
    threads = max(1, host_cpu_share() // max(world, 1))

    def phase(what):
        nonlocal t0
        import resource
        log(f"[bench] rank {rank}: shard assembly: {what} {time.time() - t0:.2f}s "
            f"(peak host RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6:.2f} GB, {threads} threads)")
        t0 = time.time()

    _, row_off, m_loc = SH.partition(m, world, rank)
    _, col_off, n_loc = SH.partition(n, world, rank)
    rp, ci, v = gen_banded(m, n, per_row, band, seed, row0=row_off, rows=m_loc, threads=threads)
    phase(f"rows [{row_off}, {row_off + m_loc}) of A generated")
    trp, tci, tv = SH.transposed_rows_generated(H, m, n, per_row, band, seed, rank, world, threads=threads)
    phase(f"columns [{col_off}, {col_off + n_loc}) of A (rows of A^T) kept from a sweep over all {m} rows")
    p = planted_vectors(m, n, seed)
    A_loc = sparse.csr_matrix((v, ci, rp), shape=(m_loc, n), copy=False)
    AT_loc = sparse.csr_matrix((tv, tci, trp), shape=(n_loc, m), copy=False)
    b = A_loc @ p["x"]
    rs, cs = slice(row_off, row_off + m_loc), slice(col_off, col_off + n_loc)
    AL = np.where(p["is_eq"][rs], b, -np.inf)
    AU = np.where(p["is_eq"][rs] | p["active"][rs], b, b + p["slack"][rs])
    c = AT_loc @ p["y"] + p["z"][cs]
    obj_loc = float(c @ p["x"][cs])
    if dist is not None and world > 1:
        import torch
        obj = torch.tensor([obj_loc], dtype=torch.float64)
        dist.all_reduce(obj)
        obj_loc = float(obj[0])
    shard = SH.ShardArrays(H, m, n, rank, world, rp, ci, v, trp, tci, tv, AL, AU, p["l"][cs], p["u"][cs], c)
    phase("planted vectors, b = A x, c = A^T y + z")
    return shard, obj_loc, len(v)


def bytes_per_iteration(m, n, nnz):
    """algorithmic HBM bytes of one fused normal HPR iteration."""
    return 24 * nnz + 4 * (m + n + 2) + 8 * (7 * n + 5 * m) + 8 * (m + n)


def bytes_x_half(m, n, nnz):
    """x-half launch: A^T CSR (12 B/nnz + row pointers), gather of y once (8m), x,c,l,u,last_x read and
    x,x_hat written (7 n-vectors)."""
    return 12 * nnz + 4 * (n + 1) + 8 * m + 56 * n


def bytes_y_half(m, n, nnz):
    return 12 * nnz + 4 * (m + 1) + 8 * n + 40 * m


def host_cpu_share():
    """CPUs this process may actually use: the cgroup quota if there is one, else the affinity mask."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def _oracle_rate(ms, ns, per_row, band, budget_s, min_iters):
    """Normal HPR iterations of oracle/hpr_oracle.c on the banded generator at ms x ns: (iterations, seconds, nnz)."""
    from oracle import oracle as O
    rp, ci, v = gen_banded(ms, ns, per_row, band, seed=5)
    trp, tci, tv = O.transpose(ms, ns, rp, ci, v)
    lp = O.ScaledLP.__new__(O.ScaledLP)
    lp.m, lp.n = ms, ns
    lp.Arp, lp.Aci, lp.Av = rp, ci, v
    lp.ATrp, lp.ATci, lp.ATv = trp, np.ascontiguousarray(tci), np.ascontiguousarray(tv)
    rng = np.random.default_rng(1)
    lp.AL = -np.ones(ms); lp.AU = np.ones(ms); lp.l = np.zeros(ns); lp.u = np.full(ns, 10.0); lp.c = rng.normal(size=ns)
    t1 = lp.time_iterations(1.0, 50.0, 2)  # warm caches, estimate
    iters = min(2000, max(min_iters, int(budget_s / max(t1 / 2, 1e-6))))
    t = lp.time_iterations(1.0, 50.0, iters)
    return iters, t, len(v)


def cpu_baseline(name, steps_budget_s=12.0):
    """Oracle (CPU port of the reference's iteration, oracle/hpr_oracle.c) timed on the host cores ON THE FULL
    WORKLOAD: the same banded generator at the workload's own size, >= 5 normal iterations in about
    steps_budget_s seconds.  One OpenMP thread per CPU of the process' share (an oversubscribed team would only
    measure the scheduler).  The 1/16-size sample of round 1 is kept beside it (`sample_1_16`) as a cross-check
    of the linear-in-nnz assumption."""
    from oracle import oracle as O
    O.set_num_threads(host_cpu_share())
    m, n, per_row, band = WORKLOADS[name]
    iters, t, nnz = _oracle_rate(m, n, per_row, band, steps_budget_s, 5)
    out = {"value": iters / t, "unit": "iterations/s", "cores": O.num_threads(), "kind": "port",
           "sample": f"oracle/hpr_oracle.c normal iterations on the full workload ({m}x{n}, {nnz} nnz, same banded "
                     f"generator, seed 5): {iters} iterations in {t:.1f}s"}
    if m >= 1_000_000:
        try:
            it2, t2, nnz2 = _oracle_rate(m // 16, n // 16, per_row, max(band // 16, 1), 4.0, 3)
            out["sample_1_16"] = {"iterations_per_s_scaled": it2 / t2 / 16, "nnz": nnz2, "iterations": it2, "seconds": t2}
        except Exception as e:  # noqa: BLE001
            out["sample_1_16"] = {"error": str(e)}
    return out


def fresh_process_solves(which):
    """Cold start: tools/cold_start.py in a FRESH process (this one has long been warm): four whole solve() calls of the
    config; the first pays for the HIP runtime, the device context and the code objects.  Returns {cold, warm} with the
    whole-call wall, the reference's instrument (HPRLP_results.time = power iteration + loop) and the library's phase
    table each; warm = the median call of the other three."""
    import subprocess
    out = {}
    for label, extra in (("first_solve_of_a_process", []), ("after_hprlp_warmup", ["warm"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cold_start.py"), which] + extra, env=dict(os.environ, HPRLP_COLD_START_JSON="1"),
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
        rec = None
        for ln in r.stderr.decode(errors="replace").splitlines():
            if ln.startswith("COLDJSON "):
                rec = json.loads(ln[len("COLDJSON "):])
        if rec is None:
            out[label] = {"error": r.stderr.decode(errors="replace")[-300:]}
            continue
        sv = rec["solves"]
        later = sorted(sv[1:], key=lambda q: q["whole_call_wall_s"])[len(sv[1:]) // 2]
        out[label] = {"cold": sv[0], "warm": later, "warmup_call_s": rec["warmup_s"], "library_load_s": rec["library_load_s"]}
    return out


def side_configs(cold_start=True):
    """BASELINE configs 2 and 3 (shape-matched stand-ins) on one GPU: it/s by graph replay and time-to-1e-4."""
    out = {}
    for key, lp in (("c2_25fv47_like", G.c2_25fv47_like()), ("c3_pds20_like", G.c3_pds20_like())):
        model = H.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"],
                                 lp["l"], lp["u"], lp["c"])
        s = H.Solver(model, H.Parameters(stop_tol=1e-4, use_presolve=False))
        s.scale()
        lam, _ = s.power_iteration()
        s.init(-1.0, lam * 1.01)
        t = s.time_iterations(200, 2000, 0)
        nnz = len(lp["values"])
        rate = 2000 / (t["total_ms"] * 1e-3)
        s.close()
        # time to 1e-4 = power iteration + loop (wall of hprlp_solver_run incl. the solution's way back).  These solves are
        # 30-50 ms of ~1500 launches and ~400 host waits: a neighbour on the host's cores or a GPU clock that has dropped
        # shows as a 3 x longer run now and then (tools/probe_small_env.py: 0.029 s or 0.10 s for the same loop), so the
        # leg runs three times; the figure is the fastest, all three are listed
        runs = []
        for _rep in range(3):
            s = H.Solver(model, H.Parameters(stop_tol=1e-4, use_presolve=False))
            s.scale()
            lam, pw_it = s.power_iteration()
            s.init(-1.0, lam * 1.01)
            t0 = time.time()
            r = s.run()
            tt = time.time() - t0
            runs.append({"power_iteration": s.scalars()["power_time"], "power_iterations": int(pw_it), "loop_wall": tt,
                         "solver_reported": r.time, "total": tt + s.scalars()["power_time"]})
            if _rep < 2:
                s.close()
        best = min(runs, key=lambda q: q["total"])
        out[key] = {"m": lp["m"], "n": lp["n"], "nnz": nnz, "iterations_per_s": rate,
                    "GBps_algorithmic": bytes_per_iteration(lp["m"], lp["n"], nnz) * rate / 1e9,
                    "time_to_1e-4_s": best["total"], "iters_to_1e-4": r.iter, "status": r.status,
                    # solver_reported is HPRLP_results.time (power iteration + loop, reference src/HPRLP.cu:150,246)
                    "time_to_1e-4_parts_s": best, "time_to_1e-4_all_runs_s": [q["total"] for q in runs],
                    "rel_obj_err": abs(r.primal_obj - lp["obj_star"]) / (1 + abs(lp["obj_star"]))}
        s.close()
        # what a caller's FIRST solve() of a process costs, and the following ones (a fresh process each; round 4).  Four child
        # processes inside the driver-timed run: 60 s each at most, none under a profiler (its preloaded library would profile
        # the children as well) or with --no-cold-start
        if cold_start and "rocprof" not in os.environ.get("LD_PRELOAD", "") and not any(k.startswith("ROCP") for k in os.environ):
            try:
                out[key]["solve_call_in_a_fresh_process"] = fresh_process_solves("c2" if key.startswith("c2") else "c3")
            except Exception as e:  # noqa: BLE001
                out[key]["solve_call_in_a_fresh_process"] = {"error": str(e)}
        if key == "c3_pds20_like":
            # BASELINE config 4: solve_batched, shared A = config-3 matrix, B = 64 perturbed c / AU columns.  Members are
            # kept bounded (infinite upper bounds -> 50: with the recipe's perturbed c an unbounded-above column makes the
            # member unbounded and the run meaningless).  Rate: a fixed 1500 iterations of the whole batch (tolerance
            # unreachable, nobody freezes); then the same batch to 1e-4, every member checked.
            B, iters = 64, 1500
            rng = np.random.default_rng(4)
            m, n = lp["m"], lp["n"]
            Cm = lp["c"][:, None] * (1 + 0.1 * rng.normal(size=(n, B)))
            AU = lp["AU"][:, None] + np.abs(rng.normal(scale=0.1, size=(m, B)))
            AL = np.repeat(lp["AL"][:, None], B, axis=1)
            AL = np.where(np.isfinite(AL), np.minimum(AL, AU), AL)
            L = np.repeat(lp["l"][:, None], B, axis=1)
            U = np.repeat(lp["u"][:, None], B, axis=1)
            U = np.where(np.isfinite(U), U, 50.0)
            rb = H.solve_batched(model, Cm, AL, AU, L, U, None,
                                 H.Parameters(stop_tol=1e-30, max_iter=iters, use_presolve=False))
            rate_b = iters / rb["solve_time"]
            bytes_b = 24 * nnz + 4 * (m + n + 2) + 8 * B * (8 * n + 6 * m)
            finite = bool(np.isfinite(rb["x"]).all() and np.isfinite(rb["y"]).all() and np.isfinite(rb["primal_obj"]).all())
            rt = H.solve_batched(model, Cm, AL, AU, L, U, None, H.Parameters(stop_tol=1e-4, max_iter=60000, use_presolve=False))
            n_opt = sum(1 for st in rt["status"] if st == "OPTIMAL")
            out["c4_batched_B64"] = {"m": m, "n": n, "nnz": nnz, "batch_size": B, "batch_iterations_per_s": rate_b,
                                     "lp_iterations_per_s": rate_b * B, "GBps_algorithmic": bytes_b * rate_b / 1e9,
                                     "solve_time_s": rb["solve_time"], "setup_time_s": rb["setup_time"],
                                     "finite_after_fixed_run": finite,
                                     "to_1e-4": {"optimal_members": n_opt, "max_kkt": float(np.max(rt["residuals"])),
                                                 "iterations_min_max": [int(np.min(rt["iter"])), int(np.max(rt["iter"]))],
                                                 "solve_time_s": rt["solve_time"], "setup_time_s": rt["setup_time"]}}
            if not finite or n_opt != B or not float(np.max(rt["residuals"])) <= 1e-4:
                raise RuntimeError(f"config 4 check failed: finite={finite}, optimal members {n_opt}/{B}, "
                                   f"max KKT {float(np.max(rt['residuals']))}")
        model.free()
    return out


def uniform_random_lp(m, n, per_row, seed=11):
    """Planted LP on a matrix WITHOUT hidden structure: `per_row` distinct uniformly random columns in every row (the generator
    of config 5 with a band as wide as the matrix: the far-column rule for all entries).  What BASELINE.json config 5 literally
    says ("synthetic random CSR"); the reference's kernels make no structure assumption (HPR_cuda_kernels.cu:297-427)."""
    return banded_lp(m, n, per_row, max(m, n), seed=seed)


def scaled_c3_lp(factor, seed=3):
    """The config-3 recipe (pds-20-like: ~2.2 entries per column, ~6.8 per row, +-1 values, uniformly random pattern = an
    expander) at `factor` times the size."""
    return G.planted_lp(33874 * factor, 105728 * factor, 230200 * factor, seed, values="network", dense_col_frac=0.0005 / factor)


# Size-and-structure ladder between config 3 (2.4e5 nnz) and config 5 (2e8): the Mittelmann regime.  Banded points use the
# config-5 generator; the block-angular point (hpr-lp-c_amd/lpgen.py) carries 200 linking rows and 200 linking columns of 5000
# entries (the long-row paths); round 4: a uniformly random pattern (no structure to find: the propagation-blocking form) and the
# config-3 recipe x 30 (an expander with 2-7 entries per row / column).
LADDER_POINTS = {
    "band_2e6": lambda: banded_lp(100_000, 100_000, 20, 1_000),
    "band_2e7": lambda: banded_lp(1_000_000, 1_000_000, 20, 10_000),
    "band_6e7": lambda: banded_lp(3_000_000, 3_000_000, 20, 30_000),
    "block_angular_2e7": lambda: G.block_angular_lp(1000, 1000, 2000, 18, 200, 200, 5000, 7),
    "unstructured_4e7": lambda: uniform_random_lp(2_000_000, 2_000_000, 20),
    "expander_7e6": lambda: scaled_c3_lp(30),
    # what ONE rank of a 2 / 4 / 8-GPU run of config 5 holds (round 5): the y-half of these points is a rank's half-step on
    # its whole shard -- the figures `predicted_scaling` is made of
    "c5_shard_of_2": lambda: shard_rows_lp("c5", 2),
    "c5_shard_of_4": lambda: shard_rows_lp("c5", 4),
    "c5_shard_of_8": lambda: shard_rows_lp("c5", 8),
}
SHARD_POINTS = {2: "c5_shard_of_2", 4: "c5_shard_of_4", 8: "c5_shard_of_8"}


def thread_rank_rehearsal(model, world, steps, lam):
    """The sharded solver's REAL code path at `world` ranks -- shard extraction, halo plans, split local / remote launches, pack /
    scatter, the exchange itself as device copies -- with the ranks as threads of this process time-sharing the ONE GPU
    (hprlp_solver_create_local; tools/dist_rehearsal.py is the stand-alone form).  Wall time of `steps` iterations of all ranks
    together; / world = GPU time per rank and iteration, host barriers of the in-process exchange included: an upper bound of
    what a rank of a `world`-GPU run needs per iteration, not a measurement of one."""
    import threading
    group = H.Solver.local_group(world)
    out, err = [None] * world, [None] * world
    prm = H.Parameters(stop_tol=1e-4, use_presolve=False)

    def work(rank):
        try:
            s = H.Solver.create_local(model, prm, rank, world, group)
            s.scale()
            s.init(-1.0, lam * 1.01)
            s.iterate(5)
            t = time.time()
            s.iterate(steps)
            s.residuals(steps + 6, True)   # (ends with a fetch: everything has run)
            out[rank] = (time.time() - t, s.dist_info(), s.describe())
            s.close()
        except Exception as e:  # noqa: BLE001
            err[rank] = repr(e)

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    H.Solver.free_local_group(group)
    if any(err):
        return {"error": str([e for e in err if e][0])[:300]}
    ms_all = 1e3 * max(o[0] for o in out) / steps
    mid = out[world // 2]
    return {"ms_per_iteration_all_ranks_on_one_gpu": ms_all, "gpu_ms_per_rank_iteration": ms_all / world, "steps": steps,
            "middle_rank_entries_received_per_iteration": mid[1]["m_received"] + mid[1]["n_received"], "middle_rank_kernels": kernel_forms(mid[2])}


def predicted_scaling(iteration_ms_1gpu, ladder_out):
    """What the first N > 1 record can be held against: per-rank kernel time at P ranks = 2 x the y-half of the rank's shard
    (the x-half runs the same shape: rows of A^T, by the band's symmetry), x 1.05 for the split into a local-column and a
    remote-column launch that the overlapped exchange needs (measured with thread ranks, HISTORY.md section 5), + the exposed
    part of the exchange (model: 0.01 / 0.02 / 0.03 ms at 2 / 4 / 8 ranks; the rest hides behind the local-column launch).
    A MODEL from one-GPU measurements of this run, not a measurement of N GPUs."""
    out = {"basis": "this run: config 5 iteration on one GPU, y-half launches of the shard-shaped ladder points", "P1_iteration_ms": iteration_ms_1gpu}
    exposed = {2: 0.01, 4: 0.02, 8: 0.03}
    for P, key in SHARD_POINTS.items():
        pt = (ladder_out or {}).get(key) or {}
        if "yhalf_ms" not in pt:
            out[f"P{P}"] = {"error": pt.get("error", "shard point not measured")}
            continue
        k = 2.0 * pt["yhalf_ms"]
        it = 1.05 * k + exposed[P]
        out[f"P{P}"] = {"shard_yhalf_ms": pt["yhalf_ms"], "shard_yhalf_frac_of_8000": pt["yhalf_frac_of_8000"], "kernels_ms": k, "iteration_ms_model": it,
                        "speedup_model": iteration_ms_1gpu / it, "speedup_kernels_only": iteration_ms_1gpu / k, "shard_kernel": pt["kernels"].split("A^T:")[0].strip()}
    return out


# The four Mittelmann-family generators at table size (lpgen.FAMILIES_LARGE): `--ladder-point family_<name>` measures their
# half-steps the same way; they are not part of the default ladder (generation takes longer than the measurement).
FAMILY_POINTS = {"family_" + k: mk for k, mk in G.FAMILIES_LARGE.items()}


def kernel_forms(description):
    """hprlp_solver_describe without its tail of environment switches (csrc/env.h): the kernel forms alone, the key the counter
    files are matched by."""
    return description.split("; switches:")[0].split("; ignored without")[0]


def ladder_traffic(key, kernels):
    """FETCH / WRITE counters of this ladder point (profiles/pmc_traffic.json, entry "ladder:<key>", collected by
    tools/profile_ladder.sh in separate rocprofv3 --pmc passes): carried only if they were taken on the kernel forms this run
    chose (`kernels` = hprlp_solver_describe)."""
    tf = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        ent = json.load(open(tf)).get("ladder:" + key)
    except Exception:  # noqa: BLE001
        ent = None
    if not ent:
        return None
    src = {"file": "profiles/pmc_traffic.json", "entry": "ladder:" + key, "commit": ent.get("commit"), "date": ent.get("date")}
    if ent.get("kernels") != kernels:
        return {"xhalf_hbm_bytes_per_launch": None, "yhalf_hbm_bytes_per_launch": None,
                "source": dict(src, note="counters were taken on other kernel forms: traffic withheld", counters_kernels=ent.get("kernels"))}
    return {"xhalf_hbm_bytes_per_launch": ent.get("xhalf_hbm_bytes_per_launch"), "yhalf_hbm_bytes_per_launch": ent.get("yhalf_hbm_bytes_per_launch"),
            "source": src}


def ladder_point(key, steps=100, warmup=20, timed=True):
    """One ladder point: which kernels the library chose, the half-step times by HIP events around every kernel
    (hprlp_solver_time_iterations mode 1), the algorithmic-bytes fraction of 8 TB/s and -- from the counter passes -- the HBM
    bytes a half-step really moves and their ratio to the algorithmic bytes."""
    if key.startswith("banded_"):  # banded_<rows>_<entries per row>_<band>: sweeps of the kernel-form decision (tools/ab_forms.sh)
        rows_, per_row_, band_ = (int(v) for v in key.split("_")[1:4])
        lp = banded_lp(rows_, rows_, per_row_, band_)
    else:
        lp = (LADDER_POINTS.get(key) or FAMILY_POINTS[key])()
    # A rank's two matrices are both shard-shaped.  The stand-alone LP of a shard point has the (m / P) x n matrix as A only -- its A^T
    # (n rows, most of them nearly empty) is not what a rank holds, and whether A's remainder products come by hand-off depends on it.
    # At 2 ranks both of a rank's matrices run the fused tiled kernel, whose epilogue hands the other half's products over: the
    # point forces the tiled form on A^T too (test hook).  At 4 and 8 ranks both run the PIECE form, which does not hand over: every
    # half-step runs its own remainder pre-pass -- which is what the point measures as it stands (its A^T keeps the stream kernel:
    # the row-block balance rule declines it, and a stream kernel hands nothing over).
    hooks = {"HPRLP_TEST_HOOKS": "1", "HPRLP_TILED_ANYWAY": "1"} if key == SHARD_POINTS[2] else {}
    saved = {k: os.environ.get(k) for k in hooks}
    os.environ.update(hooks)
    try:
        return _ladder_point_of(key, lp, steps, warmup, timed)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _ladder_point_of(key, lp, steps, warmup, timed):
    m, n, nnz = lp["m"], lp["n"], len(lp["values"])
    model = H.Model.from_csr(m, n, lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    del lp
    s = H.Solver(model, H.Parameters(stop_tol=1e-4, use_presolve=False))
    s.scale()
    lam, _ = s.power_iteration(max_iter=50)
    s.init(-1.0, lam * 1.01)
    info = s.info()
    t = s.time_iterations(warmup, steps, 1)
    g = s.time_iterations(warmup, steps, 0) if timed else t  # as the product runs it (graph replay where it applies)
    s.iterate(0, True)
    res = s.residuals(2 * steps + 41)
    x_ms, y_ms = t["xhalf_ms"] / steps, t["yhalf_ms"] / steps
    bx, by = bytes_x_half(m, n, nnz), bytes_y_half(m, n, nnz)
    kernels = kernel_forms(s.describe())
    out = {"m": m, "n": n, "nnz": nnz, "kernels": kernels, "tiled_flags": info["tiled"], "reordered_at_setup": bool(info.get("reordered")),
           "iterations_per_s": steps / (g["total_ms"] * 1e-3), "xhalf_ms": x_ms, "yhalf_ms": y_ms,
           "xhalf_frac_of_8000": bx / (x_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "yhalf_frac_of_8000": by / (y_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "iteration_frac_of_8000": bytes_per_iteration(m, n, nnz) * steps / (g["total_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "xhalf_algorithmic_bytes": bx, "yhalf_algorithmic_bytes": by,
           "finite": bool(np.isfinite(res["kkt"]))}
    tr = ladder_traffic(key, kernels)
    if tr is not None:
        out["traffic"] = tr
        if tr.get("xhalf_hbm_bytes_per_launch"):
            out["traffic"]["xhalf_ratio_to_algorithmic"] = tr["xhalf_hbm_bytes_per_launch"] / bx
            out["traffic"]["yhalf_ratio_to_algorithmic"] = tr["yhalf_hbm_bytes_per_launch"] / by
    s.close()
    model.free()
    return out


def ladder():
    out = {}
    for key in LADDER_POINTS:
        try:
            out[key] = ladder_point(key)
        except Exception as e:  # noqa: BLE001
            out[key] = {"error": str(e)}
    return out


DUMP_SAMPLE = 1 << 21  # entries per dumped vector at most: x and y of config 5 as float64 stay at 32 MB together


def dump_outputs(s, directory, cap):
    """--dump-outputs: x and y as the timed steps left them, in the caller's numbering (hprlp_solver_get_vector; at N > 1 this
    rank's rows / columns), float64.  A vector longer than DUMP_SAMPLE is written as the same seeded sample of DUMP_SAMPLE
    positions on every run, so that two builds can be compared entry for entry."""
    os.makedirs(directory, exist_ok=True)
    L = H.lib()
    buf = np.empty(max(cap, 1))
    for name in ("x", "y"):
        k = L.hprlp_solver_get_vector(s.h, name.encode(), buf.ctypes.data_as(H.c_dbl_p), len(buf))
        if k < 0:
            raise RuntimeError(H.last_error())
        v = buf[:k]
        if k > DUMP_SAMPLE:
            v = v[np.sort(np.random.default_rng(2024).choice(k, DUMP_SAMPLE, replace=False))]
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(v, dtype=np.float64))


def xhalf_kernel_key(tiled, description=""):
    """Short identity of the kernel avg_launch_ms covers; tools/profile_c5.sh stores the same key beside the counters it collects,
    and the bench line carries `traffic` only when the two agree.  k_tiled_fused<XEpi<false, true>, REP, PUSH, NARROW>: the key
    names PUSH (hand-off) and NARROW (1024-column tiles, from hprlp_solver_describe of A^T)."""
    if not tiled & 2:
        return "k_spmv_fused<XEpi<false>>"
    at = description.split("A^T:")[-1]
    if "all-remainder form" in at:
        return "k_pb_fused<XEpi<false, true>>"
    push = os.environ.get("HPRLP_NO_FAR_PUSH", "0") != "1"
    return "k_tiled_fused<XEpi<false, true>, *, %s, %s>" % ("true" if push else "false", "true" if "tiles of 1024 columns" in at else "false")


def xhalf_kernel_label(tiled):
    """Name of what avg_launch_ms covers on one GPU (rocprofv3 kernel names in profiles/)."""
    if not tiled & 2:
        return "k_spmv_fused<XEpi<false>> (x-half: SpMV(A^T,y) + prox + Halpern)"
    if os.environ.get("HPRLP_NO_FAR_PUSH", "0") == "1":
        return ("k_far_products + k_tiled_fused<XEpi<false, true>> (x-half: SpMV(A^T,y) + prox + Halpern; avg_launch_ms = remainder "
                "pre-pass + fused kernel, the two launches of the half-step)")
    return ("k_tiled_fused<XEpi<false, true>, REP, PUSH=true, NARROW> (x-half: SpMV(A^T,y) + prox + Halpern in ONE launch; the products of its "
            "far-column remainder were written by the preceding y-half's epilogue and its own epilogue writes the y-half's "
            "(hand-off, DESIGN.md section 4); shard-shaped matrices: k_tiled_part + k_tiled_finish)")


# ---- N > 1: a supervisor that cannot end without saying why ---------------------------------------------------------------
# The ranks run in FRESH child processes of a parent that never touches a GPU (it loads neither torch.cuda nor lib/libhprlp.so and
# never execs).  The parent watches them: a rank that dies ends the tier, and so does SILENCE -- no new line on any rank's stderr
# for HPRLP_BENCH_STALL_S seconds (every phase of a rank announces itself: "[bench] rank r: phase ...") or a tier outliving its
# share of HPRLP_BENCH_BUDGET_S; the parent then terminates exactly the PIDs it started and moves to the next transport tier, in
# fresh processes again.  The line that comes out says which tier produced it and how the earlier ones ended.
TIERS = [
    # (name, environment of the ranks)
    ("rccl: two communicators, neighbour exchange overlapped with the local part of the half-steps", {}),
    ("rccl: one communicator, exchange in line (HPRLP_NO_OVERLAP=1)", {"HPRLP_NO_OVERLAP": "1", "HPRLP_BENCH_SINGLE_COMM": "1"}),
    ("rccl: one communicator, in-place all-gather (HPRLP_DIST_EXCHANGE=allgather)",
     {"HPRLP_NO_OVERLAP": "1", "HPRLP_BENCH_SINGLE_COMM": "1", "HPRLP_DIST_EXCHANGE": "allgather", "HPRLP_TEST_HOOKS": "1"}),  # (the exchange form is a test hook)
    ("host-staged shared memory between the processes, no RCCL (HPRLP_DIST_TRANSPORT=shm)", {"HPRLP_DIST_TRANSPORT": "shm"}),
]
TIER_WEIGHTS = [4.0, 2.5, 2.0, 2.5]


def _env_float(name, default):
    try:
        return float(os.environ.get(name, default))
    except ValueError:
        return float(default)


def run_tier(n, argv, tier, tier_env, limit_s, stall_s):
    """One attempt: n fresh rank processes.  Returns (json line or None, how it ended, seconds, last stderr lines)."""
    import collections
    import signal
    import socket
    import subprocess
    import threading
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    drop = ("TORCHELASTIC_", "GROUP_", "ROLE_", "LOCAL_WORLD_SIZE", "TORCH_NCCL_ASYNC_ERROR_HANDLING")
    base = {k: v for k, v in os.environ.items() if not k.startswith(drop)}
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HPRLP_BENCH_ROLE="rank", HPRLP_BENCH_TIER=str(tier),
                   HPRLP_BENCH_LAUNCHER=os.environ.get("HPRLP_BENCH_LAUNCHER", "bench.py supervisor") + " -> fresh rank processes")
        env.update(tier_env)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this pool
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE))
    log(f"[bench] tier {tier}: {TIERS[tier][0]}: started ranks as child processes {[p.pid for p in procs]} (127.0.0.1:{port}); "
        f"limit {limit_s:.0f}s, silence limit {stall_s:.0f}s")
    t0 = time.time()
    state = {"last": time.time()}
    tail = collections.deque(maxlen=12)

    def relay(r):
        for raw in procs[r].stderr:
            ln = raw.decode(errors="replace").rstrip("\n")
            state["last"] = time.time()
            tail.append(ln[:300])
            sys.stderr.write(ln + "\n")
            sys.stderr.flush()

    out0 = []
    threads = [threading.Thread(target=relay, args=(r,), daemon=True) for r in range(n)]
    threads.append(threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True))
    for t in threads:
        t.start()
    how = None
    alive = set(range(n))
    while alive and how is None:
        for r in sorted(alive):
            rc = procs[r].poll()
            if rc is None:
                continue
            alive.discard(r)
            if rc != 0:
                how = f"rank {r} exited with code {rc}"
                break
        now = time.time()
        if how is None and alive:
            if now - state["last"] > stall_s:
                how = f"stalled: no line from any rank for {stall_s:.0f}s"
            elif now - t0 > limit_s:
                how = f"over its time share of {limit_s:.0f}s"
        time.sleep(0.05)
    if how is not None:
        time.sleep(1.0)  # let the others print their own error
        for r in sorted(alive):
            if procs[r].poll() is None:
                procs[r].terminate()  # exactly the PIDs started above
        deadline = time.time() + 15
        for r in sorted(alive):
            try:
                procs[r].wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                procs[r].send_signal(signal.SIGKILL)
        for r in sorted(alive):
            try:
                procs[r].wait(timeout=20)
            except subprocess.TimeoutExpired:
                how += f"; rank {r} (pid {procs[r].pid}) did not die"
        log(f"[bench] tier {tier} ended: {how} (exit codes {[p.returncode for p in procs]})")
        return None, how, time.time() - t0, list(tail)
    for t in threads:
        t.join(timeout=10)
    line = None
    for ln in (out0[0] if out0 else b"").decode().splitlines():
        if ln.startswith("{"):
            line = ln
    if line is None:
        return None, "rank 0 printed no JSON line", time.time() - t0, list(tail)
    got = json.loads(line).get("n_gpus")
    if got != n:
        return None, f"rank 0 reported n_gpus={got}, wanted {n}", time.time() - t0, list(tail)
    return line, "ok", time.time() - t0, list(tail)


def supervise(n, argv, out_fd=1):
    """`python bench.py --gpus N` (N > 1): the staged fallback over TIERS.  Exit code 0 and ONE line on stdout, or non-zero and
    on stderr how every tier ended -- never a line for another number of GPUs than asked for."""
    budget = _env_float("HPRLP_BENCH_BUDGET_S", 1500.0)
    stall = _env_float("HPRLP_BENCH_STALL_S", 240.0)
    first = int(_env_float("HPRLP_BENCH_FIRST_TIER", 0))
    t0 = time.time()
    attempts = []
    for tier in range(first, len(TIERS)):
        left = budget - (time.time() - t0)
        if left < 20.0:
            attempts.append({"tier": tier, "name": TIERS[tier][0], "ended": "not started: the time budget is spent"})
            continue
        limit = left * TIER_WEIGHTS[tier] / sum(TIER_WEIGHTS[tier:])
        line, how, secs, tail = run_tier(n, argv, tier, TIERS[tier][1], limit, stall)
        attempts.append({"tier": tier, "name": TIERS[tier][0], "ended": how, "seconds": round(secs, 1)})
        if line is None:
            attempts[-1]["last_lines"] = tail[-6:]
            continue
        rec = json.loads(line)
        rec["transport"] = {"tier": tier, "name": TIERS[tier][0], "attempts": attempts,
                            "supervisor": {"budget_s": budget, "silence_limit_s": stall, "seconds": round(time.time() - t0, 1)}}
        sys.stdout.flush()
        os.write(out_fd, (json.dumps(rec) + "\n").encode())
        return 0
    log("[bench] no result line: every transport tier failed")
    for a in attempts:
        log(f"[bench]   tier {a['tier']} ({a['name']}): {a['ended']}")
    return 1


def supervise_under_launcher(n, argv):
    """The same when a launcher (python -m torch.distributed.run --nproc-per-node N) started N copies of this script: the
    copies become supervisors that make no HIP call; rank 0's runs the tiers (its fresh children are the one-process-per-GPU
    ranks, on their own rendezvous port), the others wait for its verdict over gloo and leave with the same exit code."""
    import datetime
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    budget = _env_float("HPRLP_BENCH_BUDGET_S", 1500.0)
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)  # (gloo announces its connections on the C-level stdout; stdout carries the one JSON line and nothing else)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=budget + 900.0))
    rc = torch.zeros(1, dtype=torch.int64)
    if rank == 0:
        os.environ["HPRLP_BENCH_LAUNCHER"] = "torch.distributed.run -> rank 0 as supervisor"
        try:
            rc[0] = supervise(n, argv, real_stdout)
        except BaseException as e:  # noqa: BLE001  (the waiting copies must hear about it)
            log(f"[bench] supervisor failed: {e!r}")
            rc[0] = 1
    dist.broadcast(rc, src=0)
    dist.destroy_process_group()
    return int(rc[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default=os.environ.get("HPRLP_BENCH_WORKLOAD", "c5"), choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-side", action="store_true", help="skip the config-2/3 side measurements")
    ap.add_argument("--no-cold-start", action="store_true", help="skip the fresh-process first-solve measurements of configs 2 and 3")
    ap.add_argument("--no-solve", action="store_true", help="skip the time-to-tolerance solve of the workload")
    ap.add_argument("--no-ladder", action="store_true", help="skip the size-and-structure ladder (2e6 .. 6e7 nnz)")
    ap.add_argument("--ladder-point", default=None,
                    help="run ONE ladder point and print its record (what tools/profile_ladder.sh puts under rocprofv3)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: bare SpMVs, KKT check, time to 1e-4, "
                         "configs 2-4, ladder, predicted scaling, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write x and y after the last timed step to DIR/<name>.npy (float64; a fixed sample of longer vectors)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be at least 1")
    if not args.full:  # a plain run: set-up, warm-up, the timed steps, the line
        args.no_cpu = args.no_side = args.no_cold_start = args.no_solve = args.no_ladder = True
    if args.ladder_point:
        sys.stdout.flush()
        real = os.dup(1)
        os.dup2(2, 1)  # (the library's banner goes to the C-level stdout)
        rec = ladder_point(args.ladder_point, steps=args.steps, warmup=args.warmup, timed=False)
        sys.stdout.flush()
        os.write(real, (json.dumps({args.ladder_point: rec}) + "\n").encode())
        return
    if args.gpus > 1 and os.environ.get("HPRLP_BENCH_ROLE") != "rank" and os.environ.get("HPRLP_BENCH_DIRECT") != "1":
        # (HPRLP_BENCH_DIRECT=1: the launcher's processes ARE the ranks, as in rounds 1-4: no watchdog, no fallback)
        if "WORLD_SIZE" not in os.environ:
            raise SystemExit(supervise(args.gpus, sys.argv[1:]))
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}: launch one copy per GPU (torch.distributed.run "
                             f"--nproc-per-node {args.gpus}), or leave WORLD_SIZE unset and bench.py starts the ranks itself")
        raise SystemExit(supervise_under_launcher(args.gpus, sys.argv[1:]))
    # The library prints its banner / "problem information" lines to the C-level stdout like the
    # reference does; stdout of this script must carry exactly one JSON line, so route fd 1 to
    # stderr for the duration of the run and keep the real stdout for the result.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("HPRLP_BENCH_ONE_DEVICE"):  # rehearsal of the multi-rank path on a one-GPU box (if RCCL allows it)
        local_rank = 0
    if world != args.gpus:  # never print a line whose n_gpus is not what --gpus asked for
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (torch.distributed.run "
                         f"--nproc-per-node {args.gpus}), or leave WORLD_SIZE unset and bench.py starts the ranks itself")

    tier = int(os.environ.get("HPRLP_BENCH_TIER", "0"))

    def phase(what):
        """Every phase of a rank announces itself on stderr (the supervisor's watchdog listens for silence).  Test hook:
        HPRLP_BENCH_TEST_HANG=<tier>:<rank>:<word> makes that rank of that tier sleep for ever at the first phase whose name
        contains <word> (tests/test_dist_cpu.py: a hung exchange must not cost the run its line)."""
        log(f"[bench] rank {rank}: phase {what}")
        hang = os.environ.get("HPRLP_BENCH_TEST_HANG")
        if hang:
            ht, hr, hw = hang.split(":", 2)
            if int(ht) == tier and int(hr) == rank and hw in what:
                log(f"[bench] rank {rank}: TEST HOOK: hanging at phase '{what}'")
                time.sleep(1e7)

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # gloo carries only the bootstrap (RCCL unique ids), barriers and the max-over-ranks of the
        # timing; the data path is RCCL inside lib/libhprlp.so.
        dist.init_process_group("gloo", rank=rank, world_size=world)
        ndev = torch.cuda.device_count()  # (counting devices does not initialise the GPU)
        if local_rank >= ndev:
            log(f"[bench] rank {rank}: needs GPU {local_rank}, this box has {ndev} -- the RCCL communicator cannot be built")

    m, n, per_row, band = WORKLOADS[args.workload]
    t0 = time.time()
    prm = H.Parameters(stop_tol=1e-4, use_presolve=False, device_number=local_rank)
    model = None
    if world > 1:
        if args.workload in PERMUTED:
            raise SystemExit("the permuted workloads are single-GPU (the locality ordering runs on the whole matrix)")
        # every rank generates ITS rows only; the rows of A^T come through one all-to-all (no rank holds the whole LP)
        phase("shard assembly")
        shard, obj_star, nnz_loc = banded_lp_shard(m, n, per_row, band, rank, world, dist)
        tn = torch.tensor([nnz_loc], dtype=torch.int64)
        dist.all_reduce(tn)
        nnz = int(tn[0])
        if rank == 0:
            import resource
            log(f"[bench] rank 0 assembled its shard of {args.workload} ({m}x{n}, nnz={nnz} over {world} ranks; {nnz_loc} here) "
                f"in {time.time() - t0:.1f}s, peak host RSS {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6:.2f} GB")
        t0 = time.time()
        # two unique ids: the exchange stream gets its own communicator (no communicator is driven from two streams)
        # (fallback tiers: one id = one communicator; HPRLP_DIST_TRANSPORT=shm: the id names a shared-memory segment instead)
        id_bytes = 128 if (os.environ.get("HPRLP_BENCH_SINGLE_COMM") == "1" or os.environ.get("HPRLP_DIST_TRANSPORT") == "shm") else 256
        uid = np.zeros(256 + 1, np.uint8)
        phase("transport ids")
        if rank == 0:
            log(f"[bench] rank 0: creating the RCCL unique ids for {world} ranks" if os.environ.get("HPRLP_DIST_TRANSPORT") != "shm" else
                f"[bench] rank 0: naming the shared-memory segment for {world} ranks")
            if H.lib().hprlp_dist_unique_id(uid.ctypes.data_as(C.c_void_p), id_bytes) != 0:
                log(f"[bench] rank 0: FAILED at communicator creation (unique id): {H.last_error()}")
                uid[256] = 1
        tu = torch.from_numpy(uid)
        dist.broadcast(tu, src=0)
        if uid[256]:
            raise SystemExit(3)  # every rank leaves: no line is better than a line for fewer GPUs
        phase(f"communicators and device set-up (rank {rank} of {world}, device {local_rank}, {id_bytes // 128} id(s))")
        try:
            s = H.Solver.create_dist_from_shard(shard, prm, rank, world, uid[:id_bytes])
        except Exception as e:  # noqa: BLE001
            log(f"[bench] rank {rank}: FAILED at communicator / solver creation: {e}")
            raise SystemExit(3)
        dinfo = s.dist_info()
        cinfo = s.dist_comm_info()
        # what RCCL itself says, from every rank: communicator sizes and the device each rank sits on
        tc = torch.tensor([cinfo["comm_ranks"], cinfo["comm_device"], cinfo["xcomm_ranks"], cinfo["hip_device"]], dtype=torch.int64)
        allc = [torch.zeros_like(tc) for _ in range(world)]
        dist.all_gather(allc, tc)
        comm_report = {"rccl_ranks": int(min(int(t[0]) for t in allc)),
                       "rccl_ranks_exchange_comm": int(min(int(t[2]) for t in allc)),
                       "devices": [int(t[1]) for t in allc], "hip_devices": [int(t[3]) for t in allc],
                       "overlap": bool(cinfo["overlap"]),
                       "transport": "shared memory (host-staged)" if os.environ.get("HPRLP_DIST_TRANSPORT") == "shm" else "rccl"}
        one_device = bool(os.environ.get("HPRLP_BENCH_ONE_DEVICE"))
        if one_device:
            comm_report["rehearsal"] = f"all {world} ranks on device 0 of a one-GPU box: NOT a {world}-GPU measurement"
        if comm_report["rccl_ranks"] != world or (len(set(comm_report["devices"])) != world and not one_device):
            log(f"[bench] rank {rank}: the transport reports {comm_report}: not {world} ranks on {world} distinct devices")
            raise SystemExit(3)
        del shard
    else:
        lp = banded_lp(m, n, per_row, band)
        if args.workload in PERMUTED:
            lp = permute_lp(lp)
        nnz = len(lp["values"])
        log(f"[bench] generated {args.workload}: {m}x{n}, nnz={nnz} in {time.time() - t0:.1f}s")
        model = H.Model.from_csr(m, n, lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
        lp.pop("rowptr"); lp.pop("colind"); lp.pop("values")
        t0 = time.time()
        s = H.Solver(model, prm)
        dinfo = None
        comm_report = None
        obj_star = lp["obj_star"]
        if args.no_solve:
            model.free()
            model = None
    phase("scaling")
    s.scale()
    phase("power iteration")
    lam, pw_it = s.power_iteration()
    s.init(-1.0, lam * 1.01)
    sc = s.scalars()
    info = s.info()
    tiled = info["tiled"]
    kernels_desc = kernel_forms(s.describe())
    if rank == 0:
        log(f"[bench] setup {time.time() - t0:.1f}s (device setup {sc['setup_time']:.2f}s, scaling {sc['scaling_time']:.2f}s, "
            f"power iteration {sc['power_time']:.2f}s / {pw_it} its, lambda_max={lam:.4g})")

    # ---- timed region: warmup W, then exactly K iterations between barrier+synchronize pairs
    phase(f"warm-up, {args.warmup} iterations")
    s.iterate(args.warmup)
    if dist:
        dist.barrier()
    phase(f"timed region, {args.steps} iterations")
    torch.cuda.set_device(local_rank)  # (for torch.cuda.synchronize below; the library selects its device itself)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    tm = s.time_iterations(0, args.steps, 1)  # eager launches with HIP events around every kernel
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t_start
    if dist:
        te = torch.tensor([elapsed, tm["xhalf_ms"], tm["yhalf_ms"]], dtype=torch.float64)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed, tm["xhalf_ms"], tm["yhalf_ms"] = float(te[0]), float(te[1]), float(te[2])
    if args.dump_outputs and rank == 0:
        dump_outputs(s, args.dump_outputs, max(m, n))

    spmv = s.time_iterations(2, 20, 2) if world == 1 and args.full else None  # bare SpMVs, outside the timed region
    res = None
    if args.full:
        # sanity: the iterate must be finite and the KKT error must not have blown up
        s.iterate(0, True)
        res = s.residuals(args.warmup + args.steps + 1)
        ok = np.isfinite(res["kkt"])

    out = None
    if rank == 0:
        P = world
        # per-rank algorithmic bytes of the dominant kernel (x-half): 1/P of the matrix and streams, full gather vector
        bx = (12 * nnz + 4 * (n + P) + 56 * n) / P + 8 * m
        x_ms = tm["xhalf_ms"] / args.steps
        y_ms = tm["yhalf_ms"] / args.steps
        achieved = bx / (x_ms * 1e-3) / 1e9
        # HBM bytes per launch from the PMC counters: collected in separate rocprofv3 passes (tools/profile_c5.sh), not in this run.
        # The line says where the figure comes from, and carries it only if it was taken on the kernel this run measured.
        traffic, traffic_source = None, None
        tf = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tf) and P == 1:
            try:
                ent = json.load(open(tf)).get(args.workload, {})
                traffic_source = {"file": "profiles/pmc_traffic.json", "entry": args.workload, "kernel": ent.get("kernel_key"),
                                  "commit": ent.get("commit"), "date": ent.get("date"), "this_run_kernel": xhalf_kernel_key(tiled, kernels_desc)}
                if ent.get("kernel_key") == xhalf_kernel_key(tiled, kernels_desc):
                    traffic = ent.get("xhalf_hbm_bytes_per_launch")
                else:
                    traffic_source["note"] = "counters were taken on another kernel: traffic withheld"
            except Exception as e:  # noqa: BLE001
                traffic, traffic_source = None, {"error": str(e)}
        out = {
            "metric": "HPR iterations/sec (FP64)", "value": args.steps / elapsed, "unit": "iterations/s",
            "n_gpus": P, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (f"BASELINE config 5: banded-random CSR LP {m}x{n}, nnz={nnz} " if args.workload == "c5" else
                                    f"{args.workload}: banded-random CSR LP {m}x{n}, nnz={nnz}"
                                    f"{', rows and columns renumbered at random' if args.workload in PERMUTED else ''} ") +
                                   f"({'row-partitioned over %d GPUs, 2 RCCL exchanges per iteration' % P if P > 1 else 'one GPU'})",
                       "reordered_at_setup": bool(info.get("reordered")),
                       "m": m, "n": n, "nnz": nnz, "parallelism": f"rowpart{P}",
                       "launcher": os.environ.get("HPRLP_BENCH_LAUNCHER", "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ
                                                  else "single process" if P == 1 else "external"),
                       "kernels": kernels_desc,
                       "rccl": comm_report,
                       "exchange": None if dinfo is None else {
                           "kind_m": "neighbour send/recv" if dinfo["m_sparse"] else "all-gather",
                           "kind_n": "neighbour send/recv" if dinfo["n_sparse"] else "all-gather",
                           "rank0_entries_received_per_iteration": (dinfo["m_received"] if dinfo["m_sparse"] else m - m // P)
                                                                   + (dinfo["n_received"] if dinfo["n_sparse"] else n - n // P)},
                       "bytes_per_iteration_algorithmic": bytes_per_iteration(m, n, nnz)},
            "roofline": {"bound": "hbm", "kernel": xhalf_kernel_label(tiled)
                         if P == 1 else "x-half window of one rank: local-column SpMV beside the exchange of y, then the remote-column fused kernel "
                                        "(k_spmv_fused<WithBase<XEpi<false>>>); avg_launch_ms is that window, exchange wait included",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_source, "algorithmic_bytes_per_launch": bx, "avg_launch_ms": x_ms,
                         "frac_of_achievable_6300": achieved / 6300.0,
                         "yhalf_avg_launch_ms": y_ms,
                         "yhalf_GBps": ((12 * nnz + 4 * (m + P) + 40 * m) / P + 8 * n) / (y_ms * 1e-3) / 1e9,
                         "iteration_GBps": bytes_per_iteration(m, n, nnz) / P / (1e-3 * (x_ms + y_ms)) / 1e9},
            # outside the timed region (rank 0): device set-up incl. transpose and tiled copies, scaling, power iteration
            "phases_s": {"device_setup": sc["setup_time"], "scaling": sc["scaling_time"], "power_iteration": sc["power_time"],
                         "power_iterations": int(pw_it)},
        }
        if res is not None:
            out["kkt_after_run"], out["finite"] = res["kkt"], bool(ok)
        if spmv is not None:
            # SpMV-only figure B_spmv = 12 nnz + 4 (rows+1) + 8 cols + 8 rows over the bare kernel's time,
            # against the 8.0 TB/s spec peak and the 6.3 TB/s the guide gives as achievable
            bat, ba = 12 * nnz + 4 * (n + 1) + 8 * m + 8 * n, 12 * nnz + 4 * (m + 1) + 8 * n + 8 * m
            t_at, t_a = spmv["xhalf_ms"] / 20, spmv["yhalf_ms"] / 20
            out["spmv_only"] = {"AT_y_ms": t_at, "A_xhat_ms": t_a, "AT_y_GBps": bat / (t_at * 1e-3) / 1e9,
                                "A_xhat_GBps": ba / (t_a * 1e-3) / 1e9,
                                "AT_y_frac_of_8000": bat / (t_at * 1e-3) / 1e9 / 8000.0,
                                "AT_y_frac_of_6300": bat / (t_at * 1e-3) / 1e9 / 6300.0}
    if world > 1 and not args.no_solve:
        # the metric's second half at N GPUs: the SAME sharded solver, set back to zero iterates, run to 1e-4 (a second solver
        # would need a second set of communicators).  Wall of the loop = max over ranks; scaling and the power iteration were
        # timed when this solver was prepared above.  Every rank takes part (the loop's reductions are collectives).
        ttt = None
        phase("solve to 1e-4 on the same ranks")
        try:
            s.reset()
            s.init(-1.0, lam * 1.01)
            dist.barrier()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r = s.run()
            torch.cuda.synchronize()
            dist.barrier()
            te = torch.tensor([time.perf_counter() - t1], dtype=torch.float64)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            loop_s = float(te[0])
            ttt = {"tol": 1e-4, "loop_seconds": loop_s, "power_iteration_seconds": sc["power_time"], "scaling_seconds": sc["scaling_time"],
                   "device_setup_seconds_rank0": sc["setup_time"],
                   # the reference's `time` = power iteration + loop (src/HPRLP.cu:150,246)
                   "solver_seconds": loop_s + sc["power_time"], "seconds": loop_s + sc["power_time"] + sc["scaling_time"] + sc["setup_time"],
                   "iterations": int(r.iter), "status": r.status, "kkt": float(r.residuals),
                   "rel_obj_err": (abs(r.primal_obj - obj_star) / (1 + abs(obj_star))) if obj_star is not None else None,
                   "note": "sharded solve on the N ranks of this run, from zero iterates; set-up = this rank's shard only"}
        except Exception as e:  # noqa: BLE001
            ttt = {"error": str(e)}
        if out is not None:
            out["time_to_tol"] = ttt
    s.close()
    rehearsal = None
    if rank == 0 and world == 1:
        if model is not None:
            # the metric's second half: wall time of a whole solve() to 1e-4 on the same LP (model already on the host;
            # includes transpose, tiling, scaling and the power iteration), checked against the planted optimum
            try:
                t1 = time.time()
                r = model.solve(H.Parameters(stop_tol=1e-4, use_presolve=False, time_limit=600.0))
                wall = time.time() - t1
                ph = H.last_solve_phases()
                # `seconds` = the harness's own clock around the C call solve() (hprlp.py: Model.solve, perf_counter before and
                # after the ctypes call: what a caller of the reference's ABI waits for); `c_call_seconds` = the library's own
                # figure for the same call (hprlp_last_solve_phases: whole_call; rounds 4's `seconds`), `python_wrapper_seconds`
                # adds the harness's wrapping of the three 80 MB solution vectors into numpy arrays
                out["time_to_tol"] = {"tol": 1e-4, "seconds": r.c_call_wall_s, "c_call_seconds": ph["whole_call"], "python_wrapper_seconds": wall,
                                      "solver_seconds": r.time, "iterations": r.iter,
                                      # the reference's own instrument (HPRLP_results.time4 / iter4, include/structs.h:50-57)
                                      "time4_s": r.time4, "iter4": r.iter4,
                                      "reference_style_iterations_per_s": r.iter / max(r.time, 1e-9),
                                      "status": r.status, "rel_obj_err": abs(r.primal_obj - obj_star) / (1 + abs(obj_star)),
                                      # where `seconds` goes (hprlp_last_solve_phases); the reference's `time` = power iteration + loop
                                      "phases_s": ph}
            except Exception as e:
                out["time_to_tol"] = {"error": str(e)}
            if args.workload == "c5" and not args.no_ladder and not args.no_side:
                # (while the model is still on the host) the sharded code path at 4 and 8 ranks as threads on this one GPU
                rehearsal = {}
                for P in (4, 8):
                    try:
                        rehearsal[P] = thread_rank_rehearsal(model, P, 30, lam)
                    except Exception as e:  # noqa: BLE001
                        rehearsal[P] = {"error": str(e)[:300]}
            model.free()
        if not args.no_side:  # before the CPU leg: its OpenMP team keeps spinning for a while and disturbs the
            try:              # latency-bound small solves
                out["other_configs"] = side_configs(cold_start=not args.no_cold_start)
            except Exception as e:
                out["other_configs"] = {"error": str(e)}
        if not args.no_ladder and not args.no_side:
            try:
                out["ladder"] = ladder()
            except Exception as e:  # noqa: BLE001
                out["ladder"] = {"error": str(e)}
            if args.workload == "c5":
                out["predicted_scaling"] = predicted_scaling(out["ms_per_step"], out["ladder"])
                if rehearsal is not None:
                    out["predicted_scaling"]["thread_rank_rehearsal"] = rehearsal
                    for P, r in rehearsal.items():
                        if "gpu_ms_per_rank_iteration" in r and f"P{P}" in out["predicted_scaling"]:
                            out["predicted_scaling"][f"P{P}"]["speedup_bound_from_rehearsal"] = out["ms_per_step"] / r["gpu_ms_per_rank_iteration"]
        if not args.no_cpu:
            try:
                out["cpu_baseline"] = cpu_baseline(args.workload)
            except Exception as e:  # the oracle is only a reported baseline; never fail the bench on it
                out["cpu_baseline"] = {"value": None, "unit": "iterations/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}
    if rank == 0:
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
