"""solve_batched against the oracle ITERATE BY ITERATE (GPU): what hpr-lp-c_amd/csrc/batched.hip's header claims -- every
member's row sums are added in CSR order, "so the result is bit-identical to the oracle's batched restatement" -- checked as
written, on the shapes where its kernels can go wrong.

How the claim becomes checkable.  solve_batched with max_iter = K returns every member's X_bar / Y_bar / Z_bar of the last
check-variant iteration (iteration K if K is a check or log step, an older one or the zeros of the start otherwise), mapped to the
caller's units by the same three operations on both sides.  No member has to be solvable for that: the batch holds unbounded
and infeasible members.  The two sides share every bit of their input when
  * lambda_max comes from the test through the hook HPRLP_BATCH_LAMBDA (float.hex() -> strtod) and the oracle's
    lambda_override: the two power iterations reduce in different orders (1e-12 relative, test_power_iteration_matches) and
    that alone would move every iterate in its last places;
  * Curtis-Reid scaling is off: Ruiz and Pock-Chambolle are bit-exact against the oracle (test_scaling_without_cr_is_bit_exact),
    both sides are built with -ffp-contract=off, and the per-member vector scaling runs on the host in the same order on
    both sides (bound_norm_host / column_norm_host in both files).
The first restart of any member happens at iter == check_iter; up to there no host decision depends on a device reduction:
  * K <= check_iter: np.array_equal on x, y, z of every member; status and iter equal outright; primal_obj / residuals / gap
    (device reductions) within 1e-11 * (1 + |reference|), the form test_residuals_and_weighted_norm uses for its objectives
    (gap = |p - d| / (1 + |p| + |d|) and the kkt maximum inherit the objectives' ABSOLUTE error, hence the same form);
  * K > check_iter: sigma after a restart carries the reduction order of four device sums, so equality is no longer owed.  The
    bound is measured on the reference side alone: the oracle runs twice at the same K, with lambda and with
    nextafter(lambda, inf); the largest difference of x, y, z between those two CPU runs, relative to the member's vector
    max-norm, is the sensitivity s(K) of the trajectory to a last-place change.  The GPU must agree with the oracle within
    max(64 * s(K), 1e-13) in the same measure (a restart feeds four reductions of a few hundred terms into sigma, each good for
    a few last places; the floor covers s = 0).

Which batch size reaches which kernel (padded_batch / choose_chunk in batched.hip; Bp = padded batch, Bc = chunk width):
  B = 1, 2, 3   -> Bp = 1, 2, 4, one chunk, kb_half (64, 32, 16 sub-rows per wave)
  B = 5, 12, 24 -> Bp = 8, 16, 32, one chunk, kb_halfN<8 | 16 | 32>
  B = 64        -> kb_half64, one chunk;  B = 70 -> Bp = 128, two chunks, 58 dead columns in the second;  B = 130 -> Bp = 192
  B = 70 with HPRLP_BATCH_CHUNK = 8, 16, 32 -> kb_halfN<..> with 16, 8, 4 chunks
  HPRLP_BATCH_GRID = 1, 3 -> every workgroup of the normal half-steps wraps in its row loop;  HPRLP_NO_GRAPH = 1 -> eager launches
The residual kernels kb_resid<0..3>, kb_lu, kb_movement, kb_restart and kb_finalize run in every one of these geometries.

The matrices.  "long": 123 x 205 (no multiple of 4, 16 or 32: the last row group is ragged in every kernel), a row of 150
entries and a column of 90 (both sides get a launch-order table), rows 60 and 122 and columns 33 and 204 empty.  "short":
121 x 207, at most 6 entries per row and per column (no table), last row and last column NOT empty -- the rows a group read
one row short would lose.  Per member and per row / column an independent draw of the bound kind (both finite, lower only,
upper only, free, equality row); c perturbed per member, member 1 with c = 0 (sigma falls back to 1), member 2 with an
objective constant.

The lambda bump (the reference's "estimated maximum eigenvalue is too small" rule) is reached by handing both sides a lambda
far below the power iteration's: tests at the end of the module, single solver and batch.

Measured on one MI355X (also DESIGN.md, "Batched parity"); worst over the batch shapes, in the measure above:
  long  check_iter  10  K  11   s(K) 3.8e-15   worst GPU-vs-oracle 9.0e-16
  long  check_iter  10  K  17   s(K) 3.8e-15   worst GPU-vs-oracle 9.0e-16
  long  check_iter  10  K  20   s(K) 7.2e-15   worst GPU-vs-oracle 3.8e-15
  long  check_iter  10  K  31   s(K) 1.5e-13   worst GPU-vs-oracle 1.5e-13
  long  check_iter 150  K 151   s(K) 1.9e-13   worst GPU-vs-oracle 4.3e-16
  long  check_iter 150  K 157   s(K) 1.9e-13   worst GPU-vs-oracle 4.3e-16
  long  check_iter 150  K 300   s(K) 1.5e-12   worst GPU-vs-oracle 2.3e-14
  long  check_iter 150  K 451   s(K) 6.8e-11   worst GPU-vs-oracle 8.4e-11
  short check_iter  10  K  11   s(K) 6.3e-15   worst GPU-vs-oracle 5.3e-16
  short check_iter  10  K  17   s(K) 6.3e-15   worst GPU-vs-oracle 5.3e-16
  short check_iter  10  K  20   s(K) 9.1e-15   worst GPU-vs-oracle 9.9e-15
  short check_iter  10  K  31   s(K) 4.1e-15   worst GPU-vs-oracle 6.1e-15
  short check_iter 150  K 151   s(K) 1.5e-13   worst GPU-vs-oracle 5.3e-16
  short check_iter 150  K 157   s(K) 1.5e-13   worst GPU-vs-oracle 5.3e-16
  short check_iter 150  K 300   s(K) 1.0e-12   worst GPU-vs-oracle 6.6e-14
  short check_iter 150  K 451   s(K) 2.2e-11   worst GPU-vs-oracle 2.0e-12
K <= check_iter: equal bits everywhere; scalars of the evaluation within 1.4e-15 of 1 + |reference|.  The bump case (B = 64,
check_iter 10, K = 53, a quarter of the true lambda; the oracle bumps at every evaluation from iteration 10 to 90): s = 2.0e-14,
GPU-vs-oracle 1.3e-13 with graphs and eager; 5.7e5 with graphs before BatchWS::drop_graphs (eager 1.3e-13 then too).
The module's oracle runs take about 5 s of CPU in all, the whole module 8 s on the GPU machine.
"""
import functools

import numpy as np
import pytest

from conftest import hprlp, lpgen
from oracle import oracle as O

pytestmark = pytest.mark.gpu
INF = np.inf
BMAX = 130
STOP_TOL = 1e-12  # no member ends early (asserted on the oracle's statuses)


# ---- matrices and the batch ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(kind):
    """(m, n, csr) of the "long" / "short" matrix of the module docstring."""
    from scipy import sparse
    if kind == "long":
        m, n, seed = 123, 205, 811
        rng = np.random.default_rng(seed)
        A = lpgen.planted_lp(m, n, 1000, seed, dense_col_frac=0.0)["A"].tolil()
        live_cols, live_rows = np.setdiff1d(np.arange(n), [33, n - 1]), np.setdiff1d(np.arange(m), [60, m - 1])
        A[17, rng.choice(live_cols, size=150, replace=False)] = rng.normal(size=150)
        A[rng.choice(live_rows, size=90, replace=False), 101] = rng.normal(size=90).reshape(-1, 1)
        A[60, :] = 0
        A[m - 1, :] = 0
        A[:, 33] = 0
        A[:, n - 1] = 0
    else:
        m, n, seed = 121, 207, 812
        rng = np.random.default_rng(seed)
        rows = np.concatenate([np.repeat(np.arange(m), 3), rng.integers(0, m, size=n)])
        cols = np.concatenate([rng.integers(0, n, size=3 * m), np.arange(n)])  # every column, three per row and a few more
        A = sparse.csr_matrix((rng.normal(size=len(rows)), (rows, cols)), shape=(m, n)).tolil()
        A[m - 1, n - 1] = 1.5
    A = sparse.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return m, n, A


@functools.lru_cache(maxsize=None)
def batch(kind):
    """The BMAX-member batch on matrix(kind): dict of the csr arrays, the panels (rows x BMAX) and obj_constants."""
    m, n, A = matrix(kind)
    rng = np.random.default_rng(97 if kind == "long" else 98)
    base = lpgen._plant(np.random.default_rng(5), A)
    B = BMAX
    xs, bs = base["x_star"][:, None], (A @ base["x_star"])[:, None]
    # columns: 0 both finite, 1 lower only, 2 upper only, 3 free
    ck = rng.integers(0, 4, size=(n, B))
    L = xs - rng.uniform(0.0, 1.5, size=(n, B))
    U = xs + rng.uniform(0.0, 2.0, size=(n, B))
    L = np.where((ck == 2) | (ck == 3), -INF, L)
    U = np.where((ck == 1) | (ck == 3), INF, U)
    # rows: 0 both finite, 1 lower only, 2 upper only, 3 free, 4 equality
    rk = rng.integers(0, 5, size=(m, B))
    mid = bs + 0.2 * rng.normal(size=(m, B))
    AL = mid - np.abs(rng.normal(size=(m, B)))
    AU = mid + np.abs(rng.normal(size=(m, B)))
    AL = np.where((rk == 2) | (rk == 3), -INF, AL)
    AU = np.where((rk == 1) | (rk == 3), INF, AU)
    AL = np.where(rk == 4, mid, AL)
    AU = np.where(rk == 4, mid, AU)
    Cm = base["c"][:, None] * (1 + 0.1 * rng.normal(size=(n, B))) + 0.05 * rng.normal(size=(n, B))
    Cm[:, 1] = 0.0
    objc = np.zeros(B)
    objc[2] = 7.25
    # members differ in kind within one row / one column, and every kind occurs
    assert all(len(np.unique(ck[j])) > 1 for j in range(n)) and all(len(np.unique(rk[i])) > 1 for i in range(m))
    assert set(np.unique(ck)) == {0, 1, 2, 3} and set(np.unique(rk)) == {0, 1, 2, 3, 4}
    return dict(m=m, n=n, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy(),
                C=Cm, AL=AL, AU=AU, L=L, U=U, objc=objc)


def test_the_matrices_are_what_the_docstring_says():
    m, n, A = matrix("long")
    rl, cl = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    assert (m, n) == (123, 205) and all(m % g and n % g for g in (4, 16, 32))
    assert rl.max() >= 150 and cl.max() >= 90 and 1100 <= A.nnz <= 1500
    assert rl[60] == 0 and rl[m - 1] == 0 and cl[33] == 0 and cl[n - 1] == 0
    m, n, A = matrix("short")
    rl, cl = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    # no launch-order table: no lane group's four rows hold more than kLongGroup = 32 entries
    assert 4 * rl.max() <= 32 and 4 * cl.max() <= 32 and rl[m - 1] > 0 and cl[n - 1] > 0 and m % 4 and n % 4


@functools.lru_cache(maxsize=None)
def lam_of(kind):
    """1.01 x the oracle's power iteration on the shared matrix as solve_batched scales it (zero vectors, no CR, no b/c)."""
    b = batch(kind)
    m, n = b["m"], b["n"]
    sl = O.ScaledLP(m, n, b["rowptr"], b["colind"], b["values"], np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(n),
                    O.Params.default(use_CR_scaling=0, use_bc_scaling=0))
    return sl.power_iteration()[0] * 1.01


@functools.lru_cache(maxsize=None)
def oracle_run(kind, K, check_iter, lam):
    """The oracle on all BMAX members (members are independent while lambda is not bumped: smaller batches are slices)."""
    b = batch(kind)
    return O.solve_batched(b["m"], b["n"], b["rowptr"], b["colind"], b["values"], BMAX, b["C"].T.ravel(), b["AL"].T.ravel(),
                           b["AU"].T.ravel(), b["L"].T.ravel(), b["U"].T.ravel(), b["objc"], lambda_override=lam,
                           params=O.Params.default(max_iter=K, stop_tol=STOP_TOL, check_iter=check_iter, use_CR_scaling=0))


def gpu_run(monkeypatch, kind, B, K, check_iter, lam, env=()):
    b = batch(kind)
    model = hprlp.Model.from_csr(b["m"], b["n"], b["rowptr"], b["colind"], b["values"], np.zeros(b["m"]), np.zeros(b["m"]),
                                 np.zeros(b["n"]), np.zeros(b["n"]), np.zeros(b["n"]))
    prm = hprlp.Parameters(max_iter=K, stop_tol=STOP_TOL, check_iter=check_iter, use_CR_scaling=False, use_presolve=False)
    with monkeypatch.context() as mp:
        mp.setenv("HPRLP_BATCH_LAMBDA", float(lam).hex())
        for k, v in env:
            mp.setenv(k, v)
        r = hprlp.solve_batched(model, b["C"][:, :B], b["AL"][:, :B], b["AU"][:, :B], b["L"][:, :B], b["U"][:, :B], b["objc"][:B], prm)
    model.free()
    assert r["batch_size"] == B and r["x"] is not None, hprlp.last_error()
    for name in ("x", "y", "z"):
        r[name] = np.ascontiguousarray(r[name].T)  # members x vector, as the oracle returns them
    return r


def rel_diff(r, ref, B):
    """Largest difference of x, y, z over the first B members, relative to the member's vector max-norm in the reference."""
    worst = 0.0
    for name in ("x", "y", "z"):
        a, w = r[name][:B], ref[name][:B]
        scale = np.maximum(np.abs(w).max(axis=1), np.finfo(float).tiny)
        worst = max(worst, float((np.abs(a - w).max(axis=1) / scale).max()))
    return worst


def check_common(r, ref, B, tag):
    assert r["status"] == ref["status"][:B], tag
    assert list(r["iter"]) == list(ref["iter"][:B]), tag
    for name in ("x", "y", "z", "primal_obj", "residuals", "gap"):
        assert np.isfinite(r[name]).all(), (tag, name)


# ---- section 1: state parity through the iteration limit ---------------------------------------------------------------
# (matrix, B, hooks)
CONFIGS = [("long", B, ()) for B in (1, 2, 3, 5, 12, 24, 64, 70, 130)]
CONFIGS += [("long", 70, (("HPRLP_BATCH_CHUNK", str(c)),)) for c in (8, 16, 32)]
CONFIGS += [("long", B, (("HPRLP_BATCH_GRID", g),)) for B in (64, 5) for g in ("1", "3")]
CONFIGS += [("long", 64, (("HPRLP_NO_GRAPH", "1"),))]
CONFIGS += [("short", B, ()) for B in (3, 12, 64, 70)]
CONFIGS += [("short", 70, (("HPRLP_BATCH_CHUNK", "16"),)), ("short", 64, (("HPRLP_BATCH_GRID", "3"),))]
IDS = ["%s-B%d%s" % (k, B, "".join("-%s=%s" % (a.replace("HPRLP_", ""), v) for a, v in env)) for k, B, env in CONFIGS]

# (check_iter, K).  Check-variant iterations are those before a periodic check or a log step (every 10th): at check_iter = 150,
# K = 1, 2, 7 return the zeros of the start, 13 the bars of iteration 10, 149 those of 140.  check_iter = K = 1, 2, 7 makes
# the last iteration a check variant, so that the first iterations' states are looked at as well.
K_EXACT = [(150, K) for K in (0, 1, 2, 7, 10, 13, 100, 149, 150)] + [(10, K) for K in (1, 2, 7, 9, 10)] + [(1, 1), (2, 2), (7, 7)]
K_AFTER = [(150, K) for K in (151, 157, 300, 451)] + [(10, K) for K in (11, 17, 20, 31)]
RTOL_SCALARS = 1e-11


@pytest.mark.parametrize("kind,B,env", CONFIGS, ids=IDS)
def test_iterates_are_the_oracles_bits_up_to_the_first_restart(gpu, monkeypatch, kind, B, env):
    lam = lam_of(kind)
    for check_iter, K in K_EXACT:
        ref = oracle_run(kind, K, check_iter, lam)
        assert ref["lambda_max"] == lam and ref["status"] == ["ITER_LIMIT"] * BMAX  # no bump, nobody ends early
        r = gpu_run(monkeypatch, kind, B, K, check_iter, lam, env)
        tag = (kind, B, env, check_iter, K)
        check_common(r, ref, B, tag)
        for name in ("x", "y", "z"):
            got, want = r[name], ref[name][:B]
            bad = np.argwhere(got != want)
            assert np.array_equal(got, want), (tag, name, "first (member, index):", bad[0].tolist(), "of", len(bad),
                                               float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
        if K in (0, check_iter):  # the evaluation at K: device reductions against the oracle's sequential sums
            for name in ("primal_obj", "residuals", "gap"):
                dev = np.abs(r[name] - ref[name][:B]) / (1 + np.abs(ref[name][:B]))
                print("scalars", tag, name, "max deviation / (1 + |ref|) = %.3g" % dev.max())
                assert (dev <= RTOL_SCALARS).all(), (tag, name, int(dev.argmax()), float(dev.max()))
    # what the oracle says about the odd limits: 13 returns the bars of iteration 10, 7 the zeros of the start
    assert np.array_equal(oracle_run(kind, 13, 150, lam)["x"], oracle_run(kind, 10, 150, lam)["x"])
    assert not oracle_run(kind, 7, 150, lam)["y"].any() and oracle_run(kind, 7, 7, lam)["y"].any()


@functools.lru_cache(maxsize=None)
def sensitivity(kind, K, check_iter):
    """s(K): the oracle against itself with lambda one place up (module docstring)."""
    lam = lam_of(kind)
    a, b = oracle_run(kind, K, check_iter, lam), oracle_run(kind, K, check_iter, float(np.nextafter(lam, INF)))
    assert a["status"] == b["status"] and list(a["iter"]) == list(b["iter"])
    return rel_diff(b, a, BMAX)


def bound_of(s):
    return max(64.0 * s, 1e-13)


@pytest.mark.parametrize("kind,B,env", CONFIGS, ids=IDS)
def test_iterates_after_restarts_stay_within_the_oracles_own_sensitivity(gpu, monkeypatch, kind, B, env):
    lam = lam_of(kind)
    for check_iter, K in K_AFTER:
        ref = oracle_run(kind, K, check_iter, lam)
        assert ref["lambda_max"] == lam and ref["status"] == ["ITER_LIMIT"] * BMAX
        s = sensitivity(kind, K, check_iter)
        r = gpu_run(monkeypatch, kind, B, K, check_iter, lam, env)
        tag = (kind, B, env, check_iter, K)
        check_common(r, ref, B, tag)
        d = rel_diff(r, ref, B)
        print("after-restart", tag, "s(K) = %.3g  bound = %.3g  gpu-vs-oracle = %.3g" % (s, bound_of(s), d))
        assert d <= bound_of(s), (tag, s, d)


def test_a_member_has_the_same_bits_in_every_batch_it_is_in(gpu, monkeypatch):
    """Member k of B = 130 against member k of B = 5 (kb_half64 in three chunks / kb_halfN<8>) and of B = 3 (kb_half): the GPU
    side alone, so this holds whatever the oracle says."""
    lam = lam_of("long")
    big = gpu_run(monkeypatch, "long", 130, 150, 150, lam)
    for B in (5, 3):
        small = gpu_run(monkeypatch, "long", B, 150, 150, lam)
        for name in ("x", "y", "z"):
            assert np.array_equal(small[name], big[name][:B]), (B, name)


# ---- section 2: the lambda bump ------------------------------------------------------------------------------------------
BUMP_FRACTION = 0.25  # of the power iteration's lambda: the oracle's trace shows the bump (asserted below)


def first_rise(trace):
    """Index of the first trace row whose lambda_max exceeds the first row's (None: never)."""
    return next((i for i, t in enumerate(trace) if t["lambda_max"] > trace[0]["lambda_max"]), None)


def test_single_solver_bumps_lambda_where_the_oracle_does(gpu):
    lp = lpgen.planted_lp(200, 320, 2000, 31)
    model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"],
                                 lp["u"], lp["c"])
    tol, max_iter = 1e-6, 20000
    s = hprlp.Solver(model, hprlp.Parameters(stop_tol=tol, max_iter=max_iter, use_presolve=False))
    s.scale()
    lam, _ = s.power_iteration()
    lam_small = BUMP_FRACTION * lam
    s.init(-1.0, lam_small)
    res = s.run()
    ref = O.solve(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                  params=O.Params.default(stop_tol=tol, max_iter=max_iter), lambda_override=lam_small)
    i_ref, i_gpu = first_rise(ref["trace"]), first_rise(res.trace)
    assert i_ref is not None, "the oracle never bumps lambda for this LP and fraction: the case tests nothing"
    assert i_gpu == i_ref and res.trace[i_gpu]["iter"] == ref["trace"][i_ref]["iter"]
    a, b = res.trace[i_gpu]["lambda_max"], ref["trace"][i_ref]["lambda_max"]
    print("single bump at trace row %d (iteration %d): %.17g -> gpu %.17g oracle %.17g" % (i_ref, ref["trace"][i_ref]["iter"],
                                                                                      lam_small, a, b))
    assert abs(a - b) <= 1e-9 * b and b > lam_small
    assert res.status == ref["status"]
    s.close(); model.free()


BUMP_CHECK_ITER, BUMP_B = 10, 64


@functools.lru_cache(maxsize=None)
def oracle_bump_run(K, lam):
    """The oracle on the first BUMP_B members (a bump couples the members through the shared lambda: no slicing here)."""
    b = batch("long")
    B = BUMP_B
    return O.solve_batched(b["m"], b["n"], b["rowptr"], b["colind"], b["values"], B, b["C"][:, :B].T.ravel(),
                           b["AL"][:, :B].T.ravel(), b["AU"][:, :B].T.ravel(), b["L"][:, :B].T.ravel(), b["U"][:, :B].T.ravel(),
                           b["objc"][:B], lambda_override=lam,
                           params=O.Params.default(max_iter=K, stop_tol=STOP_TOL, check_iter=BUMP_CHECK_ITER, use_CR_scaling=0))


def bump_case():
    """(lam_small, first bump, K): a quarter of the batch's lambda, the first iteration limit at which the oracle returns a larger
    one, and an iteration limit a few check periods after that."""
    lam_small = BUMP_FRACTION * lam_of("long")
    at = None
    for K in range(BUMP_CHECK_ITER, 40 * BUMP_CHECK_ITER + 1, BUMP_CHECK_ITER):
        if oracle_bump_run(K, lam_small)["lambda_max"] > lam_small:
            at = K
            break
    assert at is not None, "the oracle never bumps lambda for this batch and fraction: the case tests nothing"
    return lam_small, at, at + 4 * BUMP_CHECK_ITER + 3


@pytest.mark.parametrize("graphs", ["graphs", "eager"])
def test_batch_follows_the_oracle_through_a_lambda_bump(gpu, monkeypatch, graphs):
    """Both sides start from a lambda far too small; the oracle raises it at some evaluation (the condition below keeps the case
    honest), and a few check periods later the GPU's iterates must still be the oracle's within the s(K) bound.  The normal
    iterations are replayed hipGraphs that hold lambda by value: a replay that kept the lambda of its capture would miss the
    bound by many orders of magnitude (it did, before BatchWS::drop_graphs)."""
    lam_small, at, K = bump_case()
    ref = oracle_bump_run(K, lam_small)
    assert ref["lambda_max"] > lam_small                                                       # (a)
    up = oracle_bump_run(K, float(np.nextafter(lam_small, INF)))
    assert up["status"] == ref["status"] and list(up["iter"]) == list(ref["iter"])
    s = rel_diff(up, ref, BUMP_B)
    env = (("HPRLP_NO_GRAPH", "1"),) if graphs == "eager" else ()
    r = gpu_run(monkeypatch, "long", BUMP_B, K, BUMP_CHECK_ITER, lam_small, env)
    check_common(r, ref, BUMP_B, (graphs, K))                                                  # (b)
    d = rel_diff(r, ref, BUMP_B)
    print("bump", graphs, "oracle bumps by iteration %d: %.17g -> %.17g; K = %d  s(K) = %.3g  bound = %.3g  gpu-vs-oracle = %.3g"
          % (at, lam_small, ref["lambda_max"], K, s, bound_of(s), d))
    assert d <= bound_of(s), (graphs, K, s, d)                                                 # (c)


# ---- the hook itself -------------------------------------------------------------------------------------------------------
def test_the_lambda_hook_is_listed_and_ignored_without_the_gate(gpu, monkeypatch):
    import ctypes as C
    L = hprlp.lib()
    n = L.hprlp_env_switches(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.hprlp_env_switches(buf, n + 1)
    table = dict(ln.split("\t")[:2] for ln in buf.value.decode().splitlines())
    assert table["HPRLP_BATCH_LAMBDA"] == "hook" and table["HPRLP_BATCH_GRID"] == "hook"
    b = batch("short")
    model = hprlp.Model.from_csr(b["m"], b["n"], b["rowptr"], b["colind"], b["values"], np.zeros(b["m"]), np.zeros(b["m"]),
                                 np.zeros(b["n"]), np.zeros(b["n"]), np.zeros(b["n"]))
    prm = hprlp.Parameters(max_iter=40, stop_tol=STOP_TOL, check_iter=10, use_CR_scaling=False, use_presolve=False)
    run = lambda: hprlp.solve_batched(model, b["C"][:, :5], b["AL"][:, :5], b["AU"][:, :5], b["L"][:, :5], b["U"][:, :5], None, prm)
    plain = run()
    small = (BUMP_FRACTION * lam_of("short")).hex()
    monkeypatch.setenv("HPRLP_BATCH_LAMBDA", small)
    hooked = run()
    assert not np.array_equal(hooked["y"], plain["y"])                       # with the gate (conftest sets it) the hook acts
    monkeypatch.delenv("HPRLP_TEST_HOOKS")
    ignored = run()
    for name in ("x", "y", "z"):
        assert np.array_equal(ignored[name], plain[name]), name             # without it: nothing changes ...
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False))
    d = s.describe()
    s.close(); model.free()
    assert "ignored without HPRLP_TEST_HOOKS=1: HPRLP_BATCH_LAMBDA=" + small in d, d   # ... and a solver of the process says so
