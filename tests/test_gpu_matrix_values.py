"""New matrix values for a resident solver on the GPU (hprlp_solver_set_matrix_values / hprlp_batched_solver_set_matrix_values,
DESIGN.md "Matrix values"), everything through the C ABI via hprlp.py.  The reference of every bit-for-bit check is a FRESH
solver on the changed model: after set_matrix() the resident solver holds the same scaled matrix, factors, vectors, scalars and
lambda_max, runs the same iterations, and says the same in describe().  Then the CPU oracle, the composition with set_data and
the infeasibility detection, the refusals, the seconds, and the resident batched solver."""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen
from oracle import oracle as O
from fuzz_parity import fork_verdict
from test_gpu_detect import BASE_ENV, FORM_ENV, check_certificate, model_of
from test_gpu_resolve import TOL, close, params, prepared, same_bits, same_run, six, snapshot, VECS, B_SIDE, C_SIDE
from test_matrix_values import KINDS, changed_matrix
from test_resolve import SEEDS, base_lp, changed

pytestmark = pytest.mark.gpu
STATE = ("A_val", "AT_val", "row_norm", "col_norm")
# iterations to OPTIMAL at 1e-6 of a fresh solve of the changed LP on the CPU oracle alone (its own power iteration), computed
# before any GPU run: changed_matrix(base_lp(seed), kind, 100 + seed)
ORACLE_ITERS = {("rel1e-3", 11): 1200, ("rows", 11): 2000, ("rel1e-3", 12): 900, ("rows", 12): 1700,
                ("rel1e-3", 13): 9900, ("rows", 13): 3400, ("rel1e-3", 14): 700, ("rows", 14): 1600}


def mat(lp):
    return dict(values=lp["values"], c=lp["c"], AL=lp["AL"], AU=lp["AU"], l=lp["l"], u=lp["u"])


def full_state(s):
    d = snapshot(s)
    d.update({k: s.get(k) for k in STATE})
    return d


ALL = VECS + B_SIDE + C_SIDE + STATE


def check_maps(s, lp):
    """value_maps() of the solver against the host restatement on the solver's own ordering."""
    order = s.ordering()
    pr, pc = order if order is not None else (None, None)
    a, t = s.value_maps()
    wa, wt = hprlp.value_maps_host(lp["m"], lp["n"], lp["rowptr"], lp["colind"], pr, pc)
    assert np.array_equal(a, wa) and np.array_equal(t, wt)
    return order is not None


# ---- 1. the state against a fresh solver, on every kernel form -----------------------------------------------------------------
FORM_SCRIPT = r'''
import os, sys
import numpy as np
from scipy import sparse
sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import hprlp, lpgen
from test_gpu_detect import model_of
from test_resolve import base_lp
from test_matrix_values import KINDS, changed_matrix
import test_gpu_matrix_values as T
import test_gpu_resolve as R
form, solves = sys.argv[1], sys.argv[2] == "solves"
def planted_on(A, seed):
    A = sparse.csr_matrix(A); A.sum_duplicates(); A.sort_indices()
    lp = lpgen._plant(np.random.default_rng(seed), A)
    lp.update(m=A.shape[0], n=A.shape[1], A=A, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy())
    return lp
def permuted_banded(m, n, per_row, band):
    rp, ci, v = lpgen.banded_csr(m, n, per_row, band, 5)
    A = sparse.csr_matrix((v, ci, rp), shape=(m, n)); A.sum_duplicates()
    rng = np.random.default_rng(8)
    pr, pc = rng.permutation(m), rng.permutation(n)
    inv = np.empty(n, np.int64); inv[pc] = np.arange(n)
    B = A[pr]; return sparse.csr_matrix((B.data, inv[B.indices], B.indptr), shape=(m, n))
if form in ("small", "stream"):
    lps = [base_lp(s) for s in (11, 12)]
elif form == "all-remainder":
    lps = [lpgen.planted_lp(3000, 4000, 18000, 31, values="network")]
elif form == "reordered":   # the 1.6 M shape of tests/test_gpu_resolve.py (see the test's docstring)
    lps = [planted_on(permuted_banded(1_600_000, 1_600_000, 10, 16000), 32)]
else:   # tiled forms: a banded matrix
    rp, ci, v = lpgen.banded_csr(8000, 10000, 8, 1500, 6)
    lps = [planted_on(sparse.csr_matrix((v, ci, rp), shape=(8000, 10000)), 33)]
expect = {"small": "single-workgroup kernel", "stream": "A: stream kernel", "tiled": "tiled, fused (k_tiled_fused",
          "pieces": "tiled, piece form", "all-remainder": "all-remainder form (k_pb_fused", "reordered": "locality ordering applied"}[form]
switches = [{}]
if form in ("small", "stream") and not solves:   # each scaling switch off in turn (all on: the default)
    switches += [{k: False} for k in ("use_CR_scaling", "use_Ruiz_scaling", "use_Pock_Chambolle_scaling", "use_bc_scaling")]
for lp in lps:
    for sw in switches:
        prm = hprlp.Parameters(use_presolve=False, stop_tol=1e-4, max_iter=3000, **sw)
        S = hprlp.Solver(model_of(lp), prm)
        hprlp.lib().hprlp_solver_set_verbose(S.h, 0)
        d = S.describe()
        assert expect in d, d
        info = S.info()
        if solves:
            S.prepare()
            r0 = S.run()
        else:
            S.scale()
        for i, kind in enumerate(KINDS):   # S goes from one changed model to the next; F is fresh on each
            lp2 = changed_matrix(lp, kind, 40 + i)
            lam, its = S.set_matrix(**T.mat(lp2))
            F = hprlp.Solver(model_of(lp2), prm)
            hprlp.lib().hprlp_solver_set_verbose(F.h, 0)
            F.scale()
            bad = R.same_bits(T.full_state(S), T.full_state(F), T.ALL)
            assert not bad, (form, sw, kind, bad)
            lamF, itsF = F.power_iteration()
            assert (lam, its) == (lamF, itsF), (form, sw, kind, lam, its, lamF, itsF)
            assert S.describe() == d == F.describe(), (S.describe(), d, F.describe())
            assert S.info() == info
            reordered = T.check_maps(S, lp)
            assert reordered == (form == "reordered")
            if solves:
                F.init(-1.0, 1.01 * lamF)
                rs, rf = S.resolve(), F.run()
                bad = R.same_run(rs, rf)
                assert not bad, (form, kind, bad[:3])
                print(form, kind, "whole solve", rs.status, rs.iter)
            R.close(F)
        R.close(S)
print("OK", form)
''' % ROOT

def run_script(script, args, env, timeout=600):
    r = subprocess.run([sys.executable, "-c", script] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0 or "OK" not in r.stdout:
        pytest.fail("%s: exit %d\n%s\n%s" % (args, r.returncode, r.stdout[-1500:], r.stderr[-2500:]), pytrace=False)
    print("\n".join(r.stdout.strip().splitlines()[-6:]))


@pytest.mark.parametrize("form", list(FORM_ENV))
def test_state_after_set_matrix_is_a_fresh_solvers(gpu, form):
    """A_val, AT_val, row_norm, col_norm, the five vectors, the six scalars, lambda and the power iteration's count, describe() and
    info(), and the device's value maps against the host restatement.  small / stream / tiled / pieces take the host transpose, the
    all-remainder form the device transpose, `reordered` the device transpose under a locality ordering.  The reordered shape is
    the existing 1.6 M one (randomly permuted banded 1 600 000 x 1 600 000, 10 per row, band 16 000): on the issue's small shape --
    60 000 x 60 000, 10 per row, band 2000, HPRLP_DEVICE_TRANSPOSE_MIN=1000, HPRLP_TILED_MIN_ROWS=1 -- the tiled build accepts the
    permuted matrix as it is (8 super-blocks, every entry in a staged tile), so no ordering is looked for and describe() does not
    say "locality ordering applied"."""
    env = dict(os.environ, **BASE_ENV, **FORM_ENV[form])
    run_script(FORM_SCRIPT, [form, "state"], env)


def test_whole_solves_on_the_tiled_form(gpu):
    """Check 1's tiled case with whole solves: the resident solver ran the base LP first, then every changed model against a fresh
    solver's run, status, iteration count, trace and solution bit for bit (at 1e-4, at most 3000 iterations)."""
    run_script(FORM_SCRIPT, ["tiled", "solves"], dict(os.environ, **BASE_ENV, **FORM_ENV["tiled"]))


# ---- 2. history independence, whole solves ---------------------------------------------------------------------------------------
HISTORY_SCRIPT = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import hprlp
from test_resolve import base_lp
from test_matrix_values import changed_matrix
import test_gpu_matrix_values as T
import test_gpu_resolve as R
form, first = sys.argv[1], sys.argv[2]
expect = {"small": "single-workgroup kernel", "stream": "A: stream kernel"}[form]
for seed in (11, 12):
    lp = base_lp(seed)
    lp2, lp3 = changed_matrix(lp, "rel1e-3", 100 + seed), changed_matrix(lp, "rows", 100 + seed)
    prm = R.params()
    S = R.prepared(lp, prm)
    assert expect in S.describe(), S.describe()
    if first == "detect+warm":   # S's first run with detection on and a start
        S.set_detection(1e-8, 1e-8)
        rng = np.random.default_rng(3)
        S.set_start(lp["x_star"] + rng.normal(scale=0.1, size=lp["n"]), lp["y_star"] + rng.normal(scale=0.1, size=lp["m"]))
    r0 = S.run()
    assert r0.status == "OPTIMAL", r0.status
    if first == "detect+warm":
        S.set_detection(on=False)
    for chain in ((lp2,), (lp2, lp3)):   # S: base -> ... -> target; G: the target directly
        for step in chain:
            S.set_matrix(**T.mat(step))
            rs = S.resolve()
        target = chain[-1]
        G = R.prepared(target, prm)
        assert not R.same_bits(T.full_state(S), T.full_state(G), T.ALL)
        rg = G.resolve()
        assert rs.status == "OPTIMAL", rs.status
        bad = R.same_run(rs, rg)
        assert not bad, (seed, len(chain), bad[:3])
        ws, wg = S.resolve(r0.x, r0.y), G.resolve(r0.x, r0.y)
        bad = R.same_run(ws, wg)
        assert not bad, ("warm", seed, len(chain), bad[:3])
        print("seed", seed, "chain", len(chain), "cold iterations", rs.iter, "warm from the base optimum", ws.iter, ws.status)
        R.close(G)
    R.close(S)
print("OK", form, first)
''' % ROOT


@pytest.mark.parametrize("form,graph,first", [("small", True, "plain"), ("small", True, "detect+warm"), ("stream", True, "plain"),
                                              ("stream", False, "plain"), ("stream", True, "detect+warm")])
def test_resolve_after_set_matrix_does_not_depend_on_the_history(gpu, form, graph, first):
    """S ran the base LP to OPTIMAL (plain, or with detection and a warm start on), then got the changed matrix -- and a second one in
    the chained case; G was prepared on the target and never ran anything else.  Cold and warm re-solves agree in every bit.  The
    cold and warm iteration counts are printed; nothing is asserted about their ratio."""
    env = dict(os.environ, **BASE_ENV, **FORM_ENV[form])
    if not graph:
        env["HPRLP_NO_GRAPH"] = "1"
    run_script(HISTORY_SCRIPT, [form, first], env)


# ---- 3. against the CPU oracle ------------------------------------------------------------------------------------------------------
def oracle_solve(lp, lam):
    return O.solve(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                   params=O.Params.default(stop_tol=TOL, max_iter=500000), lambda_override=lam, max_trace=8192)


def test_resolve_after_set_matrix_against_the_oracle(gpu):
    """Eight changed LPs: OPTIMAL on both sides, the objective within 2 tol (1 + 2 |obj|) of the oracle's, the oracle's iteration
    count -- or a fork by tests/fuzz_parity.py's rule, for at most two of the eight.  The oracle gets the solver's lambda."""
    forks, lines = [], []
    for seed in SEEDS:
        lp = base_lp(seed)
        S = prepared(lp, params())
        assert S.run().status == "OPTIMAL"
        for kind in ("rel1e-3", "rows"):
            lp2 = changed_matrix(lp, kind, 100 + seed)
            S.set_matrix(**mat(lp2))
            lam = S.scalars()["lambda_max"]
            r = S.resolve(max_trace=8192)
            assert S.scalars()["lambda_max"] == lam   # (no bump: the oracle runs on the same lambda)
            ref = oracle_solve(lp2, lam)
            lines.append((seed, kind, r.status, r.iter, ref["status"], ref["iter"], r.primal_obj, ref["primal_obj"]))
            print(*lines[-1])
            assert ref["status"] == "OPTIMAL" and ref["iter"] == ORACLE_ITERS[(kind, seed)], lines[-1]
            assert r.status == "OPTIMAL", lines[-1]
            assert abs(r.primal_obj - ref["primal_obj"]) <= 2 * TOL * (1 + 2 * abs(ref["primal_obj"])), lines[-1]
            if r.iter != ref["iter"]:
                ok, why, info = fork_verdict(r.trace, ref["trace"], TOL)
                print("  fork?", ok, why)
                assert ok, (lines[-1], why, info)
                forks.append((seed, kind, why))
        close(S)
    assert len(lines) == 8
    assert len(forks) <= 2, forks


# ---- 4. composition ------------------------------------------------------------------------------------------------------------------
def test_set_matrix_then_set_data_equals_a_fresh_solver_with_the_same_set_data(gpu):
    lp = base_lp(12)
    lp2 = changed_matrix(lp, "rows", 112)
    data = changed(lp2, "c1e-3")
    S = prepared(lp, params())
    assert S.run().status == "OPTIMAL"
    S.set_matrix(**mat(lp2))
    S.set_data(**six(data))
    rs = S.resolve()
    G = prepared(lp2, params())
    G.set_data(**six(data))
    rg = G.resolve()
    assert not same_bits(full_state(S), full_state(G), ALL)
    assert not same_run(rs, rg) and rs.status == "OPTIMAL"
    close(S, G)


def test_detection_across_a_change_of_the_matrix_and_back(gpu):
    """The changed model is primal infeasible: lpgen.planted_infeasible_lp (the construction of tests/test_gpu_detect.py) on the
    changed matrix.  Verdict and certificate bits equal a fresh solver's, the certificate passes the numpy ratio test; back on the
    base values the first optimum returns."""
    lp = base_lp(11)
    A2 = changed_matrix(lp, "rel1e-3", 111)["A"]
    bad = lpgen.planted_infeasible_lp(lp["m"], lp["n"], 0, 21, A=A2)
    assert np.array_equal(bad["rowptr"], lp["rowptr"]) and np.array_equal(bad["colind"], lp["colind"])
    prm = params(max_iter=100000)
    S = prepared(lp, prm)
    S.set_detection(1e-8, 1e-8)
    r0 = S.run()
    assert r0.status == "OPTIMAL"
    S.set_matrix(**mat(bad))
    r = S.resolve()
    ks = S.certificate()
    G = prepared(bad, prm)
    G.set_detection(1e-8, 1e-8)
    rg = G.resolve()
    kg = G.certificate()
    print("infeasible on the changed matrix:", r.status, r.iter, "certificate kind", ks.kind, "iteration", ks.iter)
    assert (r.status, r.iter) == (rg.status, rg.iter) and (ks.kind, ks.iter) == (kg.kind, kg.iter)
    for f in ("y", "z", "d"):
        a, b = getattr(ks, f), getattr(kg, f)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f
    assert not same_run(r, rg)
    r.certificate = ks
    check_certificate(bad, r, "PRIMAL_INFEASIBLE")
    S.set_matrix(**mat(lp))
    back = S.resolve()
    assert back.status == "OPTIMAL" and S.certificate().kind == 0
    assert abs(back.primal_obj - r0.primal_obj) <= 2 * TOL * (1 + 2 * abs(r0.primal_obj)), (back.primal_obj, r0.primal_obj)
    close(S, G)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_everything_bit_for_bit(gpu):
    lp = base_lp(11)
    lp2 = changed_matrix(lp, "rows", 111)
    S = hprlp.Solver(model_of(lp), params())
    L = hprlp.lib()
    p = lambda a: a.ctypes.data_as(hprlp.c_dbl_p)
    good = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in mat(lp2).items()}

    def raw(nnz=None, **kw):   # the C call itself, past the wrapper's length checks
        a = dict(good, **kw)
        ptr = lambda k: None if a[k] is None else p(a[k])
        return L.hprlp_solver_set_matrix_values(S.h, ptr("values"), len(good["values"]) if nnz is None else nnz, ptr("c"), None,
                                                ptr("AL"), ptr("AU"), ptr("l"), ptr("u"))

    assert raw() == -1 and "scale" in hprlp.last_error()   # never scaled
    S.prepare()
    before = full_state(S)
    nan_v, inf_v, nan_u = good["values"].copy(), good["values"].copy(), good["u"].copy()
    nan_v[-1], inf_v[-1], nan_u[-1] = np.nan, np.inf, np.nan
    for kw, word in ((dict(nnz=len(good["values"]) - 1), "nnz"), (dict(values=nan_v), "not finite"), (dict(values=inf_v), "not finite"),
                     (dict(u=nan_u), "NaN"), (dict(AL=None), "required"), (dict(values=None), "required")):
        assert raw(**kw) == -1, kw.keys()
        assert word in hprlp.last_error(), (kw.keys(), hprlp.last_error())
        assert not same_bits(before, full_state(S), ALL), kw.keys()
    assert raw(values=nan_v) == -1 and "val[%d]" % (len(nan_v) - 1) in hprlp.last_error()   # (the position of the bad value)
    with pytest.raises(ValueError, match="length"):
        S.set_matrix(**dict(mat(lp2), values=lp2["values"][:-1]))
    assert not same_bits(before, full_state(S), ALL)
    assert S.matrix_seconds()["calls"] == 0
    # a valid call after the refused ones: check 1's bits
    inf_side = dict(mat(lp2))   # (infinite sides and bounds are legal: lp2 has them)
    assert np.isinf(inf_side["AL"]).any() and np.isinf(inf_side["u"]).any()
    S.set_matrix(**inf_side)
    F = hprlp.Solver(model_of(lp2), params())
    F.scale()
    assert not same_bits(full_state(S), full_state(F), ALL)
    close(S, F)


def test_sharded_solvers_refuse_set_matrix(gpu):
    lp = lpgen.planted_lp(300, 400, 2000, 3)
    model = model_of(lp)
    group = hprlp.Solver.local_group(2)
    errs = [None, None]

    def refusal(s):
        try:
            s.set_matrix(**mat(lp))
        except RuntimeError as e:
            return str(e)
        return None

    def work(rank):   # thread ranks
        s = hprlp.Solver.create_local(model, params(), rank, 2, group)
        errs[rank] = refusal(s)
        s.close()

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    hprlp.Solver.free_local_group(group)
    assert all(e and "one GPU only" in e for e in errs), errs
    os.environ["HPRLP_DIST_TRANSPORT"] = "shm"   # a rank of the shared-memory transport, a world of one
    try:
        uid = hprlp.Solver.dist_unique_id(1)
    finally:
        os.environ.pop("HPRLP_DIST_TRANSPORT")
    s = hprlp.Solver.create_dist(model, params(), 0, 1, uid)
    e = refusal(s)
    s.close()
    assert e and "one GPU only" in e, e
    model.free()


# ---- 6. structure ----------------------------------------------------------------------------------------------------------------------
def test_set_matrix_pays_no_setup_again(gpu):
    lp = base_lp(13)
    lp2, lp3 = changed_matrix(lp, "rel1e-3", 113), changed_matrix(lp, "rows", 113)
    S = prepared(lp, params())
    S.run()
    before, info = S.scalars(), S.info()
    t0 = time.perf_counter()
    S.set_matrix(**mat(lp2))
    first = S.matrix_seconds()
    r = S.resolve()
    wall = time.perf_counter() - t0
    after = S.scalars()
    print("set_matrix seconds", first, "resolve time", r.time, "wall", wall)
    assert after["setup_time"] == before["setup_time"] and S.info() == info
    assert after["scaling_time"] != before["scaling_time"] and after["scaling_time"] == first["scale"]
    assert first["maps"] > 0 and first["calls"] == 1
    parts = ("maps", "upload", "kernels", "scale")
    assert sum(first[k] for k in parts) <= first["total"] * (1 + 1e-9) + 1e-9
    assert r.status == "OPTIMAL" and first["total"] <= r.time < first["total"] + wall
    S.set_matrix(**mat(lp3))
    second = S.matrix_seconds()
    assert second["maps"] == 0 and second["calls"] == 2 and second["total"] > 0
    assert sum(second[k] for k in parts) <= second["total"] * (1 + 1e-9) + 1e-9
    close(S)


# ---- 7. the resident batched solver ----------------------------------------------------------------------------------------------------
BATCH_PRM = dict(stop_tol=1e-6, max_iter=3000, use_presolve=False)
SCALARS = ("primal_obj", "residuals", "gap")


def assert_same_batch(got, ref, tag):
    assert got["status"] == ref["status"], (tag, got["status"], ref["status"])
    assert list(got["iter"]) == list(ref["iter"]), (tag, list(got["iter"]), list(ref["iter"]))
    for f in ("x", "y", "z") + SCALARS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(ref[f])), (tag, f)


def matrix_model(lp):
    z = np.zeros
    return hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], z(lp["m"]), z(lp["m"]), z(lp["n"]), z(lp["n"]),
                                z(lp["n"]))


@pytest.mark.parametrize("B", [5, 64])
def test_batched_handle_after_set_matrix_is_a_fresh_handle(gpu, B):
    """The handle is created on lp's matrix and solves a batch; after set_matrix(values2) a host-entry call under norm rule 0 and
    under norm rule 1 and a device-entry call each equal a fresh handle's on lp2's matrix, scalars() included; carry is refused
    right after set_matrix and legal after one solve; no panel is allocated anew; detection off / on / off behaves as on the fresh
    handle."""
    from test_gpu_warm import make_batch
    from test_gpu_batched_device import T as on_gpu, on_host
    lp = base_lp(12)
    lp2 = changed_matrix(lp, "rows", 112)
    prm = hprlp.Parameters(**BATCH_PRM)
    m1, m2 = matrix_model(lp), matrix_model(lp2)
    h = hprlp.BatchedSolver(m1, prm)
    first = h.solve(*make_batch(lp, B, 2))
    assert len(first["status"]) == B
    info = h.info()
    with pytest.raises(ValueError, match="length"):
        h.set_matrix(lp2["values"][:-1])
    bad = lp2["values"].copy(); bad[-1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        h.set_matrix(bad)
    assert_same_batch(h.solve(*make_batch(lp, B, 2)), first, "after a refused set_matrix")
    h.set_matrix(lp2["values"])
    args = make_batch(lp2, B, 3)
    with pytest.raises(RuntimeError, match="carry"):
        h.solve(*args, carry=True)
    f = hprlp.BatchedSolver(m2, prm)
    for rule in (0, 1):
        h.set_norms(rule); f.set_norms(rule)
        got, ref = h.solve(*args), f.solve(*args)
        assert_same_batch(got, ref, ("host entry, norm rule", rule))
        sa, sb = h.scalars(), f.scalars()
        assert all(np.array_equal(sa[k], sb[k]) for k in hprlp.BATCH_SCALARS), rule
    targs = [on_gpu(a) for a in args]
    got, ref = on_host(h.solve_tensors(*targs)), on_host(f.solve_tensors(*targs))
    assert_same_batch(got, ref, "device entry")
    sa, sb = h.scalars(), f.scalars()
    assert all(np.array_equal(sa[k], sb[k]) for k in hprlp.BATCH_SCALARS)
    assert_same_batch(h.solve(*args, carry=True), f.solve(*args, carry=True), "carry after one solve")
    assert h.info()["panel_allocations"] == info["panel_allocations"], (info, h.info())   # (no new panel for the new values)
    for step, on in enumerate((False, True, False)):
        eps = 1e-8 if on else None
        assert_same_batch(h.solve(*args, eps_primal=eps, eps_dual=eps), f.solve(*args, eps_primal=eps, eps_dual=eps), ("detection", step, on))
    after = h.info()
    assert after["panel_allocations"] == f.info()["panel_allocations"], (after, f.info())   # (the detection's own panels, once)
    assert after["solves"] == info["solves"] + 8 and h.seconds()["create_power"] > 0
    h.close(); f.close(); m1.free(); m2.free()
