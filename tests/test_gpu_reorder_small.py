"""GPU: the locality ordering INSIDE a Solver at a small shape (HPRLP_REORDER_ANYWAY, csrc/solver.cpp: try_reorder) -- every
gather and scatter of the permutation at the solver's boundary, by value.

The LP is evalcases.all_bounds_lp on a permuted band of 20 011 x 26 003 (every bound kind, -0.0 and l = u cross the permutation).
Three checks:
  * the solver's ordering() is what the step entry's device path gives for the same pattern and hooks;
  * the BIT TWIN: a second solver on the explicitly permuted LP (tests/reorderref.py: permuted_csr, the vectors gathered by
    ordering()) with the same form hooks and HPRLP_NO_REORDER=1.  Both solvers' kernels see identical device arrays, so everything
    read back from the reordered solver in the caller's numbering must equal the twin's, mapped back by the permutation, bit for
    bit: no tolerance;
  * the oracle on the LP as given, at the tolerances of tests/test_gpu_reorder.py: test_reordered_iterates_match_oracle -- so the
    twin test cannot pass on two equally wrong sides.
The power iteration is the known exception to the twin: its start vector is defined in the caller's numbering (solver.cpp,
power_start: zp[i] = z0[perm_r[i]]), so lambda is compared with the oracle on the LP as given, and the start vector is read back."""
import contextlib
import os

import numpy as np
import pytest
from scipy import sparse

import bench_helpers as bh
import evalcases
import reorderref as R
from conftest import hprlp, lpgen
from oracle import oracle as O
from test_gpu_detect import model_of
from test_gpu_kernels import NAMES_M, NAMES_N, run_steps

pytestmark = pytest.mark.gpu

M, N = 20011, 26003
FORM = {"HPRLP_NO_SMALL": "1", "HPRLP_TILED_MIN_ROWS": "1", "HPRLP_TILED_MIN_DENSE": "0.0", "HPRLP_TILE_PIECES": "0",
        "HPRLP_DEVICE_TRANSPOSE_MIN": "1000", "HPRLP_REORDER_CLUSTER": "64"}
STREAM = dict(FORM, HPRLP_TILED_MIN_DENSE="1.01")        # the staged-tile form always declines: the stream kernel on P A Q
ANYWAY, GIVEN = {"HPRLP_REORDER_ANYWAY": "1"}, {"HPRLP_NO_REORDER": "1"}
CLEAR = ("HPRLP_NO_TILED", "HPRLP_NO_REORDER", "HPRLP_REORDER_ANYWAY", "HPRLP_TILED_MIN_COLS", "HPRLP_PIECES_ANYWAY", "HPRLP_TILE_ROWS",
         "HPRLP_TILE_COLS", "HPRLP_REORDER_HOST", "HPRLP_REORDER_SWEEPS", "HPRLP_REORDER_TRIM")
DATA = ("AL", "AU", "l", "u", "c", "row_norm", "col_norm")
ROWS = set(NAMES_M) | {"AL", "AU", "row_norm", "ray_y", "ray_prev_y"}
RAYS = ("ray_d", "ray_prev_x", "ray_y", "ray_prev_y")


@contextlib.contextmanager
def hooks(*sets):
    env = {k: v for s in sets for k, v in s.items()}
    old = {k: os.environ.get(k) for k in set(env) | set(CLEAR)}
    for k in CLEAR:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def band_matrix():
    r, c = R.permuted_band(M, N, 8, 31, bh.gen_banded)
    rng = np.random.default_rng(32)
    A = sparse.csr_matrix((rng.uniform(0.5, 1.5, size=len(r)) * rng.choice([-1.0, 1.0], size=len(r)), (r, c)), shape=(M, N))
    A.sum_duplicates()
    A.sort_indices()
    return A


_lps = {}


def the_lp(kind="feasible"):
    """Built once per process; callers leave it unchanged."""
    if kind not in _lps:
        A = band_matrix()
        if kind == "feasible":
            _lps[kind] = evalcases.all_bounds_lp(A, 33)
        else:
            lp = lpgen.planted_infeasible_lp(M, N, 0, 34, A=A)
            for k in ("rowptr", "colind"):
                lp[k] = np.asarray(lp[k], np.int32)
            _lps[kind] = lp
    return _lps[kind]


def twin_of(lp, pr, pc):
    """The explicitly permuted LP (the reference's permuted copy, the vectors gathered) and the source entry of each of its entries."""
    rp, ci, v, src = R.permuted_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], pr, pc)
    return dict(m=lp["m"], n=lp["n"], rowptr=rp, colind=ci, values=np.ascontiguousarray(v), AL=lp["AL"][pr], AU=lp["AU"][pr],
                l=lp["l"][pc], u=lp["u"][pc], c=lp["c"][pc]), src


class Pair:
    """The reordered solver s on the LP as given and its twin t on the explicitly permuted LP."""

    def __init__(self, lp, form=FORM, **params):
        self.lp, self.form = lp, form
        self.prm = hprlp.Parameters(use_presolve=False, **params)
        self.model = model_of(lp)
        with hooks(form, ANYWAY):
            self.s = hprlp.Solver(self.model, self.prm)
        self.pr, self.pc = self.s.ordering()
        self.tlp, self.src = twin_of(lp, self.pr, self.pc)
        self.tmodel = model_of(self.tlp)
        with hooks(form, GIVEN):
            self.t = hprlp.Solver(self.tmodel, self.prm)
        assert self.t.ordering() is None

    def back(self, name, v):
        """A vector of the twin in the caller's numbering."""
        out = np.empty_like(v)
        out[self.pr if name in ROWS else self.pc] = v
        return out

    def same(self, names, where):
        for name in names:
            a, b = self.s.get(name), self.back(name, self.t.get(name))
            assert bits_equal(a, b), (where, name, int((a.view(np.int64) != b.view(np.int64)).sum()), float(np.nanmax(np.abs(a - b))))

    def both(self, f):
        return f(self.s), f(self.t)

    def close(self):
        self.s.close(); self.t.close(); self.model.free(); self.tmodel.free()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def forms_of(d):
    """describe() without the ordering note and the switches: the kernel forms and their geometry."""
    return d.split("; locality ordering applied")[0].split("; switches:")[0]


def assert_forms(p, tiled):
    ds, dt = p.s.describe(), p.t.describe()
    info = p.s.info()
    assert "locality ordering applied" in ds and info["reordered"] and info["tiled"] == tiled, ds
    assert "HPRLP_REORDER_ANYWAY=1" in ds.split("switches:")[1] and "HPRLP_NO_REORDER=1" in dt.split("switches:")[1]
    assert not p.t.info()["reordered"] and p.t.info()["tiled"] == tiled, dt
    assert forms_of(ds) == forms_of(dt), (ds, dt)
    if tiled == 3:
        assert ds.count("tiled, fused (k_tiled_fused") == 2, ds
    else:
        assert ds.count("stream kernel (k_spmv_fused") == 2, ds
    return ds


@pytest.mark.parametrize("form,tiled", [(FORM, 3), (STREAM, 0)], ids=["tiled", "stream"])
def test_ordering_is_the_step_entrys_and_the_forms_are_the_twins(gpu, form, tiled):
    """ "locality ordering applied", info()["reordered"], tiled == 3 (second case: the stream kernel on P A Q); the permutations
    are the step entry's device permutations for the same pattern and hooks; the twin runs the same forms on the same geometry.
    Without HPRLP_TEST_HOOKS the hook is ignored and reported, and without the hook a small matrix is not reordered."""
    lp = the_lp()
    p = Pair(lp, form)
    assert_forms(p, tiled)
    with hooks(form):
        st = hprlp.reorder_steps(M, N, lp["rowptr"], lp["colind"], device=True, sweeps=3)
        plain = hprlp.Solver(p.model, p.prm)
    assert np.array_equal(p.pr, st["row_new2old"]) and np.array_equal(p.pc, st["col_new2old"])
    assert st["clusters"] == R.cluster_count(M, N, 64) > 500 and st["share_before"] == 1.0     # (the gate the hook skips)
    assert plain.ordering() is None and "locality ordering" not in plain.describe()
    plain.close()
    # the clustering on the host (HPRLP_REORDER_HOST=1, try_reorder's other branch) gives the same permutations: the BFS is over
    # within the host's 12 synchronous levels
    assert st["bfs_levels"] <= R.HOST_LEVELS
    with hooks(form, ANYWAY, {"HPRLP_REORDER_HOST": "1"}):
        hs = hprlp.Solver(p.model, p.prm)
    oh = hs.ordering()
    assert oh is not None and np.array_equal(oh[0], p.pr) and np.array_equal(oh[1], p.pc)
    hs.close()
    with hooks(form, ANYWAY, {"HPRLP_TEST_HOOKS": "0"}):
        off = hprlp.Solver(p.model, p.prm)
    d = off.describe()
    assert off.ordering() is None and "HPRLP_REORDER_ANYWAY=1" in d.split("ignored without HPRLP_TEST_HOOKS=1:")[1], d
    off.close()
    # the value maps are the host rule's for this ordering
    mapA, mapAT = p.s.value_maps()
    hA, hAT = hprlp.value_maps_host(M, N, lp["rowptr"], lp["colind"], p.pr, p.pc)
    assert np.array_equal(mapA, hA) and np.array_equal(mapAT, hAT) and np.array_equal(mapA, p.src)
    p.close()


@pytest.mark.parametrize("form,tiled", [(FORM, 3), (STREAM, 0)], ids=["tiled", "stream"])
def test_bit_twin_scaling_iterates_evaluation_and_rays(gpu, form, tiled):
    """Curtis-Reid on.  Equal bits: the seven data vectors and A_val / AT_val after scale(); the eleven state vectors after
    iterate(17, True), iterate(5, False), a restart and iterate(9, True); residuals and weighted_norm(); the nine ray-test scalars
    and the four ray vectors."""
    p = Pair(the_lp(), form)
    assert_forms(p, tiled)
    p.both(lambda s: s.scale())
    p.same(DATA, "after scale()")
    for name in ("A_val", "AT_val"):          # (device order on both sides: P A Q and its transpose)
        a, b = p.both(lambda s: s.get(name))
        assert bits_equal(a, b) and np.abs(a).min() > 0, name
    sc = p.both(lambda s: s.scalars())
    for k in ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org"):
        assert sc[0][k] == sc[1][k], k
    sigma, lam = 0.6, 1.4
    p.both(lambda s: s.init(sigma, lam))
    p.both(lambda s: s.iterate(17, True))
    p.same(NAMES_N + NAMES_M, "after 17 + check")
    ra, rb = p.both(lambda s: s.residuals(18, True))
    assert all(bits_equal(ra[k], rb[k]) for k in ra), (ra, rb)
    assert np.isfinite(ra["weighted_norm"]) and ra["err_Rp"] > 0 and ra["err_Rd"] > 0
    wa, wb = p.both(lambda s: s.weighted_norm())
    assert wa == wb == ra["weighted_norm"]
    p.both(lambda s: s.iterate(5, False))
    p.same(NAMES_N + NAMES_M, "after 5 more")
    na, nb = p.both(lambda s: s.restart(current_gap=0.3, best_gap=0.3, best_sigma=0.8, err_Rd=1e-2, err_Rp=1e-2, rel_gap=1e-2))
    assert na == nb
    p.same(NAMES_N + NAMES_M, "after the restart")
    p.both(lambda s: s.iterate(9, True))
    p.same(NAMES_N + NAMES_M, "after the restart and 9 + check")
    assert np.abs(p.s.get("x")).max() > 0 and np.abs(p.s.get("y")).max() > 0
    # the ray test: store, move on, test
    assert p.both(lambda s: s.ray_step(restart=True)) == (None, None)
    p.same(RAYS[1::2], "stored iterate")
    p.both(lambda s: s.iterate(6, True))
    qa, qb = p.both(lambda s: s.ray_step())
    assert qa is not None and set(qa) == set(qb) and all(bits_equal(qa[k], qb[k]) for k in qa), (qa, qb)
    assert qa["YN"] > 0 and qa["DN"] > 0
    p.same(RAYS, "ray vectors")
    p.close()


def _same_results(p, ra, rb, where):
    assert ra.status == rb.status and ra.iter == rb.iter, (where, ra.status, ra.iter, rb.status, rb.iter)
    assert len(ra.trace) == len(rb.trace) > 0
    for a, b in zip(ra.trace, rb.trace):
        assert a["iter"] == b["iter"] and a["restart_flag"] == b["restart_flag"]
        for k in a:
            assert bits_equal(a[k], b[k]), (where, a["iter"], k, a[k], b[k])
    for f in ("x", "y", "z"):
        a, b = getattr(ra, f), p.back("y" if f == "y" else "x", getattr(rb, f))
        assert bits_equal(a, b), (where, f, int((a != b).sum()))
    assert bits_equal(ra.primal_obj, rb.primal_obj) and bits_equal(ra.residuals, rb.residuals) and bits_equal(ra.gap, rb.gap)


def test_bit_twin_run_warm_start_new_data_and_new_matrix(gpu):
    """run() from init(-1, lam): status, iteration count, trace, x, y, z (unpermute of the results); a warm start through
    set_start (start_apply's gather); set_data + resolve (k_data_in); set_matrix with new values: A_val, AT_val through the value
    maps, the maps against value_maps_host."""
    lp = the_lp()
    p = Pair(lp, FORM, stop_tol=1e-4, max_iter=2500)
    assert_forms(p, 3)
    p.both(lambda s: s.scale())
    lam = 1.01 * p.s.power_iteration()[0]
    p.both(lambda s: s.init(-1.0, lam))
    ra, rb = p.both(lambda s: s.run())
    _same_results(p, ra, rb, "run")
    assert ra.iter > 100
    # warm start: the caller's x0 / y0, gathered for the twin
    rng = np.random.default_rng(35)
    x0 = lp["x_star"] + 0.01 * rng.normal(size=N)
    y0 = lp["y_star"] + 0.01 * rng.normal(size=M)
    p.both(lambda s: (s.reset(), s.init(-1.0, lam)))
    p.s.set_start(x0, y0)
    p.t.set_start(x0[p.pc], y0[p.pr])
    p.same(("x", "x_bar", "y", "y_bar"), "start_apply")
    wa, wb = p.both(lambda s: s.run())
    _same_results(p, wa, wb, "warm run")
    assert wa.iter != ra.iter or not np.array_equal(wa.x, ra.x)
    # new data: c and all four bounds
    c2 = lp["c"] + 0.05 * rng.normal(size=N)
    AL2, AU2 = lp["AL"] - 0.1, lp["AU"] + 0.2
    l2, u2 = lp["l"] - 0.05, lp["u"] + 0.05
    p.s.set_data(c=c2, AL=AL2, AU=AU2, l=l2, u=u2)
    p.t.set_data(c=c2[p.pc], AL=AL2[p.pr], AU=AU2[p.pr], l=l2[p.pc], u=u2[p.pc])
    p.same(DATA, "set_data")
    da, db = p.s.resolve(), p.t.resolve()
    _same_results(p, da, db, "resolve")
    xa, xb = p.s.resolve(x=x0, y=y0), p.t.resolve(x=x0[p.pc], y=y0[p.pr])
    _same_results(p, xa, xb, "resolve from a point")
    # new matrix values on the pattern
    v2 = lp["values"] * rng.uniform(0.5, 2.0, size=len(lp["values"]))
    p.s.set_matrix(v2, lp["c"], lp["AL"], lp["AU"], lp["l"], lp["u"])
    p.t.set_matrix(v2[p.src], lp["c"][p.pc], lp["AL"][p.pr], lp["AU"][p.pr], lp["l"][p.pc], lp["u"][p.pc])
    for name in ("A_val", "AT_val"):
        a, b = p.both(lambda s: s.get(name))
        assert bits_equal(a, b), name
    p.same(DATA, "set_matrix")
    mapA, mapAT = p.s.value_maps()
    hA, hAT = hprlp.value_maps_host(M, N, lp["rowptr"], lp["colind"], p.pr, p.pc)
    assert np.array_equal(mapA, hA) and np.array_equal(mapAT, hAT)
    # ... and by value: unscaled, entry e of the solver's A is the caller's entry mapA[e]
    fresh = Pair(dict(lp, values=v2), FORM, stop_tol=1e-4, max_iter=2500)
    fresh.s.scale()
    assert bits_equal(fresh.s.get("A_val"), p.s.get("A_val")) and bits_equal(fresh.s.get("AT_val"), p.s.get("AT_val"))
    fresh.close()
    p.close()


def test_bit_twin_certificate_of_a_planted_infeasible_lp(gpu):
    """unpermute of a certificate: y, z of the Farkas ray in the caller's numbering equal the twin's, mapped back."""
    lp = the_lp("infeasible")
    p = Pair(lp, FORM, max_iter=50000)
    assert_forms(p, 3)
    p.both(lambda s: s.set_detection())
    p.both(lambda s: s.scale())
    lam = 1.01 * p.s.power_iteration()[0]
    p.both(lambda s: s.init(-1.0, lam))
    ra, rb = p.both(lambda s: s.run(max_trace=1))
    ka, kb = p.both(lambda s: s.certificate())
    assert ra.status == rb.status == "PRIMAL_INFEASIBLE" and ra.iter == rb.iter and ka.kind == kb.kind == 1 and ka.iter == kb.iter
    assert ka.d is None and kb.d is None
    assert bits_equal(ka.y, p.back("y", kb.y)) and bits_equal(ka.z, p.back("x", kb.z))
    assert bits_equal(ka.objective, kb.objective) and bits_equal(ka.violation, kb.violation)
    # the ray is one of the LP as given: D(y) > 0 (lpgen.farkas_terms on the caller's bounds), z = -A'y
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(M, N))
    assert abs(np.abs(ka.y).max() - 1.0) <= 1e-12
    np.testing.assert_allclose(ka.z, -(A.T @ ka.y), rtol=1e-9, atol=1e-9)
    p.close()


def test_unbounded_ray_of_the_twin(gpu):
    """The d of a dual-infeasible certificate crosses the column permutation."""
    A = band_matrix()
    lp = lpgen.planted_unbounded_lp(M, N, 0, 36, A=A)
    for k in ("rowptr", "colind"):
        lp[k] = np.asarray(lp[k], np.int32)
    p = Pair(lp, FORM, max_iter=50000)
    p.both(lambda s: s.set_detection())
    p.both(lambda s: s.scale())
    lam = 1.01 * p.s.power_iteration()[0]
    p.both(lambda s: s.init(-1.0, lam))
    ra, rb = p.both(lambda s: s.run(max_trace=1))
    ka, kb = p.both(lambda s: s.certificate())
    assert ra.status == rb.status == "DUAL_INFEASIBLE" and ra.iter == rb.iter and ka.kind == kb.kind == 2
    assert ka.y is None and bits_equal(ka.d, p.back("x", kb.d))
    p.close()


def test_power_iteration_and_iterates_against_the_oracle_on_the_lp_as_given(gpu):
    """The oracle works on the LP exactly as given.  Data at rtol 1e-12 and iterates at rtol 1e-11 / atol 1e-12 (the figures of
    test_reordered_iterates_match_oracle, Curtis-Reid off as there); lambda and the iteration count of the power iteration at
    1e-11 (tests/test_gpu_tiled.py); the start vector, read back, is the oracle's in the caller's numbering -- the twin's is the
    same numbers at other rows, which is why the power iteration is no bit twin."""
    lp = the_lp()
    p = Pair(lp, FORM, use_CR_scaling=False)
    assert_forms(p, 3)
    ref = O.ScaledLP(M, N, lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                     O.Params.default(use_CR_scaling=0))
    p.both(lambda s: s.scale())
    for name, want in (("AL", ref.AL), ("AU", ref.AU), ("l", ref.l), ("u", ref.u), ("c", ref.c), ("row_norm", ref.row_norm),
                       ("col_norm", ref.col_norm)):
        got = p.s.get(name)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), name
        assert np.array_equal(np.signbit(got), np.signbit(want)), name            # (-0.0 stays -0.0 across the permutation)
        np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, err_msg=name)
    z0 = O.power_start_vector(M)
    assert np.array_equal(p.s.power_start(), z0)
    assert np.array_equal(p.t.power_start(), z0) and not np.array_equal(p.back("y", p.t.power_start()), z0)
    lam, it = p.s.power_iteration()
    lam_ref, it_ref = ref.power_iteration()
    assert it == it_ref and abs(lam - lam_ref) <= 1e-11 * lam_ref, (it, it_ref, lam, lam_ref)
    st = run_steps(p.s, ref, 0.6, 1.4, [(17, True), (5, True), (9, False)])
    for name in NAMES_N + NAMES_M:
        np.testing.assert_allclose(p.s.get(name), st[name], rtol=1e-11, atol=1e-12, err_msg=name)
    p.close()
