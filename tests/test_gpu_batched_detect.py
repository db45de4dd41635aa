"""Infeasibility detection in solve_batched (include/hprlp_amd.h hprlp_solve_batched_detect, DESIGN.md "Batched detection") on the
GPU: per-member verdicts against HiGHS, certificates judged by the numpy restatement of the ratio tests in each member's units,
every panel form, the limits' precedence, and no perturbation of the feasible members.

Every certificate's objective and violation are also held BY VALUE, from both sides, to D and V resp. c'd and W of the returned
ray (tests/evalref.py: check_certificate_values, in the member's units; the solves run with use_CR_scaling off, whose device
`exp` rounds by more than one u), on the panel forms of test_mixed_batch_verdicts_and_certificates: B = 5 (one chunk of 8),
B = 64, and B = 70 with chunks of 8 and of 32.  The nine device scalars of the batched ray kernels (kb_ray_form, kb_ray_col,
kb_ray_row) themselves are checked by value, step by step and in every panel geometry, by
tests/test_gpu_batched_ray_values.py through hprlp_batched_solver_ray_step."""
import functools
import json
import os

import numpy as np
import pytest
from scipy import sparse

import evalref
from conftest import hprlp, lpgen
from test_detect import dual_ray_test, highs_status, primal_ray_test
from test_gpu_batched import make_batch

pytestmark = pytest.mark.gpu
INF = np.inf
EPS = 1e-8
HERE = os.path.dirname(os.path.abspath(__file__))
RESULT_FIELDS = ("x", "y", "z", "iter", "primal_obj", "residuals", "gap")
STATUS_OF_HIGHS = {0: "OPTIMAL", 2: "PRIMAL_INFEASIBLE", 3: "DUAL_INFEASIBLE"}


def _member_equal(a, b, k):
    for f in RESULT_FIELDS:
        va, vb = (a[f][:, k], b[f][:, k]) if a[f].ndim == 2 else (a[f][k], b[f][k])
        assert np.array_equal(va, vb), (f, k)
    assert a["status"][k] == b["status"][k]


def _check_certificate(lp, r, k):
    """Member k's verdict and certificate, in its units, by the numpy ratio tests (10 x eps, as tests/test_gpu_detect.py), and
    its objective and violation by value from both sides (tests/evalref.py: check_certificate_values; use_CR_scaling off)."""
    cert = r["certificates"]
    kind, st = int(cert["kind"][k]), r["status"][k]
    assert st == {1: "PRIMAL_INFEASIBLE", 2: "DUAL_INFEASIBLE"}[kind], (k, st, kind)
    assert cert["iter"][k] == r["iter"][k]
    if kind == 1:
        y, z = cert["y"][:, k], cert["z"][:, k]
        assert abs(np.abs(y).max() - 1.0) <= 1e-12
        D, V = primal_ray_test(lp, y)
        assert D > 0 and V <= 10 * EPS * D, (k, D, V)
        A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
        np.testing.assert_allclose(z, -(A.T @ y), rtol=1e-9, atol=1e-12)
        assert abs(cert["objective"][k] - D) <= 1e-6 * abs(D) and cert["violation"][k] <= 10 * EPS * D
        evalref.check_certificate_values(lp, 1, y, float(cert["objective"][k]), float(cert["violation"][k]), "member %d" % k)
        assert cert["d"] is None or not cert["d"][:, k].any()
    else:
        d = cert["d"][:, k]
        assert abs(np.abs(d).max() - 1.0) <= 1e-12
        cd, W = dual_ray_test(lp, d)
        assert cd < 0 and W <= 10 * EPS * -cd, (k, cd, W)
        assert abs(cert["objective"][k] - cd) <= 1e-6 * abs(cd) and cert["violation"][k] <= 10 * EPS * -cd
        evalref.check_certificate_values(lp, 2, d, float(cert["objective"][k]), float(cert["violation"][k]), "member %d" % k)
        assert cert["y"] is None or (not cert["y"][:, k].any() and not cert["z"][:, k].any())


# ---- 1. the three-member batch of tests/test_gpu_batched.py, member 1 infeasible --------------------------------------------------
def test_three_member_batch_with_an_infeasible_member(gpu):
    g = json.load(open(os.path.join(HERE, "golden", "known_lps.json")))
    rp, ci, v = g[0]["rowptr"], g[0]["colind"], [float(t) for t in g[0]["values"]]
    model = hprlp.Model.from_csr(2, 2, rp, ci, v, [-INF, -INF], [10, 12], [0, 0], [INF, INF], [-3, -5])
    B = 3
    Cm = np.array([[-3.0, -5.0]] * B).T
    AU = np.array([[10.0, 12.0]] * B).T
    AL = np.full((2, B), -INF)
    L = np.zeros((2, B)); U = np.full((2, B), INF)
    AL[0, 1] = 11.0
    U[:, 1] = 1.0
    prm = hprlp.Parameters(stop_tol=1e-6, max_iter=3000, use_presolve=False, use_CR_scaling=False)
    off = hprlp.solve_batched(model, Cm, AL, AU, L, U, [0.0, 0.0, 7.0], prm)
    on = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, [0.0, 0.0, 7.0], prm)
    assert off["status"] == ["OPTIMAL", "ITER_LIMIT", "OPTIMAL"]
    assert on["status"] == ["OPTIMAL", "PRIMAL_INFEASIBLE", "OPTIMAL"]
    assert on["iter"][1] <= 1500 and on["iter"][1] % prm.check_iter == 0
    lp1 = dict(m=2, n=2, rowptr=np.array(rp), colind=np.array(ci), values=np.array(v), AL=AL[:, 1], AU=AU[:, 1], l=L[:, 1],
               u=U[:, 1], c=Cm[:, 1])
    _check_certificate(lp1, on, 1)
    assert list(on["certificates"]["kind"]) == [0, 1, 0] and on["certificates"]["d"] is None
    for k in (0, 2):
        _member_equal(on, off, k)
        assert not on["certificates"]["y"][:, k].any() and not on["certificates"]["z"][:, k].any()
    # det == NULL is solve_batched itself
    same = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, [0.0, 0.0, 7.0], prm, eps_primal=None, eps_dual=None)
    for k in range(B):
        _member_equal(same, off, k)
    assert list(same["certificates"]["kind"]) == [0] * B
    model.free()


# ---- 2. mixed batches on one shared matrix, through every panel form -----------------------------------------------------------
M, N, NNZ = 300, 400, 2400
KINDS = ("OPTIMAL", "PRIMAL_INFEASIBLE", "DUAL_INFEASIBLE")


@functools.lru_cache(maxsize=None)
def _shared_matrix():
    return lpgen.planted_infeasible_lp(M, N, NNZ, 500)["A"]


@functools.lru_cache(maxsize=None)
def _member(k):
    """Member k of every mixed batch (interleaved kinds): planted infeasible, planted unbounded, or a planted unbounded one with
    every infinite column bound replaced by -2 / 3 (its box holds the planted point: feasible and bounded).  HiGHS's status."""
    A = _shared_matrix()
    want = KINDS[k % 3]
    if want == "PRIMAL_INFEASIBLE":
        lp = lpgen.planted_infeasible_lp(M, N, NNZ, 1000 + k, A=A)
    else:
        lp = lpgen.planted_unbounded_lp(M, N, NNZ, 1000 + k, A=A)
        if want == "OPTIMAL":
            lp["l"] = np.where(np.isfinite(lp["l"]), lp["l"], -2.0)
            lp["u"] = np.where(np.isfinite(lp["u"]), lp["u"], 3.0)
    return lp, STATUS_OF_HIGHS[highs_status(lp)]


def _mixed(B):
    members = [_member(k) for k in range(B)]
    stack = lambda f: np.stack([lp[f] for lp, _ in members], axis=1)
    lp0 = members[0][0]
    model = hprlp.Model.from_csr(M, N, lp0["rowptr"], lp0["colind"], lp0["values"], lp0["AL"], lp0["AU"], lp0["l"], lp0["u"], lp0["c"])
    return members, model, (stack("c"), stack("AL"), stack("AU"), stack("l"), stack("u"))


def _with_chunk(chunk, fn):
    old = os.environ.get("HPRLP_BATCH_CHUNK")
    try:
        if chunk:
            os.environ["HPRLP_BATCH_CHUNK"] = str(chunk)
        return fn()
    finally:
        os.environ.pop("HPRLP_BATCH_CHUNK", None)
        if old is not None:
            os.environ["HPRLP_BATCH_CHUNK"] = old


MIXED_PRM = dict(stop_tol=1e-6, max_iter=30000, time_limit=60.0, use_presolve=False, use_CR_scaling=False)


@pytest.mark.parametrize("B,chunk", [(5, 0), (64, 0), (70, 8), (70, 32)])
def test_mixed_batch_verdicts_and_certificates(gpu, B, chunk):
    """B = 5: one chunk of 8 (kb_half); 64: kb_half64; 70 with chunks of 8 / 32: kb_halfN."""
    members, model, (Cm, AL, AU, L, U) = _mixed(B)
    assert {s for _, s in members} == set(KINDS)
    prm = hprlp.Parameters(**MIXED_PRM)
    on = _with_chunk(chunk, lambda: hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, None, prm))
    off = _with_chunk(chunk, lambda: hprlp.solve_batched(model, Cm, AL, AU, L, U, None, prm))
    assert on["status"] == [s for _, s in members]
    kinds = on["certificates"]["kind"]
    for k, (lp, want) in enumerate(members):
        if want == "OPTIMAL":
            assert kinds[k] == 0 and on["certificates"]["iter"][k] == 0
            _member_equal(on, off, k)
        else:
            assert on["iter"][k] % prm.check_iter == 0 and on["iter"][k] >= 2 * prm.check_iter, (k, on["iter"][k])
            _check_certificate(lp, on, k)
    model.free()


# ---- 3. the limits keep their place ------------------------------------------------------------------------------------------
def test_iteration_limit_below_the_first_possible_verdict_changes_nothing(gpu):
    """The first ray test runs at the second periodic evaluation (2 x check_iter): below that, detection on is detection off."""
    members, model, (Cm, AL, AU, L, U) = _mixed(5)
    for max_iter in (150, 299):
        prm = hprlp.Parameters(**dict(MIXED_PRM, max_iter=max_iter))
        on = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, None, prm)
        off = hprlp.solve_batched(model, Cm, AL, AU, L, U, None, prm)
        for k in range(5):
            _member_equal(on, off, k)
        assert "ITER_LIMIT" in on["status"]
        c = on["certificates"]
        assert not c["kind"].any() and not c["iter"].any() and c["y"] is None and c["z"] is None and c["d"] is None
    model.free()


# ---- 4. config 4 at full size: no false verdict, same bits ---------------------------------------------------------------------
def test_config4_full_size_with_detection(gpu):
    lp = lpgen.c3_pds20_like()
    B, tol = 64, 1e-4
    Cm, AL, AU, L, U = make_batch(lp, B, 4)
    model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    prm = hprlp.Parameters(stop_tol=tol, max_iter=60000, use_presolve=False)
    on = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, None, prm)
    off = hprlp.solve_batched(model, Cm, AL, AU, L, U, None, prm)
    assert on["status"] == ["OPTIMAL"] * B
    assert not on["certificates"]["kind"].any()
    for k in range(B):
        _member_equal(on, off, k)
    model.free()
