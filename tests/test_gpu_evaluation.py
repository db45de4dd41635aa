"""The evaluation side of the iteration BY VALUE on every kernel form (GPU): the residual epilogues RdEpi / RpEpi<false> /
RpEpi<true> / GapEpi (kernels.hip) behind hprlp_solver_residuals and hprlp_solver_weighted_norm, the restart (k_movement,
k_restart_copy, the re-gather of y, invalidate_far) with iterations after it, and the iteration-0 bound term (k_lu) with a point
outside [l, u] -- each against tests/evalref.py's high-precision evaluator ON THE SOLVER'S OWN READ-BACK STATE, within 2 x the
derived bound of that module and nothing wider.  Every LP carries every bound kind (evalcases.all_bounds_lp), so the per-form
iterate comparisons with the oracle also run the coded-bound paths (finite nonzero l, -0.0, l = u, ranged and free rows).

Forms: the hook sets of tests/test_gpu_detect.py: FORM_ENV at the smallest shapes existing tests show selecting them
(evalcases.CASES).  The REORDERED form runs these kernels on P A Q; its part is the permutation at the boundary, which
tests/test_gpu_reorder_small.py checks bit for bit against a solver on the explicitly permuted LP (residuals and weighted_norm
included, under HPRLP_REORDER_ANYWAY at 20 011 x 26 003); tests/test_gpu_reorder.py keeps the 1.6 M shape of the default thresholds.

The variant-identity tests pin the switches documented as "the same bits": HPRLP_STORE_X, HPRLP_NO_BOUND_CODES,
HPRLP_NO_FAR_PUSH.  The solver exposes eleven state vectors (NAMES_N + NAMES_M); all of them are compared."""
import numpy as np
import pytest

import evalcases as C
import evalref as E
from conftest import hprlp, lpgen
from oracle import oracle as O
from test_gpu_detect import BASE_ENV, FORM_ENV, model_of
from test_gpu_kernels import NAMES_M, NAMES_N, adopt_gpu_data

pytestmark = pytest.mark.gpu

NAMES = NAMES_N + NAMES_M
FORM_HOOKS = ("HPRLP_NO_SMALL", "HPRLP_NO_TILED", "HPRLP_NO_REORDER", "HPRLP_TILED_MIN_ROWS", "HPRLP_TILED_MIN_DENSE", "HPRLP_TILED_MIN_COLS",
              "HPRLP_TILE_PIECES", "HPRLP_PIECES_ANYWAY", "HPRLP_TILE_ROWS", "HPRLP_TILE_COLS", "HPRLP_DEVICE_TRANSPOSE_MIN", "HPRLP_PB_MIN_COLS",
              "HPRLP_PB_MIN_NNZ", "HPRLP_STORE_X", "HPRLP_NO_BOUND_CODES", "HPRLP_NO_FAR_PUSH", "HPRLP_NO_LONG_SIDE", "HPRLP_NO_GRAPH")
EXPECT = {"small": "single-workgroup kernel", "stream": "A: stream kernel", "tiled": "tiled, fused (k_tiled_fused",
          "pieces": "tiled, piece form", "all-remainder": "all-remainder form (k_pb_fused"}   # (tests/test_gpu_warm.py: FORM_SCRIPT)


def set_form(monkeypatch, case, **more):
    form, extra, tol = C.CASES[case]
    for k in FORM_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, **FORM_ENV[form], **extra, **more).items():
        monkeypatch.setenv(k, v)
    return form, tol


def assert_form(s, case, form):
    d = s.describe()
    assert EXPECT[form] in d, d
    if form == "stream":
        assert "A^T: stream kernel" in d and "single-workgroup" not in d, d
    if form in ("tiled", "pieces", "all-remainder"):
        assert s.info()["tiled"] == 3, d
    if case == "stream-rows":
        assert "2 split rows" in d and "1 split rows" in d, d      # rows of 4097 and 5000 entries in A, a column of 4097 in A^T
    if case == "tiled-rounds":
        assert d.count("625 super-blocks") == 2 and "piece form" not in d and "(64 rows" in d, d   # 625 over 512 slots: a partial second round
    if case == "tiled-aside":
        assert d.count("long rows aside") == 2, d
    return d


def make(lp):
    model = model_of(lp)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                     O.Params.default(use_CR_scaling=0))
    return model, s, ref


def oracle_steps(ref, st, sigma, lam, k, normal, check):
    for _ in range(normal):
        ref.x_half(st, sigma, k, 0)
        ref.y_half(st, sigma, lam, k, 0)
        k += 1
    if check:
        ref.x_half(st, sigma, k, 1)
        ref.y_half(st, sigma, lam, k, 1)
        k += 1
    return k


def compare_iterates(s, st, tol, where):
    for name in NAMES:
        got = s.get(name)
        if tol is None:
            assert np.array_equal(got, st[name]), (where, name, float(np.abs(got - st[name]).max()))
        else:
            np.testing.assert_allclose(got, st[name], rtol=tol[0], atol=tol[1], err_msg="%s %s" % (where, name))


def check_evaluation(s, patterns, got, sigma, lam, label, with_norm=True):
    """Step 3 / 4 of a case: got = s.residuals(...) against the evaluator, lambda_max unchanged, weighted_norm() alone the same."""
    names = E.QUANTITIES if with_norm else E.QUANTITIES[:-1]
    inp, st, want, r = E.check_solver(s, patterns, got, sigma, lam, names, label)
    assert got["lambda_max"] == lam and want["W"][0] > 0, (got["lambda_max"], lam, want["W"])      # no bump
    wn = s.weighted_norm()
    r["weighted_norm() alone"] = E.ratio(wn, want["weighted_norm"])
    print("evaluation", label, "weighted_norm() alone %.3g, equal bits %s" % (r["weighted_norm() alone"], wn == got["weighted_norm"]))
    assert np.isfinite(wn) and r["weighted_norm() alone"] <= E.TOL_FACTOR, (wn, want["weighted_norm"])
    assert s.scalars()["lambda_max"] == lam
    return inp, st, want, r


@pytest.mark.parametrize("case", list(C.CASES))
def test_evaluation_by_value_on_every_kernel_form(gpu, case, monkeypatch):
    form, tol = set_form(monkeypatch, case)
    lp = C.case_lp(case, lpgen)
    model, s, ref = make(lp)
    assert_form(s, case, form)
    patterns = (lp["rowptr"], lp["colind"], ref.ATrp, ref.ATci)
    worst = {}

    def note(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)

    # 1. the scaled data of the GPU on both sides, the real lambda_max
    s.scale()
    adopt_gpu_data(s, ref)
    sigma, lam = 0.6, 1.01 * s.power_iteration()[0]
    s.init(sigma, lam)
    st = ref.new_state()
    # 2. 17 normal iterations and a check step
    s.iterate(17, True)
    k = oracle_steps(ref, st, sigma, lam, 0, 17, True)
    compare_iterates(s, st, tol, "after 17 + check")
    # 3. RdEpi, RpEpi<true>, then GapEpi alone
    got = s.residuals(18, True)
    inp, gst, want, r = check_evaluation(s, patterns, got, sigma, lam, case + " step 18")
    note(r)
    # ... and the comparison can see one entry left out: the evaluator without it is out of bounds of the GPU's numbers
    drop_A, drop_AT = E.sensitivity_drops(inp[0], inp[1], inp[2], gst)
    bad = E.ratios(got, E.evaluate(*inp, gst, sigma, lam, drop_A=drop_A, drop_AT=drop_AT))
    assert min(bad["err_Rp"], bad["err_Rd"], bad["weighted_norm"]) > E.TOL_FACTOR, bad
    # 4. five normal iterations leave the check step's vectors alone; RpEpi<false>
    s.iterate(5, False)
    k = oracle_steps(ref, st, sigma, lam, k, 5, False)
    for name in E.STATE:
        assert np.array_equal(s.get(name), gst[name]), name
    got = s.residuals(23, False)
    assert np.isinf(got["weighted_norm"])     # (not asked for)
    note(check_evaluation(s, patterns, got, sigma, lam, case + " step 23", with_norm=False)[3])
    compare_iterates(s, st, tol, "after 5 more")
    # 5. restart
    xb, yb, lx, ly = (s.get(v) for v in ("x_bar", "y_bar", "last_x", "last_y"))
    new_sigma = s.restart(current_gap=0.3, best_gap=0.3, best_sigma=0.8, err_Rd=1e-2, err_Rp=1e-2, rel_gap=1e-2)
    assert np.array_equal(s.get("x_temp"), xb - lx) and np.array_equal(s.get("y_temp"), yb - ly)
    for name, v in (("x", xb), ("last_x", xb), ("x_bar", xb), ("y", yb), ("last_y", yb), ("y_bar", yb)):
        assert np.array_equal(s.get(name), v), name
    sc = s.scalars()
    assert sc["kx"] == 0 and sc["ky"] == 0 and sc["sigma"] == new_sigma and sc["lambda_max"] == lam
    pm, dm = float(want["move_x"][0]), float(want["move_y"][0])
    assert 1e-16 < pm < 1e12 and 1e-16 < dm < 1e12
    # hpr_rules.h: restart_sigma with kappa = 1 (max(min(err_Rd, err_Rp), min(rel_gap, current_gap)) = 1e-2 > 9e-10)
    rule = np.exp(np.exp(-0.05) * np.log((pm / dm) / np.sqrt(lam)) + (1 - np.exp(-0.05)) * np.log(0.8))
    assert abs(new_sigma - rule) <= 1e-12 * rule, (new_sigma, rule)
    # 6. the same restart on the oracle, nine iterations and a check step on: a stale remainder buffer or a wrong x-rebuild shows here
    for a, b in (("x", "x_bar"), ("last_x", "x_bar"), ("y", "y_bar"), ("last_y", "y_bar")):
        st[a][:] = st[b]
    sigma = new_sigma
    s.iterate(9, True)
    oracle_steps(ref, st, sigma, lam, 0, 9, True)
    compare_iterates(s, st, tol, "after the restart")
    got = s.residuals(10, True)
    note(check_evaluation(s, patterns, got, sigma, lam, case + " step 10 after the restart")[3])
    # 7. iteration 0 from a point outside [l, u]
    s.reset()
    s.init(0.6, lam)
    rng = np.random.default_rng(77)
    l, u = s.get("l"), s.get("u")
    x0 = np.minimum(np.maximum(rng.normal(size=lp["n"]), l), u)
    fin_l = np.flatnonzero(np.isfinite(l))
    below = fin_l[rng.random(len(fin_l)) < 1 / 3]
    fin_u = np.flatnonzero(np.isfinite(u))
    above = np.setdiff1d(fin_u[rng.random(len(fin_u)) < 1 / 3], below)
    x0[below] = l[below] - rng.uniform(0.5, 1.5, size=len(below))
    x0[above] = u[above] + rng.uniform(0.5, 1.5, size=len(above))
    assert len(below) >= lp["n"] // 8 and len(above) >= lp["n"] // 16 and (np.signbit(l[below]) & (l[below] == 0)).any()
    s.set("x_bar", x0)
    s.set("y_bar", rng.normal(size=lp["m"]))
    s.set("z_bar", rng.normal(size=lp["n"]))
    got = s.residuals(0, False)
    inp0, st0 = E.solver_inputs(s, *patterns), E.solver_state(s)
    assert np.array_equal(st0["x_bar"], x0)
    want0 = E.evaluate(*inp0, st0, 0.6, lam)
    assert want0["lu_term"][0] > 0
    r0 = {"err_Rd (iteration 0)": E.ratio(got["err_Rd"], want0["err_Rd"]), "err_Rp (iteration 0)": E.ratio(got["err_Rp"], want0["err_Rp0"])}
    print("evaluation", case, "iteration 0", r0, "bound term %.3g of err_Rp %.3g" % (float(want0["lu_term"][0]), float(want0["err_Rp"][0])))
    assert np.isfinite(got["err_Rd"]) and np.isfinite(got["err_Rp"]), got
    assert E.all_within(r0), (r0, got, want0["err_Rd"], want0["err_Rp0"])
    assert np.array_equal(st0["x_temp"], want0["lu_vector"])      # one subtraction and one division: the same bits
    # (a bound term that forgot the columns below l would be seen)
    miss = dict(inp0[2], l=np.where(np.isin(np.arange(lp["n"]), below), -np.inf, inp0[2]["l"]))
    bad0 = E.evaluate(inp0[0], inp0[1], miss, inp0[3], st0, 0.6, lam)["lu_term"]
    assert E.ratio(np.sqrt(float(np.sum(st0["x_temp"] ** 2))) * inp0[3]["b_scale"], bad0) > E.TOL_FACTOR
    note(r0)
    print("evaluation", case, "LARGEST RATIOS", " | ".join("%s %.3g" % kv for kv in worst.items()))
    s.close(); model.free()


# ---- the variants documented as giving the same bits ----------------------------------------------------------------------------
def _variant_state(monkeypatch, case, lam=None, **hook):
    form, _ = set_form(monkeypatch, case, **hook)
    lp = C.case_lp(case, lpgen)
    model = model_of(lp)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    d = assert_form(s, case, form)
    for k, v in hook.items():
        assert "%s=%s" % (k, v) in d.split("switches:")[1], d
    s.scale()
    if lam is None:
        lam = 1.01 * s.power_iteration()[0]
    s.init(0.6, lam)
    s.iterate(37, True)
    s.iterate(12, False)
    out = {name: s.get(name) for name in NAMES}
    sc = s.scalars()
    assert sc["kx"] == 50 and sc["ky"] == 49
    s.close(); model.free()
    return out, lam, d


def _assert_same_bits(a, b):
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), (name, int((a[name] != b[name]).sum()), float(np.abs(a[name] - b[name]).max()))
    assert np.abs(a["x"]).max() > 0 and np.abs(a["y"]).max() > 0


def test_store_x_gives_the_same_bits(gpu, monkeypatch):
    """HPRLP_STORE_X=1 (every normal x-half reads and stores x) against the default of a tiled matrix (x rebuilt from x_hat and
    last_x by the next launch, "bit for bit the value the previous launch would have stored")."""
    base, lam, d = _variant_state(monkeypatch, "tiled")
    assert "HPRLP_STORE_X" not in d
    other, _, _ = _variant_state(monkeypatch, "tiled", lam, HPRLP_STORE_X="1")
    _assert_same_bits(base, other)


@pytest.mark.parametrize("case", ["tiled", "stream-short"])
def test_no_bound_codes_gives_the_same_bits(gpu, monkeypatch, case):
    """HPRLP_NO_BOUND_CODES=1 (the half-steps read l, u, AL, AU) against the code bytes ("the same values the arrays hold") on an
    LP with every bound kind, -0.0 and l = u included."""
    base, lam, d = _variant_state(monkeypatch, case)
    assert "HPRLP_NO_BOUND_CODES" not in d
    other, _, _ = _variant_state(monkeypatch, case, lam, HPRLP_NO_BOUND_CODES="1")
    _assert_same_bits(base, other)


def test_no_far_push_gives_the_same_bits(gpu, monkeypatch):
    """HPRLP_NO_FAR_PUSH=1 (the remainder pre-pass k_far_products before every half-step) against the hand-off from the producing
    half-step's epilogue: the same products land in the same positions of the remainder buffer, so the sums are the same bits."""
    base, lam, d = _variant_state(monkeypatch, "tiled")
    assert "HPRLP_NO_FAR_PUSH" not in d
    other, _, _ = _variant_state(monkeypatch, "tiled", lam, HPRLP_NO_FAR_PUSH="1")
    _assert_same_bits(base, other)
