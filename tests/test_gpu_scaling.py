"""Solver::scale() BY VALUE on every kernel form and row kind (GPU): the 40 Curtis-Reid passes (kernels.hip: CrEpi through
k_spmv_fused in stream mode, vector mode and on split rows with k_long_finish, k_tiled_fused<CrEpi, REP> and its 1024-column
form, k_pb_fused with the far-products pre-pass, and the stream-kernel fall-backs on matrices that have a tiled copy), the exp /
clamp, the scaling pass that also leaves Ruiz pass 0 its norms, and the Ruiz, Pock-Chambolle and b / c stages behind them.

  1. Curtis-Reid alone on the `wide` value law (tests/scalecases.py: both clamps, stored zeros, an all-zero row, empty lines,
     every bound kind): row_norm and col_norm against tests/scaleref.py's longdouble recurrence within 2 x its derived bound and
     nothing wider; a recurrence without one entry is out of it by a factor of 100; the identities of the finished scaling.
  2. The stages after Curtis-Reid are the ORACLE'S BITS: the oracle continues from the outputs of 1. and must land on the bits
     of the GPU's full run, with the fused norms and with HPRLP_NO_FUSED_NORMS=1.
  3. The default scale() on both value laws: the identities, the six scalars included.
  4. The copies the kernels read: after a default scale() the iterates follow the oracle on the GPU's own scaled data, and one
     residual evaluation lies within tests/evalref.py's bound -- a tiled copy refreshed too early or not at all shows here.

Every case asserts its kernel form from describe() and prints its largest ratios.  LOG_ULP and EXP_ULP of scaleref are measured by
the first test.  The group form, the reordered form (tests/test_gpu_reorder_small.py: the scaled data and matrix values of a solver
with a locality ordering against a solver on the explicitly permuted LP, bit for bit, Curtis-Reid on), sharded solvers and set_matrix
re-scaling have their own tests."""
import numpy as np
import pytest

import evalref as E
import scalecases as SC
import scaleref as R
import test_gpu_evaluation as EV
from conftest import hprlp, lpgen
from oracle import oracle as O
from test_gpu_detect import BASE_ENV, FORM_ENV, model_of
from test_gpu_kernels import adopt_gpu_data

pytestmark = pytest.mark.gpu

CR_ALONE = dict(use_Ruiz_scaling=False, use_Pock_Chambolle_scaling=False, use_bc_scaling=False)
SEES_A_DROP = 100.0
_cr_alone = {}      # case -> the arrays a scaling of Curtis-Reid alone left (step 1; step 2 continues from them)
_continued = {}     # case -> the oracle's Ruiz and Pock-Chambolle stages on them


def set_form(monkeypatch, case, **more):
    form, extra, tol = SC.CASES[case]
    for k in EV.FORM_HOOKS + ("HPRLP_NO_TILED_CR", "HPRLP_NO_FUSED_NORMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, **FORM_ENV[form], **extra, **more).items():
        monkeypatch.setenv(k, v)
    return form, tol


def assert_form(s, case, form, **hooks):
    """The kernel form of the case from describe(), the instantiation facts of scalecases.INSTANTIATION among them."""
    d = EV.assert_form(s, case, form)
    head = d.split("; switches:")[0]
    parts = [p for p in head.split("; ") if p.startswith("A: ") or p.startswith("A^T: ")]
    assert len(parts) == 2, d
    assert head.count("tiles of 1024 columns") == (2 if case == "tiled-narrow" else 0), d
    if case in SC.REPEATS:
        assert all(p.endswith(", repeats") == SC.REPEATS[case] for p in parts), d
    if case == "all-remainder":     # every entry is a remainder entry, handed over by source groups (n_groups > 0: launch_far_products<true>)
        assert all("0 % of the entries in staged tiles" in p and ("source-side run tables" in p or "source groups" in p) for p in parts), d
    if case in SC.HAS_TILED_COPY:
        assert s.info()["tiled"] == 3, d
    for k, v in hooks.items():
        assert "%s=%s" % (k, v) in d.split("switches:")[1], d
    return d


def start(monkeypatch, case, lp, hooks=None, **params):
    hooks = hooks or {}
    form, tol = set_form(monkeypatch, case, **hooks)
    model = model_of(lp)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, **params))
    assert_form(s, case, form, **hooks)
    return model, s, tol


def scaled_of(s):
    return {k: s.get(k) for k in R.SCALED}, {k: s.scalars()[k] for k in R.SCALARS}


def assert_finite_where_the_callers_are(lp, got):
    for name in ("A_val", "AT_val", "AL", "AU", "l", "u", "c"):
        org = lp["values"] if name in ("A_val", "AT_val") else lp[name]
        assert np.isfinite(got[name]).sum() == np.isfinite(org).sum() and not np.isnan(got[name]).any(), name
    assert np.isfinite(got["row_norm"]).all() and np.isfinite(got["col_norm"]).all()


def check_identities(lp, perm, got, sc, S, label, use_bc_scaling=True):
    r = R.identity_ratios(lp, perm, got, sc, S, use_bc_scaling)
    print("scaling", label, "identities LARGEST RATIOS", " ".join("%s %.3g" % kv for kv in r.items()))
    assert R.all_within(r), (label, {k: v for k, v in r.items() if not v <= R.TOL_FACTOR})
    assert_finite_where_the_callers_are(lp, got)
    return r


# ---- (b) the device library's log and exp ---------------------------------------------------------------------------------------
def _column_scaling(monkeypatch, a):
    """row_norm, col_norm of an m x 1 matrix of the values a after a scaling of Curtis-Reid alone (stream kernel: the column is
    one vector-mode row of A^T)."""
    for k in EV.FORM_HOOKS + ("HPRLP_NO_TILED_CR", "HPRLP_NO_FUSED_NORMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, **FORM_ENV["stream"]).items():
        monkeypatch.setenv(k, v)
    m = len(a)
    lp = dict(m=m, n=1, rowptr=np.arange(m + 1, dtype=np.int32), colind=np.zeros(m, dtype=np.int32), values=np.asarray(a, np.float64),
              AL=np.full(m, -np.inf), AU=np.ones(m), l=np.zeros(1), u=np.full(1, np.inf), c=np.ones(1))
    model = model_of(lp)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, **CR_ALONE))
    d = s.describe()
    assert "A: stream kernel" in d and "A^T: stream kernel" in d and "0 split rows" in d.split("A^T:")[1], d
    s.scale()
    rn, cn = s.get("row_norm"), s.get("col_norm")
    s.close(); model.free()
    return rn, cn


def test_device_log_and_exp_stay_within_the_measured_constants(gpu, monkeypatch):
    """The construction of scaleref's docstring (b).  Prints the largest observed figures (what LOG_ULP and EXP_ULP were set
    from) and asserts that the device stays within the constants, sample by sample."""
    m = 4096
    rng = np.random.default_rng(2026)
    sign = rng.choice([-1.0, 1.0], size=m)
    samples = {"near 1": sign * (1.0 + rng.uniform(-2.0 ** -10, 2.0 ** -10, size=m)),
               "1e-30 .. 1e30": sign * 10.0 ** rng.uniform(-29.5, 29.5, size=m),
               "1e-250 .. 1e250": sign * 10.0 ** rng.uniform(-250, 250, size=m)}
    fig = {"exp": 0.0, "log": 0.0, "joint": 0.0}
    for label, a in samples.items():
        rn, cn = _column_scaling(monkeypatch, a)
        assert len(cn) == 1 and cn[0] == 1.0, (label, cn)       # the column's exponent is mean(L_i - L_i) = 0 exactly
        assert np.isfinite(rn).all() and (rn > 0).all(), label
        mag = np.abs(a).astype(R.LD)
        L = np.abs(np.log(mag))
        seen = L <= 69.0           # (log 1e30 = 69.08: the factor is not clamped)
        far = L >= 69.2
        assert (seen | far).all()
        # beyond a clamp: exactly 1 / 1e30 resp. 1 / 1e-30
        assert np.array_equal(rn[far], np.where(np.abs(a[far]) < 1, 1.0 / R.T_MAX, 1.0 / R.T_MIN)), label
        err = (np.abs(rn.astype(R.LD) - mag) / (R.U * mag))[seen]
        Ls = L[seen]
        if label == "near 1":
            assert seen.all() and Ls.max() < 1e-3
            fig["exp"] = float(err.max())
        else:
            big = Ls >= 16
            assert big.sum() >= (1500 if far.sum() == 0 else 150), (label, int(big.sum()))
            fig["log"] = max(fig["log"], float((err[big] / Ls[big]).max()))
        fig["joint"] = max(fig["joint"], float((err / (R.LOG_ULP * Ls + R.EXP_ULP)).max()))
        print("device log / exp,", label, "%d rows seen, %d clamped:" % (int(seen.sum()), int(far.sum())),
              "largest error %.4g u, largest error / |L| %.4g u" % (float(err.max()), float((err / np.maximum(Ls, 1e-3)).max())))
    print("device log / exp MEASURED: exp + division %.4g u (EXP_ULP %d), log %.4g u |L| (LOG_ULP %d), error / (LOG_ULP |L| + EXP_ULP) %.4g"
          % (fig["exp"], R.EXP_ULP, fig["log"], R.LOG_ULP, fig["joint"]))
    assert fig["exp"] <= R.EXP_ULP and fig["log"] <= R.LOG_ULP and fig["joint"] <= 1.0, fig


# ---- 1. Curtis-Reid alone ---------------------------------------------------------------------------------------------------------
def _curtis_reid_alone(monkeypatch, case, hooks=None):
    lp = SC.case_lp(case, "wide", lpgen)
    model, s, _ = start(monkeypatch, case, lp, hooks, **CR_ALONE)
    s.scale()
    got, sc = scaled_of(s)
    s.close(); model.free()
    return got, sc


def cr_alone(monkeypatch, case):
    if case not in _cr_alone:
        _cr_alone[case] = _curtis_reid_alone(monkeypatch, case)
    return _cr_alone[case]


@pytest.mark.parametrize("case", list(SC.CASES))
def test_curtis_reid_alone_by_value(gpu, case, monkeypatch):
    lp = SC.case_lp(case, "wide", lpgen)
    ref = SC.reference(case, "wide", lpgen)
    perm = SC.pattern_T(case, "wide", lpgen)[2]
    f = lp["facts"]
    print("scaling", case, "runs", SC.INSTANTIATION[case])
    runs = [("", cr_alone(monkeypatch, case))]
    if case in SC.HAS_TILED_COPY:       # the stream kernel over the CSR arrays of a matrix that has a tiled copy
        runs.append((" HPRLP_NO_TILED_CR=1", _curtis_reid_alone(monkeypatch, case, {"HPRLP_NO_TILED_CR": "1"})))
    for label, (got, sc) in runs:
        r = R.norm_ratios(got["row_norm"], got["col_norm"], ref)
        inside = [(t > R.T_MIN) & (t < R.T_MAX) for t in (ref["t_row"], ref["t_col"])]      # (a clamped factor shows the division's rounding alone)
        free = [R.vector_ratio(got[k][i], ref[key][0][i], ref[key][1][i]) for k, key, i in zip(("row_norm", "col_norm"), ("row", "col"), inside)]
        print("scaling", case + label, "Curtis-Reid alone LARGEST RATIO row_norm %.3g col_norm %.3g" % (r["row_norm"], r["col_norm"]),
              "(unclamped factors alone: %.3g %.3g)" % tuple(free))
        assert R.all_within(r), (case + label, r)
        check_identities(lp, perm, got, sc, 1, case + label + " Curtis-Reid alone", use_bc_scaling=False)
        # the edges of the formula: a stored zero that is its row's only entry, both clamps, empty lines, an all-zero row stays zero
        assert got["row_norm"][f["zero_row"]] == 1.0 / R.T_MAX and got["row_norm"][f["tiny_row"]] == 1.0 / R.T_MAX
        assert got["col_norm"][f["big_col"]] == 1.0 / R.T_MIN
        assert (got["A_val"][f["zeros"]] == 0).all()
        for i in f.get("empty_rows", []):
            assert got["row_norm"][i] == 1.0
        for j in f.get("empty_cols", []):
            assert got["col_norm"][j] == 1.0
        # ... and the comparison can see one entry left out of the sums
        for what, k in SC.drops(case, "wide", lpgen).items():
            bad = R.norm_ratios(got["row_norm"], got["col_norm"], SC.reference(case, "wide", lpgen, drop=k), bounds_of=ref)
            assert min(bad.values()) >= SEES_A_DROP * R.TOL_FACTOR, (case + label, what, bad)


# ---- 2. the stages after Curtis-Reid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused-norms", "separate-norms"])
@pytest.mark.parametrize("case", list(SC.CASES))
def test_stages_after_curtis_reid_are_the_oracles_bits(gpu, case, fused, monkeypatch):
    lp = SC.case_lp(case, "wide", lpgen)
    base, _ = cr_alone(monkeypatch, case)
    if case not in _continued:
        _continued[case] = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], base["A_val"], base["AL"], base["AU"], base["l"], base["u"],
                                      base["c"], O.Params.default(use_CR_scaling=0, use_bc_scaling=0))
    orc = _continued[case]
    hooks = {} if fused else {"HPRLP_NO_FUSED_NORMS": "1"}
    model, s, _ = start(monkeypatch, case, lp, hooks, use_bc_scaling=False)
    s.scale()
    got, sc = scaled_of(s)
    s.close(); model.free()
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)
    for name, want in (("A_val", orc.Av), ("AT_val", orc.ATv), ("AL", orc.AL), ("AU", orc.AU), ("l", orc.l), ("u", orc.u), ("c", orc.c)):
        assert np.array_equal(bits(got[name]), bits(want)), (case, name, int((bits(got[name]) != bits(want)).sum()))
    # the norms: the factors of Curtis-Reid times the later stages' -- S roundings here, S - 1 there, the product
    S = R.stages()
    r = {}
    for name, cont in (("row_norm", orc.row_norm), ("col_norm", orc.col_norm)):
        want = np.asarray(base[name], dtype=R.LD) * np.asarray(cont, dtype=R.LD)
        r[name] = R.vector_ratio(got[name], want, (S + 1) * R.U * np.abs(want))
    print("scaling", case, "fused" if fused else "separate", "norms after all stages LARGEST RATIO row_norm %.3g col_norm %.3g" % (r["row_norm"], r["col_norm"]))
    assert R.all_within(r), r
    assert sc["b_scale"] == 1.0 and sc["c_scale"] == 1.0
    check_identities(lp, SC.pattern_T(case, "wide", lpgen)[2], got, sc, S, case + " no b / c scaling", use_bc_scaling=False)


# ---- 3. and 4. the default scale() --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(SC.CASES))
def test_default_scale_identities_and_the_copies_the_kernels_read(gpu, case, monkeypatch):
    S = R.stages()
    lp = SC.case_lp(case, "wide", lpgen)
    model, s, _ = start(monkeypatch, case, lp)
    s.scale()
    got, sc = scaled_of(s)
    s.close(); model.free()
    check_identities(lp, SC.pattern_T(case, "wide", lpgen)[2], got, sc, S, case + " wide, default")
    lp = SC.case_lp(case, "general", lpgen)
    model, s, tol = start(monkeypatch, case, lp)
    s.scale()
    got, sc = scaled_of(s)
    check_identities(lp, SC.pattern_T(case, "general", lpgen)[2], got, sc, S, case + " general, default")
    # 4. the oracle on the GPU's own scaled data, the real lambda_max
    ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                     O.Params.default(use_CR_scaling=0, use_Ruiz_scaling=0, use_Pock_Chambolle_scaling=0, use_bc_scaling=0))
    adopt_gpu_data(s, ref)
    sigma, lam = 0.6, 1.01 * s.power_iteration()[0]
    s.init(sigma, lam)
    st = ref.new_state()
    s.iterate(7, True)
    k = EV.oracle_steps(ref, st, sigma, lam, 0, 7, True)
    EV.compare_iterates(s, st, tol, "after 7 + check")
    s.iterate(5, False)
    EV.oracle_steps(ref, st, sigma, lam, k, 5, False)
    EV.compare_iterates(s, st, tol, "after 5 more")
    assert np.abs(st["x"]).max() > 0 and np.abs(st["y"]).max() > 0
    res = s.residuals(13, False)
    E.check_solver(s, (lp["rowptr"], lp["colind"], ref.ATrp, ref.ATci), res, sigma, lam, E.QUANTITIES[:-1], case + " after a default scale()")
    s.close(); model.free()
