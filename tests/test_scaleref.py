"""The scaling reference of tests/scaleref.py on the CPU, against the oracle's scaling (oracle/hpr_oracle.c: orc_scaling) on every
LP of tests/test_gpu_scaling.py: the oracle's Curtis-Reid factors lie within the derived bound of the longdouble recurrence, a
recurrence that leaves one entry out does NOT (by a factor of at least 100), the identities of the finished scaling hold on the
oracle's full scaling and fail on three deliberately wrong ones, and the conditions the bound and the `wide` value law are held to
(largest per-element exponent bound at most 1e-8; a factor at each clamp; finite scaled data) are asserted here."""
import numpy as np
import pytest

import scalecases as SC
import scaleref as R
from conftest import lpgen
from oracle import oracle as O

BOUND_CAP = 1e-8        # the largest per-element exponent bound any case may reach (so that the bound cannot grow until it hides a failure)
SEES_A_DROP = 100.0     # a dropped entry is out of tolerance by at least this factor


def oracle_scaling(lp, **use):
    return O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                      O.Params.default(**{k: int(v) for k, v in use.items()}))


def scaled_of(ref):
    """(the SCALED arrays, the SCALARS) of an oracle scaling, as scaleref.identity_ratios takes a solver's"""
    got = dict(A_val=ref.Av, AT_val=ref.ATv, AL=ref.AL, AU=ref.AU, l=ref.l, u=ref.u, c=ref.c, row_norm=ref.row_norm, col_norm=ref.col_norm)
    return got, {k: getattr(ref.sc, k) for k in R.SCALARS}


def test_longdouble_has_a_64_bit_mantissa():
    assert R.HAVE_LD


def test_transpose_pattern_is_the_oracles():
    lp = SC.case_lp("stream-rows", "wide", lpgen)
    rpT, ciT, perm = SC.pattern_T("stream-rows", "wide", lpgen)
    trp, tci, tv = O.transpose(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"])
    assert np.array_equal(rpT, trp) and np.array_equal(ciT, tci) and np.array_equal(lp["values"][perm], tv)


def test_a_pass_by_hand():
    """2 x 3: rows (a00, a02), (a11); the first A pass is the mean of the logs, the first A^T pass takes the row exponents off; an
    empty column gives 0; the bounds are the docstring's formulas."""
    rp, ci, val = np.array([0, 2, 3]), np.array([0, 2, 1]), np.array([np.e, np.e ** 3, 0.0])
    w, Ew, v, Ev, _ = R.cr_exponents(2, 3, rp, ci, val, sweeps=1, log_ulp=2)
    L0 = -np.log(R.LD(1e-300))
    assert abs(w[0] + 2) < 1e-15 and abs(w[1] - L0) < 1e-15 * L0
    assert abs(v[0] - (-1 - w[0])) < 1e-15 and abs(v[2] - (-3 - w[0])) < 1e-15 and v[1] == L0 - w[1]
    assert abs(Ew[0] - ((2 * R.U * 1 + R.U * 1) + (2 * R.U * 3 + R.U * 3) + R.U * 4) / 2 - R.U * 2) < 1e-30
    w1, _, v1, _, _ = R.cr_exponents(2, 4, rp, ci, val, sweeps=3)
    assert v1[3] == 0 and len(v1) == 4
    # a dropped entry leaves both sums, the counts stay
    wd, _, vd, _, _ = R.cr_exponents(2, 3, rp, ci, val, sweeps=1, drop=1, with_bounds=False)
    assert abs(wd[0] + 0.5) < 1e-15 and vd[2] == 0
    # the factor: clamped on both sides with a bound of exactly 0 far from the clamp's edge, the division's u / t everywhere
    t, e_t, r, e_r = R.cr_factor(np.array([0.0, 100.0, -100.0, np.log(1e30)]), np.full(4, 1e-10))
    assert t[1] == 1e30 and t[2] == 1e-30 and e_t[1] == 0 and e_t[2] == 0 and e_t[0] > 1e-10 and 0 < e_t[3] <= 1.01e-10 * 1e30
    assert e_r[1] == R.U / t[1]


@pytest.mark.parametrize("law", SC.LAWS)
@pytest.mark.parametrize("case", list(SC.CASES))
def test_oracle_curtis_reid_factors_within_the_bound(case, law):
    lp = SC.case_lp(case, law, lpgen)
    ref = SC.reference(case, law, lpgen)
    cap = max(float(ref["E_w"].max()), float(ref["E_v"].max()))
    assert cap <= BOUND_CAP, cap
    orc = oracle_scaling(lp, use_Ruiz_scaling=0, use_Pock_Chambolle_scaling=0, use_bc_scaling=0)
    r = R.norm_ratios(orc.row_norm, orc.col_norm, ref)
    print("scaling", case, law, "LARGEST RATIO row_norm %.3g col_norm %.3g" % (r["row_norm"], r["col_norm"]), "largest exponent bound %.3g" % cap)
    assert R.all_within(r), r
    for label, k in SC.drops(case, law, lpgen).items():
        bad = R.norm_ratios(orc.row_norm, orc.col_norm, SC.reference(case, law, lpgen, drop=k), bounds_of=ref)
        print("scaling", case, law, "without one entry of the", label, "%.3g %.3g" % (bad["row_norm"], bad["col_norm"]))
        assert min(bad.values()) >= SEES_A_DROP * R.TOL_FACTOR, (label, bad)      # its row's factor AND its column's
    if law == "wide":
        f = lp["facts"]
        t1, t2 = ref["t_row"], ref["t_col"]
        assert t1[f["zero_row"]] == R.T_MAX and t1[f["tiny_row"]] == R.T_MAX and t2[f["big_col"]] == R.T_MIN, (t1[f["zero_row"]], t1[f["tiny_row"]], t2[f["big_col"]])
        assert (lp["values"][f["zeros"]] == 0).all() and np.diff(lp["rowptr"])[f["zero_row"]] == 1
        # (far beyond the clamp the bound is 0: the oracle holds the bits of 1 / 1e30)
        assert orc.row_norm[f["zero_row"]] == 1.0 / R.T_MAX and orc.col_norm[f["big_col"]] == 1.0 / R.T_MIN


@pytest.mark.parametrize("law", SC.LAWS)
@pytest.mark.parametrize("case", list(SC.CASES))
def test_identities_of_the_finished_scaling_hold_on_the_oracle_and_see_three_faults(case, law):
    lp = SC.case_lp(case, law, lpgen)
    perm = SC.pattern_T(case, law, lpgen)[2]
    orc = oracle_scaling(lp)
    got, sc = scaled_of(orc)
    S = R.stages()
    assert S == R.MAX_STAGES
    r = R.identity_ratios(lp, perm, got, sc, S)
    print("scaling", case, law, "identities", " ".join("%s %.3g" % kv for kv in r.items()))
    assert R.all_within(r), {k: v for k, v in r.items() if not v <= R.TOL_FACTOR}
    for name in ("A_val", "AT_val", "AL", "AU", "l", "u", "c"):       # finite where the caller's are
        org = lp["values"] if name in ("A_val", "AT_val") else lp[name]
        assert np.isfinite(got[name]).sum() == np.isfinite(org).sum() and not np.isnan(got[name]).any(), name
    # Curtis-Reid alone and no stage at all count their own stages
    for use, S1 in ((dict(use_Ruiz_scaling=0, use_Pock_Chambolle_scaling=0, use_bc_scaling=0), 1),
                    (dict(use_CR_scaling=0, use_Ruiz_scaling=0, use_Pock_Chambolle_scaling=0), 0)):
        g1, s1 = scaled_of(oracle_scaling(lp, **use))
        assert R.stages(**use) == S1
        r1 = R.identity_ratios(lp, perm, g1, s1, S1, use_bc_scaling=use.get("use_bc_scaling", 1))
        assert R.all_within(r1), (use, {k: v for k, v in r1.items() if not v <= R.TOL_FACTOR})
    # 1. one entry of A_val left unscaled in one stage (the last: Pock-Chambolle; the stages before it are the same bits without it)
    before, _ = scaled_of(oracle_scaling(lp, use_Pock_Chambolle_scaling=0))
    k = int(np.argmax(np.abs(before["A_val"] - got["A_val"]) / np.maximum(np.abs(got["A_val"]), 1e-300)))
    bad = dict(got, A_val=got["A_val"].copy())
    bad["A_val"][k] = before["A_val"][k]
    rb = R.identity_ratios(lp, perm, bad, sc, S)
    assert rb["A_val"] > R.TOL_FACTOR and rb["AT_val bits"] > R.TOL_FACTOR, rb
    assert all(v <= R.TOL_FACTOR for n, v in rb.items() if n not in ("A_val", "AT_val bits"))
    # ... and left unscaled in both copies: the bits agree, the value identity still sees it
    bad["AT_val"] = got["AT_val"].copy()
    bad["AT_val"][int(np.flatnonzero(perm == k)[0])] = before["A_val"][k]
    rb = R.identity_ratios(lp, perm, bad, sc, S)
    assert rb["A_val"] > R.TOL_FACTOR and rb["AT_val bits"] == 0, rb
    # 2. one AL misses the b_scale step
    i = int(np.flatnonzero(np.isfinite(got["AL"]) & (got["AL"] != 0))[7])
    bad = dict(got, AL=got["AL"].copy())
    bad["AL"][i] *= sc["b_scale"]
    assert sc["b_scale"] > 1.5
    rb = R.identity_ratios(lp, perm, bad, sc, S)
    assert rb["AL"] > R.TOL_FACTOR, rb
    # 3. one -0.0 turned into +0.0
    j = int(np.flatnonzero((lp["l"] == 0) & np.signbit(lp["l"]))[3])
    assert got["l"][j] == 0 and np.signbit(got["l"][j])
    bad = dict(got, l=got["l"].copy())
    bad["l"][j] = 0.0
    rb = R.identity_ratios(lp, perm, bad, sc, S)
    assert rb["l specials"] > R.TOL_FACTOR and all(v <= R.TOL_FACTOR for n, v in rb.items() if n != "l specials"), rb


def test_a_nan_or_a_wrong_scalar_never_passes():
    lp = SC.case_lp("small", "wide", lpgen)
    perm = SC.pattern_T("small", "wide", lpgen)[2]
    got, sc = scaled_of(oracle_scaling(lp))
    S = R.stages()
    for name in ("A_val", "AL", "c", "u", "row_norm"):
        bad = dict(got, **{name: got[name].copy()})
        bad[name][5] = np.nan
        assert not R.all_within(R.identity_ratios(lp, perm, bad, sc, S)), name
    for name in R.SCALARS:
        for wrong in (sc[name] * (1 + 1e-9), np.nan):
            assert not R.all_within(R.identity_ratios(lp, perm, got, dict(sc, **{name: wrong}), S)), name
    ref = SC.reference("small", "wide", lpgen)
    orc = oracle_scaling(lp, use_Ruiz_scaling=0, use_Pock_Chambolle_scaling=0, use_bc_scaling=0)
    rn = orc.row_norm.copy()
    rn[3] = np.nan
    assert not R.all_within(R.norm_ratios(rn, orc.col_norm, ref))
