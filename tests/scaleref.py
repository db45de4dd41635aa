"""High-precision reference of Solver::scale() (solver.cpp; oracle/hpr_oracle.c: orc_scaling), with a derived bound on what any
correct FP64 evaluation may differ by.  A plain module: no fixtures.  (The LPs the scaling tests run on are tests/scalecases.py.)

Two things are checked, by different means:

  (a) the Curtis-Reid exponents and the factors t = clamp(exp(w)) made of them, against a longdouble evaluation of the 40 passes;
  (c) identities of the FINISHED scaling (Curtis-Reid, Ruiz, Pock-Chambolle, b / c scaling) that hold whatever the factors
      were, by counting roundings: they use the solver's own outputs and the caller's data only.

u = 2^-53 is the unit roundoff of FP64; every +, -, *, / returns its exact result times (1 + d), |d| <= u.  First order in u
throughout; the tolerance is TOL_FACTOR = 2 x the bound (the u^2 terms, the reference's own 2^-64 roundings) and nothing wider;
no assumption on the order of any sum.

(a) THE CURTIS-REID EXPONENTS.  oracle/hpr_oracle.c: cr_log_update, in the oracle's pass order: 20 x (rows of A from the column
exponents v, then rows of A^T from the row exponents w), both starting at 0.  One pass over the rows of a matrix:

    L_k    = -log(max(|a_k|, 1e-300))                       (the same number in every pass; a stored zero gives 690.77...)
    term_k = L_k - v[col_k]
    w_i    = (sum_k term_k) / len_i,    w_i = 0 for an empty row

  Beside each value its error bound PER ELEMENT (E_v = 0 before the first pass):

    e(term_k) = LOG_ULP u |L_k|  +  E_v[col_k]  +  u |term_k|
                (the device's log; what the input carries; the subtraction)
    E_w[i]    = (sum_k e(term_k) + (len_i - 1) u sum_k |term_k|) / len_i  +  u |w_i|
                (rule (S) of tests/evalref.py for a sum of len terms in ANY order -- CSR order, lanes and a wave reduction, chunk
                 partials added by k_long_finish, tiles then remainder; the division: one more u)

  The pass is a MEAN: sum_k E_v[col_k] / len_i <= max E_v, so a pass hands its input's error on without amplifying it and adds
  its own (about len u mean|term|).  Errors therefore ADD over the 40 passes instead of multiplying; that is the whole reason a
  bound exists.  (An element-free bound would not do: the 5000-entry row's own term is 1e4 times a short row's.)
  The tiled path forms L_k once (launch_tiled_refresh_log) instead of in every pass: the same rounded number, the same bound.

  The factor: t = min(max(exp(w), 1e-30), 1e30).  exp(w + dw) = exp(w) (1 + dw), so the relative error of the unclamped value is
  r = E_w + EXP_ULP u.  The clamp is monotone and 1-Lipschitz: the device's t lies in [clamp(t_un (1 - r)), clamp(t_un (1 + r))],
  and the bound e_t is the larger distance of clamp(t_un) from the two ends -- 0 where both ends are clamped (so a row far beyond
  a clamp must give the clamp's bits), and no row near log 1e30 needs an exclusion.  What the solver exposes after a scaling of
  Curtis-Reid alone is row_norm = 1 / t (one division): e(1 / t) = e_t / t^2 + u / t.

(b) LOG_ULP, EXP_ULP: the device library's error of log and exp in FP64, in units of u relative to the result.  MEASURED
(tests/test_gpu_scaling.py: test_device_log_and_exp_stay_within_the_measured_constants) on an m x 1 matrix, m = 4096, Curtis-Reid
alone: after the first sweep the row exponents are fl(-log|a_i|) and the column's is mean(L_i - L_i) = 0 exactly, every later
sweep reproduces the same bits, so row_norm_i = 1 / exp(fl(-log|a_i|)) and col_norm_0 = 1.
    |a_i| in [1 - 2^-10, 1 + 2^-10]: |L_i| < 1e-3, the log's error is invisible; |row_norm_i - |a_i|| / (u |a_i|) measures exp
        together with the one division.  EXP_ULP therefore already contains that division; e(1 / t) above counts it once more
        (one u in a bound of 1e4 u or more: on the safe side).
    |a_i| = 10^U(-29.5, 29.5): the term LOG_ULP u |L_i| dominates; observed error / (u |L_i|) over |L_i| >= 16 measures log (an upper
        estimate: exp and the division are left in, at most their share over 16).
    |a_i| = 10^U(-250, 250), as the issue proposed for log: beyond 1e+-30 the factor is clamped and the log cannot be seen; those
        rows must carry exactly 1e-30 resp. 1e30, and the others add to the log sample.
The constants are the largest observed figure rounded up to an integer, plus one (inputs not sampled).

(c) IDENTITIES OF THE FINISHED SCALING.  S = (Curtis-Reid ? 1 : 0) + passes <= 12 stages; every stage multiplies (CR) or divides
(Ruiz, Pock-Chambolle) a matrix entry by its row's factor and its column's, and the norms / vectors by one factor:

    AT_val under the transpose permutation holds the BITS of A_val: both copies take the row factor of A first, then the column
        factor (scale_cr_apply and scale_pass: row_first true for A, false for A^T; the oracle: mul_rows before mul_cols on A,
        mul_cols before mul_rows on A^T), and a correctly rounded product does not depend on who forms it.
    A_val[k] row_norm[i] col_norm[j] against the caller's a_k: 2 S roundings on the entry, S - 1 on each norm that starts at 1.0
        (S at most): 4 S u |a_k|.  A stored zero stays 0.
    AL, AU against AL_org / row_norm / b_scale: S roundings on the side, S on the norm, the reciprocal of b_scale and the product
        with it, one to spare: (2 S + 3) u relative.  c against c_org / col_norm / c_scale, l, u against l_org col_norm / b_scale:
        the same count.  An infinite side keeps its infinity and sign; a zero keeps its sign bit.
    norm_b = |max(|AL|, |AU|) over the finite sides|_2 and norm_c = |c|_2 of the vectors the solver holds: a square carries
        u t (rule (Q) with an exact input), the sum rule (S), the root rule (W).  norm_b_org, norm_c_org: 1 + the same norms of the
        caller's vectors (one more u).  b_scale = 1 + the norm of AL, AU BEFORE the b scaling: those are the held ones times
        b_scale, each within 2 u (the reciprocal, the product): b_scale = 1 + |b_scale x held|_2 with e_i = 2 u |value_i|; c_scale
        likewise.  With use_bc_scaling off both are exactly 1.
"""
import math

import numpy as np
from scipy import sparse

from evalref import HAVE_LD, LD, TOL_FACTOR, U, _reduce_rows, _sqrt, _sum

# Measured on an MI355X (gfx950, ROCm device library), 2026-10-20, by test_device_log_and_exp_stay_within_the_measured_constants:
# the largest observed figures are written beside the constants; constant = figure rounded up to an integer, plus one.
LOG_ULP = 2    # measured 0.956 (error of row_norm over u |L|, the rows with |L| >= 16 of the two wide samples; the rounding of fl(-log|a|) alone gives up to 0.5 .. 1)
EXP_ULP = 3    # measured 1.001 (exp and the one division, 4096 rows)

CR_SWEEPS = 20
T_MIN, T_MAX = 1e-30, 1e30
A_FLOOR = 1e-300
MAX_STAGES = 12


def transpose_pattern(m, n, rp, ci):
    """(ATrp, ATci, perm): the CSR pattern of the transpose (rows of A^T = columns of A, entries by ascending row of A: the order
    of oracle.transpose and of the solver's AT_val) and the position in A's arrays of every entry of A^T."""
    nnz = len(ci)
    T = sparse.csr_matrix((np.arange(1, nnz + 1, dtype=np.int64), np.asarray(ci, np.int64), np.asarray(rp, np.int64)), shape=(m, n)).tocsc()
    T.sort_indices()
    return T.indptr.astype(np.int64), T.indices.astype(np.int64), (T.data - 1).astype(np.int64)


def _cr_pass(rp, lens, L, eL, other, e_other, ci, drop, with_bounds):
    term = L - other[ci]
    if drop is not None:
        term[drop] = 0
    s = _reduce_rows(rp, term)
    full = lens > 0
    d = np.where(full, lens, 1).astype(LD)
    w = np.where(full, s / d, LD(0))
    if not with_bounds:
        return w, None
    a = np.abs(term)
    e = eL + e_other[ci] + U * a
    if drop is not None:
        e[drop] = 0
    E = np.where(full, (_reduce_rows(rp, e) + np.maximum(lens - 1, 0) * U * _reduce_rows(rp, a)) / d, LD(0)) + U * np.abs(w)
    return w, E


def cr_exponents(m, n, rp, ci, val, pattern_T=None, drop=None, with_bounds=True, sweeps=CR_SWEEPS, log_ulp=None):
    """The row and column exponents after `sweeps` x (A pass, A^T pass), in np.longdouble: (w, E_w, v, E_v, facts).  drop: index
    (in A's arrays) of one stored entry left out of the sums of BOTH copies in every pass -- its row and its column still divide
    by their full counts, as a kernel that loses an entry would.  with_bounds False: values only (E_w, E_v None).
    facts["term"]: |term_k| of the last A pass (which entries a sum depends on most)."""
    assert HAVE_LD, "np.longdouble is no wider than FP64 here"
    log_ulp = LOG_ULP if log_ulp is None else log_ulp
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    rpT, ciT, perm = pattern_T if pattern_T is not None else transpose_pattern(m, n, rp, ci)
    lens, lensT = np.diff(rp), np.diff(rpT)
    L = -np.log(np.maximum(np.abs(np.asarray(val, dtype=LD)), LD(A_FLOOR)))
    eL = log_ulp * U * np.abs(L)
    LT, eLT = L[perm], eL[perm]
    dropT = None if drop is None else int(np.flatnonzero(perm == drop)[0])
    w, v = np.zeros(m, dtype=LD), np.zeros(n, dtype=LD)
    Ew, Ev = np.zeros(m, dtype=LD), np.zeros(n, dtype=LD)
    for _ in range(sweeps):
        w, Ew = _cr_pass(rp, lens, L, eL, v, Ev, ci, drop, with_bounds)
        v, Ev = _cr_pass(rpT, lensT, LT, eLT, w, Ew, ciT, dropT, with_bounds)
    facts = {"term": np.abs(L - v[ci])}
    return w, Ew, v, Ev, facts


def cr_factor(w, Ew, exp_ulp=None):
    """(t, e_t, 1 / t, e(1 / t)) of exponents with bounds: the clamped factor, and what row_norm / col_norm hold after a scaling
    of Curtis-Reid alone (module docstring (a))."""
    exp_ulp = EXP_ULP if exp_ulp is None else exp_ulp
    lo, hi = LD(T_MIN), LD(T_MAX)
    t_un = np.exp(np.asarray(w, dtype=LD))
    r = np.asarray(Ew, dtype=LD) + exp_ulp * U
    t = np.clip(t_un, lo, hi)
    e_t = np.maximum(np.clip(t_un * (1 + r), lo, hi) - t, t - np.clip(t_un * (1 - r), lo, hi))
    return t, e_t, 1 / t, e_t / (t * t) + U / t


def cr_reference(m, n, rp, ci, val, pattern_T=None, drop=None, with_bounds=True):
    """What a scaling of Curtis-Reid alone leaves in row_norm and col_norm: dict(row=(1/t1, bound), col=(1/t2, bound), w, v, E_w,
    E_v, t_row, t_col, term).  Without bounds (the sensitivity checks) the bound entries are None."""
    w, Ew, v, Ev, facts = cr_exponents(m, n, rp, ci, val, pattern_T, drop, with_bounds)
    z = lambda a: np.zeros(len(a), dtype=LD)
    t1, _, r1, e1 = cr_factor(w, Ew if with_bounds else z(w))
    t2, _, r2, e2 = cr_factor(v, Ev if with_bounds else z(v))
    return dict(row=(r1, e1 if with_bounds else None), col=(r2, e2 if with_bounds else None), w=w, v=v, E_w=Ew, E_v=Ev, t_row=t1, t_col=t2,
                term=facts["term"])


def vector_ratio(got, value, bound):
    """max over the elements of |got - value| / bound (0 where they agree); inf where an element of `got` is not finite or differs
    with a bound of 0 -- a NaN never passes."""
    got = np.asarray(got, dtype=LD)
    if len(got) == 0:
        return 0.0
    if got.shape != np.shape(value) or not np.isfinite(got).all():
        return math.inf
    d = np.abs(got - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, LD(0), np.where(bound > 0, d / bound, LD(np.inf)))
    return float(r.max())


def norm_ratios(row_norm, col_norm, ref, bounds_of=None):
    """{"row_norm": ratio, "col_norm": ratio} of a Curtis-Reid-alone scaling's norms against cr_reference (the bounds of
    `bounds_of` where `ref` was formed without)."""
    b = ref if bounds_of is None else bounds_of
    return {"row_norm": vector_ratio(row_norm, ref["row"][0], b["row"][1]), "col_norm": vector_ratio(col_norm, ref["col"][0], b["col"][1])}


def all_within(r):
    """True where EVERY ratio of the dict r is at most TOL_FACTOR (each compared on its own: a NaN fails)."""
    return all(v <= TOL_FACTOR for v in r.values())


# ---- (c) identities of the finished scaling --------------------------------------------------------------------------------------
SCALED = ("A_val", "AT_val", "AL", "AU", "l", "u", "c", "row_norm", "col_norm")
SCALARS = ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org")


def stages(use_CR_scaling=True, use_Ruiz_scaling=True, use_Pock_Chambolle_scaling=True, **_):
    return int(bool(use_CR_scaling)) + (10 if use_Ruiz_scaling else 0) + int(bool(use_Pock_Chambolle_scaling))


def _same_specials(got, org):
    """0.0 where `got` has the infinities (with sign) of `org` and the zeros of `org` with their sign bits, else inf"""
    got, org = np.asarray(got, np.float64), np.asarray(org, np.float64)
    inf, zero = np.isinf(org), org == 0
    ok = (np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], org[inf]) and np.array_equal(got == 0, zero)
          and np.array_equal(np.signbit(got[zero]), np.signbit(org[zero])) and not np.isnan(got).any())
    return 0.0 if ok else math.inf


def _rel_ratio(got, want, k):
    """max |got - want| / (k u |want|) over the finite nonzero entries of `want` (longdouble)"""
    want = np.asarray(want, dtype=LD)
    sel = np.isfinite(want) & (want != 0)
    if not sel.any():
        return 0.0
    return vector_ratio(np.asarray(got, np.float64)[sel], want[sel], k * U * np.abs(want[sel]))


def _b_terms(AL, AU):
    """max(|AL|, |AU|) over the finite sides (oracle/hpr_oracle.c: conceptual_b_norm), longdouble"""
    a = np.where(np.isinf(AL), 0.0, AL)
    b = np.where(np.isinf(AU), 0.0, AU)
    return np.maximum(np.abs(np.asarray(a, dtype=LD)), np.abs(np.asarray(b, dtype=LD)))


def _norm(t, rel=0.0, plus_one=False, scale=None):
    """(|t|_2 [x scale] [+ 1], bound): entries t >= 0 that carry rel x u |t| each; rules (Q), (S), (W); scale: an exactly known
    factor applied to every entry beforehand (in longdouble: no rounding counted); plus_one: the addition's u."""
    t = np.asarray(t, dtype=LD)
    if scale is not None:
        t = t * LD(scale)
    S, dS = _sum(t * t, 2 * t * (rel * U * t) + U * t * t)
    v, e = _sqrt(S, dS)
    if plus_one:
        v = v + 1
        e = e + U * v
    return v, e


def scalar_reference(lp, got, sc, use_bc_scaling=True):
    """{name: (value, bound)} of the six scalars from the vectors the solver holds (`got`) and the caller's (`lp`)."""
    out = {"norm_b": _norm(_b_terms(got["AL"], got["AU"])), "norm_c": _norm(np.abs(got["c"])),
           "norm_b_org": _norm(_b_terms(lp["AL"], lp["AU"]), plus_one=True), "norm_c_org": _norm(np.abs(lp["c"]), plus_one=True)}
    if use_bc_scaling:
        out["b_scale"] = _norm(_b_terms(got["AL"], got["AU"]), rel=2.0, plus_one=True, scale=sc["b_scale"])
        out["c_scale"] = _norm(np.abs(got["c"]), rel=2.0, plus_one=True, scale=sc["c_scale"])
    else:
        out["b_scale"] = out["c_scale"] = (LD(1), LD(0))
    return out


def identity_ratios(lp, perm, got, sc, S, use_bc_scaling=True):
    """The identities (c) as {name: ratio}: |difference| / bound for the counted ones, 0 / inf for the exact ones.  lp: the
    caller's LP (rowptr, colind, values, AL, AU, l, u, c); perm: transpose_pattern's; got: the solver's SCALED arrays; sc: its
    SCALARS; S: stages()."""
    assert 0 <= S <= MAX_STAGES
    rp, ci = np.asarray(lp["rowptr"], np.int64), np.asarray(lp["colind"], np.int64)
    a = np.asarray(lp["values"], dtype=LD)
    rows = np.repeat(np.arange(lp["m"]), np.diff(rp))
    rn, cn = np.asarray(got["row_norm"], dtype=LD), np.asarray(got["col_norm"], dtype=LD)
    bs, cs = LD(sc["b_scale"]), LD(sc["c_scale"])
    A_val, AT_val = np.asarray(got["A_val"], np.float64), np.asarray(got["AT_val"], np.float64)
    out = {"AT_val bits": 0.0 if (AT_val.shape == A_val.shape and np.array_equal(AT_val.view(np.int64), A_val[perm].view(np.int64))) else math.inf,
           "A_val zeros": _same_specials(A_val, lp["values"]),
           "A_val": vector_ratio(np.asarray(A_val, dtype=LD) * rn[rows] * cn[ci], a, 4 * S * U * np.abs(a)) if S else
                    (0.0 if np.array_equal(A_val, lp["values"]) else math.inf),
           "norms positive": 0.0 if ((rn > 0).all() and (cn > 0).all() and np.isfinite(rn).all() and np.isfinite(cn).all()) else math.inf}
    k = 2 * S + 3
    with np.errstate(invalid="ignore"):
        for name, org, want in (("AL", lp["AL"], np.asarray(lp["AL"], dtype=LD) / rn / bs), ("AU", lp["AU"], np.asarray(lp["AU"], dtype=LD) / rn / bs),
                                ("c", lp["c"], np.asarray(lp["c"], dtype=LD) / cn / cs), ("l", lp["l"], np.asarray(lp["l"], dtype=LD) * cn / bs),
                                ("u", lp["u"], np.asarray(lp["u"], dtype=LD) * cn / bs)):
            out[name + " specials"] = _same_specials(got[name], org)
            out[name] = _rel_ratio(got[name], want, k)
    ref = scalar_reference(lp, got, sc, use_bc_scaling)
    for name in SCALARS:
        v, b = ref[name]
        g = LD(sc[name])
        d = abs(g - v)
        out[name] = math.inf if not (np.isfinite(g) and np.isfinite(v)) else 0.0 if d == 0 else float(d / b) if b > 0 else math.inf
    return out
