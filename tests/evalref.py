"""High-precision evaluator of the EVALUATION side of the iteration (residuals, objectives, gap, KKT error, weighted norm,
movement norms, the iteration-0 bound term), with a derived bound on what any correct FP64 evaluation may differ by.  A plain
module: no fixtures.  (The LPs the evaluation tests run on are tests/evalcases.py.)

What is evaluated (solver.cpp: Solver::compute_residuals, hpr_rules.h: assemble_residuals; scaled data as the solver holds it):

    s  = A^T y_bar            rd_j = (c_j - s_j - z_bar_j) col_norm_j           err_Rd = c_scale sqrt(sum rd_j^2) / norm_c_org
    q  = A x_bar              rp_i = max(min(AU_i - q_i, 0), AL_i - q_i) row_norm_i
                                                                                err_Rp = b_scale sqrt(sum rp_i^2) / norm_b_org
    primal_obj = b_scale c_scale (c . x_bar)        dual_obj = b_scale c_scale (y_obj . y_bar + x_bar . z_bar)
    gap = |primal_obj - dual_obj| / (1 + |primal_obj| + |dual_obj|)             kkt = max(max(err_Rd, err_Rp), gap)
    g  = A x_temp             weighted_norm = sqrt(sigma (lambda |y_temp|^2) + |x_temp|^2 / sigma + 2 (g . y_temp))
    move_x = |x_bar - last_x|, move_y = |y_bar - last_y|
    iteration 0: t_j = l_j - x_bar_j below l, x_bar_j - u_j above u, else 0; r_j = t_j / col_norm_j;
                 lu_term = b_scale sqrt(sum r_j^2); err_Rp0 = max(err_Rp, lu_term)

Values are formed in np.longdouble (64-bit mantissa: its own rounding, 2^-64 per operation, is 2^-11 of FP64's and is covered
by the factor 2 of the tolerance).  Row sums are np.add.reduceat over longdouble products.

THE BOUND.  u = 2^-53 is the unit roundoff of FP64; every +, -, *, /, sqrt returns its exact result times (1 + d), |d| <= u.
First order in u throughout (the tolerance, 2 x the bound, pays for the u^2 terms and the reference's own rounding), and no
assumption on the order of any sum:

  (R) row sum of `len` products a_k v_k: each product carries u |a_k v_k|, and a sum of len terms in ANY order (sequential, tree,
      partial sums of tiles / chunks / pieces added later) carries at most (len - 1) u sum|a_k v_k|: together
      e_row <= (len + 1) u sum|a_k v_k|   (one u to spare).
  (S) a reduction of N terms t_i that carry errors e_i: sum e_i + (N - 1) u sum|t_i|, again for any order.
  (Q) a square t = r^2 of r with error e: 2 |r| e + u r^2.
  (W) a square root of S with error dS: dS / (2 sqrt S) + u sqrt S   (sqrt dS where S = 0).
  (M) a product or quotient with an exactly known factor: one more u |value| each.

  rd_j: the two subtractions are taken against the magnitudes of their operands, which holds for either association:
        e(rd_j) <= col_norm_j (e_row_j + 2 u (|c_j| + |s_j| + |z_bar_j|)) + u |rd_j|.
        err_Rd: (Q), (S) over n, (W), two (M).
  rp_i: max and min are 1-Lipschitz in each argument, so the clamp passes on at most the larger error of its two differences,
        each e_row_i + u |side_i - q_i| for a finite side (an infinite side gives an exact infinity):
        e(rp_i) <= row_norm_i (e_row_i + u max over finite sides |side_i - q_i|) + u |rp_i|.
        err_Rp: (Q), (S) over m, (W), two (M).
  objectives: terms t = a b with u |t| each, (S); dual_obj adds its two reductions (one u |sum|); b_scale c_scale and the
        product with it are two (M).
  gap:  numerator N = |p - d|: e_p + e_d + u N; denominator D = 1 + |p| + |d|: e_p + e_d + 2 u D;
        e(gap) <= e_N / D + gap e_D / D + u gap.
  kkt:  max is 1-Lipschitz in the sup norm: the largest of the three bounds.
  weighted_norm: DY = sum y_temp^2 and DX = sum x_temp^2 by (Q) with e = 0 and (S): N u DY resp. N u DX;
        G = sum g_i y_temp_i: e_i = |y_temp_i| e_row_i + u |g_i y_temp_i|, (S) over m;
        W = sigma (lambda DY) + DX / sigma + 2 G: sigma lambda e_DY + 2 u sigma lambda DY + e_DX / sigma + u DX / sigma + 2 e_G
            + 2 u (sigma lambda DY + DX / sigma + 2 |G|)   (two additions, against the magnitudes);  then (W).
        Where W < 0 the solver raises lambda_max instead; that branch is bounded the same way beside its code below.
  movement: d = a - b carries u |d|; (Q), (S), (W).
  lu_term: t_j carries u |t_j|, the quotient another u |r_j|: e(r_j) = 2 u |r_j|; (Q), (S) over n, (W), one (M).
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TOL_FACTOR = 2.0   # the one multiplier of the bound (second-order terms and the reference's own rounding)
HAVE_LD = np.finfo(LD).nmant >= 63

QUANTITIES = ("err_Rp", "err_Rd", "primal_obj", "dual_obj", "gap", "kkt", "weighted_norm")


def _reduce_rows(rp, terms):
    """Sum of terms[rp[i]:rp[i+1]] per row; empty rows give 0 (np.add.reduceat alone would return the next row's first term)."""
    rows = len(rp) - 1
    out = np.zeros(rows, dtype=terms.dtype)
    rp = np.asarray(rp, dtype=np.int64)
    full = rp[1:] > rp[:-1]
    if full.any():
        out[full] = np.add.reduceat(terms, rp[:-1][full])
    return out


def _row_sums(csr, v, drop=None, dtype=LD):
    """(sum_k a_k v_k, sum_k |a_k v_k|, len) per row of csr = (rowptr, colind, values).  `drop`: index of one stored entry left out
    of the sums (the sensitivity checks).  dtype LD: longdouble products and sums (math.fsum of the exact FP64 products' longdouble
    values where longdouble is no wider than FP64 -- then the products round, the sums do not)."""
    rp, ci, val = csr
    rp = np.asarray(rp, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    lens = np.diff(rp)
    if dtype is LD and not HAVE_LD:
        p = np.asarray(val, np.float64) * np.asarray(v, np.float64)[ci]
        if drop is not None:
            p[drop] = 0.0
        s = np.array([math.fsum(p[rp[i]:rp[i + 1]]) for i in range(len(lens))], dtype=LD)
        return s, _reduce_rows(rp, np.abs(p)).astype(LD), lens
    p = np.asarray(val, dtype=dtype) * np.asarray(v, dtype=dtype)[ci]
    if drop is not None:
        p[drop] = 0
    return _reduce_rows(rp, p), _reduce_rows(rp, np.abs(p)), lens


def _sum(terms, errs=None):
    """(sum, bound) of a reduction by rule (S)."""
    t = np.asarray(terms, dtype=LD)
    n = len(t)
    e = LD(0) if errs is None else np.sum(np.asarray(errs, dtype=LD))
    return np.sum(t), e + max(n - 1, 0) * U * np.sum(np.abs(t))


def _sqrt(S, dS):
    """rule (W)"""
    S = LD(S)
    if S > 0:
        r = np.sqrt(S)
        return r, dS / (2 * r) + U * r
    return LD(0), np.sqrt(LD(dS))


def _norm2(r, e):
    """(sqrt(sum r^2), bound) for entries r with errors e: rules (Q), (S), (W)."""
    r = np.asarray(r, dtype=LD)
    S, dS = _sum(r * r, 2 * np.abs(r) * e + U * r * r)
    return _sqrt(S, dS)


def evaluate(A, AT, data, scalars, st, sigma, lambda_max, drop_A=None, drop_AT=None):
    """All evaluation quantities of a state, each as (value, bound) in np.longdouble.

    A, AT: (rowptr, colind, values) of the scaled matrix and its transpose as the solver holds them; data: c, AL, AU, l, u,
    row_norm, col_norm (scaled); scalars: b_scale, c_scale, norm_b_org, norm_c_org; st: x_bar, y_bar, z_bar, y_obj, x_temp, y_temp,
    last_x, last_y.  drop_A / drop_AT: one stored entry of A / A^T left out (a deliberately wrong evaluation)."""
    g = lambda d, k: np.asarray(d[k], dtype=LD)
    c, AL, AU, l, u = (g(data, k) for k in ("c", "AL", "AU", "l", "u"))
    rn, cn = g(data, "row_norm"), g(data, "col_norm")
    xb, yb, zb, yo, xt, yt = (g(st, k) for k in ("x_bar", "y_bar", "z_bar", "y_obj", "x_temp", "y_temp"))
    b_scale, c_scale = LD(scalars["b_scale"]), LD(scalars["c_scale"])
    nb, nc = LD(scalars["norm_b_org"]), LD(scalars["norm_c_org"])
    sigma, lam = LD(sigma), LD(lambda_max)
    out = {}

    # dual residual
    s, s_abs, s_len = _row_sums(AT, st["y_bar"], drop_AT)
    rd = (c - s - zb) * cn
    e_rd = cn * ((s_len + 1) * U * s_abs + 2 * U * (np.abs(c) + np.abs(s) + np.abs(zb))) + U * np.abs(rd)
    v, e = _norm2(rd, e_rd)
    out["err_Rd"] = (c_scale * v / nc, c_scale * e / nc + 2 * U * c_scale * v / nc)

    # primal residual
    q, q_abs, q_len = _row_sums(A, st["x_bar"], drop_A)
    with np.errstate(invalid="ignore"):
        hi, lo = AU - q, AL - q
        rp = np.maximum(np.minimum(hi, 0), lo) * rn
    side = np.maximum(np.where(np.isfinite(hi), np.abs(hi), 0), np.where(np.isfinite(lo), np.abs(lo), 0))
    e_rp = rn * ((q_len + 1) * U * q_abs + U * side) + U * np.abs(rp)
    v, e = _norm2(rp, e_rp)
    out["err_Rp"] = (b_scale * v / nb, b_scale * e / nb + 2 * U * b_scale * v / nb)

    # objectives and gap
    obj_scale = b_scale * c_scale
    t = c * xb
    S, dS = _sum(t, U * np.abs(t))
    p, e_p = obj_scale * S, obj_scale * dS + 2 * U * abs(obj_scale * S)
    t1, t2 = yo * yb, xb * zb
    S1, d1 = _sum(t1, U * np.abs(t1))
    S2, d2 = _sum(t2, U * np.abs(t2))
    d = obj_scale * (S1 + S2)
    e_d = obj_scale * (d1 + d2 + U * (abs(S1) + abs(S2))) + 2 * U * abs(d)
    out["primal_obj"], out["dual_obj"] = (p, e_p), (d, e_d)
    N, D = abs(p - d), 1 + abs(p) + abs(d)
    gap = N / D
    out["gap"] = (gap, (e_p + e_d + U * N) / D + gap * (e_p + e_d + 2 * U * D) / D + U * gap)
    out["kkt"] = (max(max(out["err_Rd"][0], out["err_Rp"][0]), gap), max(out["err_Rd"][1], out["err_Rp"][1], out["gap"][1]))

    # weighted norm
    gx, gx_abs, _ = _row_sums(A, st["x_temp"], drop_A)
    DY, e_DY = _sum(yt * yt, U * yt * yt)
    DX, e_DX = _sum(xt * xt, U * xt * xt)
    tg = gx * yt
    G, e_G = _sum(tg, np.abs(yt) * (q_len + 1) * U * gx_abs + U * np.abs(tg))
    a1, a2 = sigma * (lam * DY), DX / sigma
    W = a1 + a2 + 2 * G
    e_W = sigma * lam * e_DY + 2 * U * a1 + e_DX / sigma + U * a2 + 2 * e_G + 2 * U * (a1 + a2 + 2 * abs(G))
    out["W"] = (W, e_W)
    if W >= 0:
        out["weighted_norm"], out["lambda_max"] = _sqrt(W, e_W), (lam, LD(0))
    else:
        # lambda_max was too small (solver.cpp: weighted_norm_from): B = -(2 G + DX / sigma) > 0 gives the bumped
        # lambda_max = 1.05 B / (sigma DY) and weighted_norm = sqrt(0.05 B); e_B as in W, the further factors by (M)
        B = -(2 * G + a2)
        e_B = e_DX / sigma + U * a2 + 2 * e_G + U * (a2 + 2 * abs(G))
        out["weighted_norm"] = _sqrt(B * LD(0.05), (e_B + U * abs(B)) * LD(0.05))
        lam2 = B / (sigma * DY) * LD(1.05)
        out["lambda_max"] = (lam2, lam2 * (e_B / abs(B) + e_DY / DY + 3 * U))

    # movement norms
    for name, a, b in (("move_x", xb, g(st, "last_x")), ("move_y", yb, g(st, "last_y"))):
        dlt = a - b
        out[name] = _norm2(dlt, U * np.abs(dlt))

    # iteration-0 bound term
    with np.errstate(invalid="ignore"):
        tt = np.where(xb < l, l - xb, np.where(xb > u, xb - u, LD(0)))
    r = tt / cn
    v, e = _norm2(r, 2 * U * np.abs(r))
    lu = (b_scale * v, b_scale * e + U * b_scale * v)
    out["lu_term"] = lu
    # the vector itself in FP64 from the FP64 inputs (one subtraction, one division: correctly rounded, so the same bits anywhere)
    x64, l64, u64 = (np.asarray(a, np.float64) for a in (st["x_bar"], data["l"], data["u"]))
    with np.errstate(invalid="ignore"):
        t64 = np.where(x64 < l64, l64 - x64, np.where(x64 > u64, x64 - u64, 0.0))
    out["lu_vector"] = t64 / np.asarray(data["col_norm"], np.float64)
    out["err_Rp0"] = (max(out["err_Rp"][0], lu[0]), max(out["err_Rp"][1], lu[1]))
    return out


def evaluate_f64(A, AT, data, scalars, st, sigma, lambda_max, drop_A=None, drop_AT=None, row_sums=None, dot=None):
    """The same quantities by the project's FP64 numpy formulas (tests/test_gpu_kernels.py: test_residuals_and_weighted_norm).
    row_sums(csr, v, drop) and dot(a, b) replace numpy's own summation orders by another FP64 order (the norms then are
    sqrt(dot(r, r)))."""
    c, AL, AU = data["c"], data["AL"], data["AU"]
    obj_scale = scalars["b_scale"] * scalars["c_scale"]
    if row_sums is None:
        row_sums = lambda csr, v, drop: _row_sums(csr, v, drop, np.float64)[0]
    norm = np.linalg.norm if dot is None else (lambda r: np.sqrt(dot(r, r)))
    if dot is None:
        dot = np.dot
    ATy = row_sums(AT, st["y_bar"], drop_AT)
    Ax = row_sums(A, st["x_bar"], drop_A)
    Adx = row_sums(A, st["x_temp"], drop_A)
    pobj = obj_scale * dot(c, st["x_bar"])
    dobj = obj_scale * (dot(st["y_obj"], st["y_bar"]) + dot(st["x_bar"], st["z_bar"]))
    rd = norm((c - ATy - st["z_bar"]) * data["col_norm"]) * scalars["c_scale"] / scalars["norm_c_org"]
    with np.errstate(invalid="ignore"):
        rp = norm(np.maximum(np.minimum(AU - Ax, 0.0), AL - Ax) * data["row_norm"]) * scalars["b_scale"] / scalars["norm_b_org"]
    wn = np.sqrt(sigma * (lambda_max * dot(st["y_temp"], st["y_temp"])) + dot(st["x_temp"], st["x_temp"]) / sigma + 2 * dot(Adx, st["y_temp"]))
    gap = abs(pobj - dobj) / (1.0 + abs(pobj) + abs(dobj))
    return dict(err_Rp=rp, err_Rd=rd, primal_obj=pobj, dual_obj=dobj, gap=gap, kkt=max(max(rd, rp), gap), weighted_norm=wn)


def ratio(got, ref):
    """|got - value| / bound of one quantity (0 where both vanish); inf where `got`, the value or the bound is not finite, so that
    a NaN can never compare as within bounds (and never hides in a max())."""
    v, b = ref
    if not (np.isfinite(LD(got)) and np.isfinite(v) and np.isfinite(b)):
        return math.inf
    d = abs(LD(got) - v)
    if d == 0:
        return 0.0
    return float(d / b) if b > 0 else math.inf


def ratios(got, ref, names=QUANTITIES):
    return {k: ratio(got[k], ref[k]) for k in names}


def within(got, ref, names=QUANTITIES):
    """True where every named quantity of `got` lies within TOL_FACTOR x its bound of the reference."""
    return all_within(ratios(got, ref, names))


def all_within(r):
    """True where EVERY ratio of the dict r is at most TOL_FACTOR (each compared on its own: a NaN fails)."""
    return all(v <= TOL_FACTOR for v in r.values())


def pick_entry(csr, *vectors, rows_ok=None):
    """Index of one stored entry whose product magnitude |a v[col]| is at least the median of the nonzero ones for EVERY given
    vector, in a row that rows_ok allows: the first such entry at or after the middle of the array (a deterministic choice)."""
    rp, ci, val = csr
    ci = np.asarray(ci, dtype=np.int64)
    ok = np.ones(len(val), dtype=bool)
    for v in vectors:
        p = np.abs(np.asarray(val) * np.asarray(v)[ci])
        ok &= p >= np.median(p[p > 0])
    if rows_ok is not None:
        ok &= np.repeat(np.asarray(rows_ok, dtype=bool), np.diff(np.asarray(rp, dtype=np.int64)))
    idx = np.flatnonzero(ok)
    assert len(idx), "no entry qualifies"
    return int(idx[np.searchsorted(idx, len(val) // 2) % len(idx)])


def sensitivity_drops(A, AT, data, st):
    """(drop_A, drop_AT): an entry of A in a row whose primal residual term is not clamped to zero and whose y_temp is not zero
    (so both err_Rp and weighted_norm see it), and an entry of A^T (every column's dual residual term sees its sum)."""
    q = _row_sums(A, st["x_bar"], None, np.float64)[0]
    with np.errstate(invalid="ignore"):
        rp = np.maximum(np.minimum(data["AU"] - q, 0.0), data["AL"] - q)
    rows_ok = (np.abs(rp) >= np.median(np.abs(rp[rp != 0]))) & (np.abs(st["y_temp"]) >= np.median(np.abs(st["y_temp"][st["y_temp"] != 0])))
    return pick_entry(A, st["x_bar"], st["x_temp"], rows_ok=rows_ok), pick_entry(AT, st["y_bar"])


# ---- a solver's own numbers against the evaluator ------------------------------------------------------------------------------
STATE = ("x_bar", "y_bar", "z_bar", "y_obj", "x_temp", "y_temp", "last_x", "last_y")


def solver_inputs(s, rowptr, colind, at_rowptr, at_colind):
    """(A, AT, data, scalars) of evaluate() read back from a solver (hprlp.Solver); the patterns are the model's and its transpose's."""
    data = {k: s.get(k) for k in ("c", "AL", "AU", "l", "u", "row_norm", "col_norm")}
    return (rowptr, colind, s.get("A_val")), (at_rowptr, at_colind, s.get("AT_val")), data, s.scalars()


def solver_state(s):
    return {k: s.get(k) for k in STATE}


def check_solver(s, patterns, got, sigma, lambda_max, names=QUANTITIES, label=""):
    """The values `got` of s.residuals() against the evaluator on the solver's OWN read-back state: every named quantity within
    TOL_FACTOR x its bound.  Prints the observed-difference / bound ratios; returns (inputs, state, reference, ratios)."""
    inp, st = solver_inputs(s, *patterns), solver_state(s)
    want = evaluate(*inp, st, sigma, lambda_max)
    r = ratios(got, want, names)
    print("evaluation", label, " ".join("%s %.3g" % kv for kv in r.items()))
    assert all(np.isfinite(float(want[k][0])) for k in names), {k: want[k] for k in names}
    assert all(np.isfinite(got[k]) for k in names), (label, {k: got[k] for k in names})
    assert all_within(r), (label, r, {k: (got[k], want[k]) for k in names if not r[k] <= TOL_FACTOR})
    return inp, st, want, r
