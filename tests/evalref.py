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

THE RAY TEST of the infeasibility detection (evaluate_rays; kernels.hip: k_ray_form, RayColEpi, RayRowEpi; solver.cpp:
Solver::ray_test, Solver::ray_scalars).  The scaled rays ds (columns) and ys (rows) are INPUTS, in FP64 as read back (one
subtraction each on the device: the same bits anywhere).  Nine slots, caller's units:

    d_j = (ds_j / cn_j) b_scale                       y_i = (ys_i / rn_i) c_scale
    CD = sum_j ((c_j cn_j) c_scale) d_j               DN = max_j |d_j|              YN = max_i |y_i|
    WD = max(0, max_{l_j finite} -d_j, max_{u_j finite} d_j)
    DY = sum_{y_i > 0, AL_i finite} ((AL_i rn_i) b_scale) y_i + sum_{y_i < 0, AU_i finite} ((AU_i rn_i) b_scale) y_i
    VY = max(0, max_{y_i > 0, AL_i infinite} y_i, max_{y_i < 0, AU_i infinite} -y_i)
    s = A^T ys,  z_j = -((s_j cn_j) c_scale),  lo'_j = (l_j / cn_j) b_scale,  hi'_j = (u_j / cn_j) b_scale
    DZ = sum_{z_j > 0, l_j finite} lo'_j z_j + sum_{z_j < 0, u_j finite} hi'_j z_j
    VZ = max(0, max_{z_j > 0, l_j infinite} z_j, max_{z_j < 0, u_j infinite} -z_j)
    g = A ds,  q_i = (g_i rn_i) b_scale,  WQ = max(0, max_{AL_i finite} -q_i, max_{AU_i finite} q_i)
    D = DY + DZ,  V = max(VY, VZ),  cd = CD,  W = max(WD, WQ),  yn = YN,  dn = DN

  elementwise values: d_j and y_i are a quotient and a product with exactly known factors: 2 u |d_j|, 2 u |y_i|  (M).
  sign branches of y: rn_i > 0 and c_scale > 0, and a correctly rounded quotient or product of a nonzero value by a positive
        factor keeps its sign (and 0 stays 0), so the device takes the branch of y_i that the exact value takes: the branch is exact.
  sums: a term of CD is coefficient x d_j: the coefficient's two products (2 u), the product (u) and the 2 u of d_j: 5 u |t_j|;
        a term of DY the like with y_i: 5 u |t_i|; then (S) over n resp. m.
  products: z_j = -((s_j cn_j) c_scale): e(z_j) = cn_j c_scale e_row_j + 2 u |z_j| by (R), (M); q_i: rn_i b_scale e_row_i + 2 u |q_i|.
  a maximum is 1-Lipschitz in the sup norm: max_k f_k moves by at most max_k |f_k - f_k'|, so the bound of VY, WD, YN, DN, VZ, WQ
        is the LARGEST bound of the elements that may enter it (every column with a finite side for WD, ...); the floor 0 is exact.
  the sign of z_j can flip within e(z_j), so the device may take another branch than the reference.  As functions of z both
        terms of a column are CONTINUOUS at 0 and piecewise linear:
            D-term  f_j(z) = lo'_j z for z > 0 with l_j finite, hi'_j z for z < 0 with u_j finite, else 0:
                    slopes at most L_j = max(|lo'_j|, |hi'_j|) over the finite sides;
            V-term  v_j(z) = z for z > 0 with l_j infinite, -z for z < 0 with u_j infinite, else 0: slopes at most 1.
        Hence |f_j(z) - f_j(z')| <= L_j |z - z'| and |v_j(z) - v_j(z')| <= |z - z'| WHICHEVER branches z and z' take:
            e(D-term_j) = L_j e(z_j) + 3 u |term_j|   (lo'_j or hi'_j: 2 u, the product: u),     e(V-term_j) = e(z_j),
        and every column with an infinite side may enter VZ.  This is what makes a bound possible without knowing the device's
        branch.  DZ: (S) over n.  (q_i enters WQ through the fixed finite sides of its row: no branch on its sign.)
  combinations: D = DY + DZ: e_DY + e_DZ + u |D|; V and W: the larger of the two bounds (a maximum again); cd, yn, dn: the slots'.
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


# ---- the ray test of the infeasibility detection ---------------------------------------------------------------------------------
RAY_SLOTS = ("DY", "CD", "VY", "WD", "YN", "DN", "DZ", "VZ", "WQ")   # (the order of hprlp_solver_ray_step's out[9])
RAY_SUMS = ("D", "V", "cd", "W", "yn", "dn")                          # (Solver::ray_scalars)
RAY_NAMES = RAY_SLOTS + RAY_SUMS
RAY_MAXIMA = ("VY", "WD", "YN", "DN", "VZ", "WQ")


def _ray_elements(dt, data, scalars, s, g, ds, ys, swap_sides):
    """The elementwise parts of the ray test in the arithmetic of the dtype dt, from the row sums s = A^T ys and g = A ds:
    (d, y, z, q, the terms of CD, DY, DZ, and per maximum the element values (0 where the element does not enter) with the mask
    of the elements that MAY enter).  swap_sides: the dual ray's signs paired with the wrong bound (y_i > 0 and z_j > 0 with the
    upper side): a deliberately wrong evaluation."""
    a = lambda k: np.asarray(data[k], dtype=dt)
    c, AL, AU, l, u, rn, cn = (a(k) for k in ("c", "AL", "AU", "l", "u", "row_norm", "col_norm"))
    bs, cs = dt(scalars["b_scale"]), dt(scalars["c_scale"])
    d = (np.asarray(ds, dtype=dt) / cn) * bs
    y = (np.asarray(ys, dtype=dt) / rn) * cs
    z = -((s * cn) * cs)
    q = (g * rn) * bs
    rlo, rhi, clo, chi = (AU, AL, u, l) if swap_sides else (AL, AU, l, u)
    fin, zero = np.isfinite, dt(0)
    with np.errstate(invalid="ignore"):
        t_cd = ((c * cn) * cs) * d
        t_dy = np.where((y > 0) & fin(rlo), ((rlo * rn) * bs) * y, np.where((y < 0) & fin(rhi), ((rhi * rn) * bs) * y, zero))
        lo_, hi_ = (clo / cn) * bs, (chi / cn) * bs
        t_dz = np.where((z > 0) & fin(clo), lo_ * z, np.where((z < 0) & fin(chi), hi_ * z, zero))
    slope = np.maximum(np.where(fin(clo), np.abs(lo_), zero), np.where(fin(chi), np.abs(hi_), zero))
    in_vy = ((y > 0) & ~fin(rlo)) | ((y < 0) & ~fin(rhi))
    el = {"VY": (np.where(in_vy, np.abs(y), zero), in_vy),
          "WD": (np.maximum(np.where(fin(l), -d, zero), np.where(fin(u), d, zero)), fin(l) | fin(u)),
          "YN": (np.abs(y), np.ones(len(y), dtype=bool)),
          "DN": (np.abs(d), np.ones(len(d), dtype=bool)),
          "VZ": (np.where((z > 0) & ~fin(clo), z, np.where((z < 0) & ~fin(chi), -z, zero)), ~fin(clo) | ~fin(chi)),
          "WQ": (np.maximum(np.where(fin(AL), -q, zero), np.where(fin(AU), q, zero)), fin(AL) | fin(AU))}
    return d, y, z, q, t_cd, t_dy, t_dz, slope, el


def _ray_sums(out):
    """the six combinations of Solver::ray_scalars from the nine slots (plain values)"""
    return {"D": out["DY"] + out["DZ"], "V": max(out["VY"], out["VZ"]), "cd": out["CD"], "W": max(out["WD"], out["WQ"]),
            "yn": out["YN"], "dn": out["DN"]}


def evaluate_rays(A, AT, data, scalars, ds, ys, drop_A=None, drop_AT=None, leave_out=None, swap_sides=False):
    """The nine slots (RAY_SLOTS) and six combinations (RAY_SUMS) of the ray test, each as (value, bound) in np.longdouble (the
    module docstring: THE RAY TEST).  A, AT, data, scalars as evaluate(); ds, ys: the scaled rays in FP64.  drop_A / drop_AT: one
    stored entry left out; leave_out: {maximum's name: index of an element left out of it}; swap_sides: see _ray_elements -- three
    deliberately wrong evaluations.  out["elements"]: per maximum the FP64 element values (0 where an element does not enter)."""
    s, s_abs, s_len = _row_sums(AT, ys, drop_AT)
    g, g_abs, g_len = _row_sums(A, ds, drop_A)
    d, y, z, q, t_cd, t_dy, t_dz, slope, el = _ray_elements(LD, data, scalars, s, g, ds, ys, swap_sides)
    rn, cn = np.asarray(data["row_norm"], dtype=LD), np.asarray(data["col_norm"], dtype=LD)
    bs, cs = LD(scalars["b_scale"]), LD(scalars["c_scale"])
    e_z = cn * cs * ((s_len + 1) * U * s_abs) + 2 * U * np.abs(z)
    e_q = rn * bs * ((g_len + 1) * U * g_abs) + 2 * U * np.abs(q)
    e_el = {"VY": 2 * U * np.abs(y), "WD": 2 * U * np.abs(d), "YN": 2 * U * np.abs(y), "DN": 2 * U * np.abs(d), "VZ": e_z, "WQ": e_q}
    out = {"CD": _sum(t_cd, 5 * U * np.abs(t_cd)), "DY": _sum(t_dy, 5 * U * np.abs(t_dy)),
           "DZ": _sum(t_dz, slope * e_z + 3 * U * np.abs(t_dz)), "elements": {}}
    for k in RAY_MAXIMA:
        v, may = el[k]
        may = may.copy()
        if leave_out and k in leave_out:
            may[leave_out[k]] = False
        out["elements"][k] = np.where(may, v, LD(0)).astype(np.float64)
        out[k] = (max(LD(0), v[may].max()), e_el[k][may].max()) if may.any() else (LD(0), LD(0))
    D = out["DY"][0] + out["DZ"][0]
    out["D"] = (D, out["DY"][1] + out["DZ"][1] + U * abs(D))
    out["V"] = (max(out["VY"][0], out["VZ"][0]), max(out["VY"][1], out["VZ"][1]))
    out["W"] = (max(out["WD"][0], out["WQ"][0]), max(out["WD"][1], out["WQ"][1]))
    out["cd"], out["yn"], out["dn"] = out["CD"], out["YN"], out["DN"]
    return out


def evaluate_rays_f64(A, AT, data, scalars, ds, ys, drop_A=None, drop_AT=None, leave_out=None, swap_sides=False, row_sums=None,
                      total=None):
    """The same fifteen numbers in plain FP64 numpy, as the device forms them.  row_sums(csr, v, drop) and total(terms) replace
    numpy's summation orders by another FP64 order; leave_out / swap_sides / drop_*: as evaluate_rays."""
    if row_sums is None:
        row_sums = lambda csr, v, drop: _row_sums(csr, v, drop, np.float64)[0]
    if total is None:
        total = np.sum
    s, g = row_sums(AT, ys, drop_AT), row_sums(A, ds, drop_A)
    _, _, _, _, t_cd, t_dy, t_dz, _, el = _ray_elements(np.float64, data, scalars, s, g, ds, ys, swap_sides)
    out = {"CD": float(total(t_cd)), "DY": float(total(t_dy)), "DZ": float(total(t_dz))}
    for k in RAY_MAXIMA:
        v, may = el[k]
        may = may.copy()
        if leave_out and k in leave_out:
            may[leave_out[k]] = False
        out[k] = max(0.0, float(v[may].max())) if may.any() else 0.0
    out.update(_ray_sums(out))
    return out


def top_two(elements):
    """(arg-max, maximum, runner-up) of a maximum's element values"""
    e = np.asarray(elements, dtype=np.float64)
    j = int(np.argmax(e))
    rest = np.delete(e, j)
    return j, float(e[j]), float(rest.max()) if len(rest) else 0.0


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


def check_rays(s, patterns, got, label=""):
    """The nine slots and six combinations `got` of s.ray_step() against evaluate_rays on the solver's OWN read-back scaled data
    and read-back rays (ray_d, ray_y): every one within TOL_FACTOR x its bound; a value that is not finite fails.  Prints the
    observed-difference / bound ratios; returns (inputs, (ds, ys), reference, ratios)."""
    inp, ds, ys = solver_inputs(s, *patterns), s.get("ray_d"), s.get("ray_y")
    want = evaluate_rays(*inp, ds, ys)
    r = ratios(got, want, RAY_NAMES)
    print("rays", label, " ".join("%s %.3g" % kv for kv in r.items()))
    assert all(np.isfinite(float(want[k][0])) for k in RAY_NAMES), {k: want[k] for k in RAY_NAMES}
    assert all(np.isfinite(got[k]) for k in RAY_NAMES), (label, {k: got[k] for k in RAY_NAMES})
    assert all_within(r), (label, r, {k: (got[k], want[k]) for k in RAY_NAMES if not r[k] <= TOL_FACTOR})
    return inp, (ds, ys), want, r


# ---- the batched ray test (batched.hip: kb_ray_form, kb_ray_col, kb_ray_row, kb_ray_product) ---------------------------------------
# Its device formulas are term by term those of _ray_elements -- (ds / cn) bs, ((c cn) cs) d, ((lo rn) bs) y, -((s cn) cs),
# ((l / cn) bs) z, (s rn) bs -- so evaluate_rays serves per member: that member's column of every read-back panel, the shared
# norms, its b_scale / c_scale.  The one difference is the finiteness rule: a panel holds +-K_INF where the caller passed +-inf.
K_INF = 1.0e100     # csrc/batch_prep.h: kInfReplacement
BOUND_PANELS = ("AL", "AU", "L", "U")


def panel_bounds_to_inf(panel, caller, name=""):
    """A read-back bound panel with +-K_INF mapped to +-inf, after asserting that it holds exactly +K_INF (-K_INF) where, and only
    where, the caller passed +inf (-inf)."""
    panel, caller = np.asarray(panel, np.float64), np.asarray(caller, np.float64)
    assert panel.shape == caller.shape, (name, panel.shape, caller.shape)
    for sign in (1.0, -1.0):
        rep, inf = panel == sign * K_INF, caller == sign * np.inf
        bad = np.argwhere(rep != inf)
        assert not len(bad), (name, "%+g" % (sign * K_INF), "first (line, member):", bad[0].tolist(), "of", len(bad),
                              float(panel[tuple(bad[0])]), float(caller[tuple(bad[0])]))
    assert np.isfinite(panel).all(), name
    return np.where(panel == K_INF, np.inf, np.where(panel == -K_INF, -np.inf, panel))


def batched_member_inputs(A, AT, panels, norms, scalars, k):
    """(A, AT, data, scalars) of evaluate_rays for member k: panels = {C, AL, AU, L, U: (rows, B), bounds with +-inf};
    norms = (row_norm, col_norm); scalars = {b_scale, c_scale: B}."""
    data = dict(c=panels["C"][:, k], AL=panels["AL"][:, k], AU=panels["AU"][:, k], l=panels["L"][:, k], u=panels["U"][:, k],
                row_norm=norms[0], col_norm=norms[1])
    return A, AT, data, dict(b_scale=float(scalars["b_scale"][k]), c_scale=float(scalars["c_scale"][k]))


def check_batched_rays(A, AT, panels, norms, scalars, caller, got, label=""):
    """The nine slots and six combinations per member, `got` (BatchedSolver.ray_step(): a list of dicts, None = not tested), against
    evaluate_rays on the solver's OWN read-back panels (scaled units): C, AL, AU, L, U, ray_d, ray_y, each (rows, B).  A, AT: the
    scaled shared matrix; caller = {AL, AU, L, U} as the caller passed them (+-inf where infinite): the bound panels must hold
    +-K_INF there and nowhere else.  Every number within TOL_FACTOR x its bound; one that is not finite fails.  Returns
    (per member None or (inputs, ds, ys, reference, ratios), the largest ratio per name)."""
    panels = dict(panels)
    for name in BOUND_PANELS:
        panels[name] = panel_bounds_to_inf(panels[name], caller[name], name)
    out, worst = [], {}
    for k, g in enumerate(got):
        if g is None:
            out.append(None)
            continue
        inp = batched_member_inputs(A, AT, panels, norms, scalars, k)
        ds, ys = panels["ray_d"][:, k], panels["ray_y"][:, k]
        want = evaluate_rays(*inp, ds, ys)
        r = ratios(g, want, RAY_NAMES)
        for name, v in r.items():
            worst[name] = max(worst.get(name, 0.0), v)
        assert all(np.isfinite(float(want[n][0])) for n in RAY_NAMES), (label, k, {n: want[n] for n in RAY_NAMES})
        assert all(np.isfinite(g[n]) for n in RAY_NAMES), (label, k, {n: g[n] for n in RAY_NAMES})
        assert all_within(r), (label, "member %d" % k, r, {n: (g[n], want[n]) for n in RAY_NAMES if not r[n] <= TOL_FACTOR})
        out.append((inp, ds, ys, want, r))
    print("batched rays", label, " ".join("%s %.3g" % kv for kv in worst.items()))
    return out, worst


def ray_product(AT, ys):
    """(z, bound) per column of the certificates' product A^T ys in scaled units (kb_ray_product): rule (R), the row-sum term of
    e_z: (len + 1) u sum|a_ij ys_i|."""
    s, s_abs, s_len = _row_sums(AT, ys)
    return s, (s_len + 1) * U * s_abs


def dominated(want, got, inp, ds, ys, slot, line, label="", **drop):
    """The reference shows `line` as the arg-max of `slot` with the runner-up at most half of it, and the evaluator without that
    line (and, with drop_A / drop_AT, without one stored entry of it) is farther than the tolerance from the number `got[slot]`."""
    k, top, second = top_two(want["elements"][slot])
    assert k == line and top > 0 and second <= 0.5 * top, (label, slot, line, k, top, second)
    bad = evaluate_rays(*inp, ds, ys, leave_out={slot: line})
    assert ratio(got[slot], bad[slot]) > TOL_FACTOR, (label, slot, "left out", got[slot], bad[slot])
    if drop:
        bad = evaluate_rays(*inp, ds, ys, **drop)
        assert ratio(got[slot], bad[slot]) > TOL_FACTOR, (label, slot, drop, got[slot], bad[slot])


# ---- the ray test in the caller's units ------------------------------------------------------------------------------------------
# The roundings a number of the model goes through in scale() with use_CR_scaling off (oracle/hpr_oracle.c: orc_scaling; the
# device runs the same passes): 10 Ruiz passes and one Pock-Chambolle pass, then the b / c scaling.
#   a matrix entry: one division by the row factor and one by the column factor per pass: 2 x 11 = 22;
#   row_norm_i and col_norm_j: one multiplication per pass: 11 each;
#   AL_i, AU_i (c_j; l_j, u_j): one division (division; multiplication) per pass: 11, the reciprocal of b_scale (c_scale;
#   b_scale): 1, the multiplication by it: 1: 13.
# Mapped back, a_s rn_i cn_j = a (1 + 44 u) and side_s rn_i b_scale = side (1 + 24 u) (the like for c, l, u); the unscaled ray
# entry y_i = (ys_i / rn_i) c_scale or d_j = (ds_j / cn_j) b_scale that the caller's-units side is given in FP64 carries 2 u.
SCALE_PASSES = 11
K_ENTRY = 2 * SCALE_PASSES + 2 * SCALE_PASSES + 2   # 46: per product a_ij y_i resp. a_ij d_j
K_SIDE = (SCALE_PASSES + 2) + SCALE_PASSES + 2      # 26: per product side_i y_i, bound_j z_j, c_j d_j


def unit_inputs(lp, AT):
    """(A, AT, data, scalars) of evaluate_rays for a model in the caller's own units: no scaling.  AT = (rowptr, colind, values)."""
    data = dict(c=lp["c"], AL=lp["AL"], AU=lp["AU"], l=lp["l"], u=lp["u"], row_norm=np.ones(lp["m"]), col_norm=np.ones(lp["n"]))
    return (lp["rowptr"], lp["colind"], lp["values"]), AT, data, dict(b_scale=1.0, c_scale=1.0)


def caller_units_allowance(A, AT, data, d, y, k_entry=K_ENTRY, k_side=K_SIDE):
    """What D, V, c'd, W of the rays d, y ON THE CALLER'S MODEL (A, AT, data unscaled) may differ by from the same sums formed on
    the scaled model, from the roundings of scale() alone: k_entry u per product with a matrix entry, k_side u per product with a
    side, a bound or a cost; through the maxima and the sign branches of z as the module docstring derives."""
    fin = np.isfinite
    a = lambda k: np.asarray(data[k], dtype=LD)
    c, AL, AU, l, u = (a(k) for k in ("c", "AL", "AU", "l", "u"))
    y, d = np.asarray(y, dtype=LD), np.asarray(d, dtype=LD)
    s, s_abs, _ = _row_sums(AT, y)
    _, g_abs, _ = _row_sums(A, d)
    z = -s
    a_z, a_q = k_entry * U * s_abs, k_entry * U * g_abs
    with np.errstate(invalid="ignore"):
        t_y = np.where((y > 0) & fin(AL), AL * y, np.where((y < 0) & fin(AU), AU * y, LD(0)))
        t_z = np.where((z > 0) & fin(l), l * z, np.where((z < 0) & fin(u), u * z, LD(0)))
    slope = np.maximum(np.where(fin(l), np.abs(l), LD(0)), np.where(fin(u), np.abs(u), LD(0)))
    open_col, shut_row = ~fin(l) | ~fin(u), fin(AL) | fin(AU)
    return {"D": k_side * U * np.sum(np.abs(t_y)) + np.sum(slope * a_z) + k_side * U * np.sum(np.abs(t_z)),
            "V": max(k_side * U * np.abs(y).max(), a_z[open_col].max() if open_col.any() else LD(0)),
            "cd": k_side * U * np.sum(np.abs(c * d)),
            "W": max(k_side * U * np.abs(d).max(), a_q[shut_row].max() if shut_row.any() else LD(0))}


# ---- rays for the tests ----------------------------------------------------------------------------------------------------------
def random_rays(m, n, seed):
    """(ds, ys): standard normal in scaled units, about one entry in eight exactly 0"""
    rng = np.random.default_rng(seed)
    ds, ys = rng.normal(size=n), rng.normal(size=m)
    ds[rng.random(n) < 0.125] = 0.0
    ys[rng.random(m) < 0.125] = 0.0
    return ds, ys


def line_of(csr, k, length, sign=1.0):
    """sign x (stored line k of csr) as a dense vector of `length`: ys = -(column j of A) from A^T gives z_j = cn_j c_scale sum a^2,
    ds = +-(row i of A) gives q_i = +- rn_i b_scale sum a^2"""
    rp, ci, val = csr
    v = np.zeros(length)
    v[np.asarray(ci[rp[k]:rp[k + 1]], dtype=np.int64)] = sign * np.asarray(val[rp[k]:rp[k + 1]], dtype=np.float64)
    return v


def largest_entry(csr, k):
    """index of the stored entry of largest magnitude in line k"""
    rp, _, val = csr
    return int(rp[k] + np.argmax(np.abs(np.asarray(val[rp[k]:rp[k + 1]]))))


def boosted(v, norm, k, sign, factor=4.0):
    """v with entry k set so that sign x v_k / norm_k is `factor` x the largest |v / norm| of the others"""
    v = np.array(v, dtype=np.float64)
    others = np.abs(np.delete(v / norm, k)).max()
    v[k] = sign * factor * others * norm[k]
    return v


def check_certificate_values(lp, kind, ray, objective, violation, label=""):
    """A certificate's objective and violation against D, V (kind 1, ray = y) resp. c'd, W (kind 2, ray = d) of the RETURNED,
    normalised ray, by value and from both sides: evaluate_rays on the caller's model in the caller's units (no scaling: unit norms
    and scales), within TOL_FACTOR x its bound plus the allowance for the roundings of scale() with use_CR_scaling off
    (caller_units_allowance; two more u per product for the division of the ray and of the sums by its infinity norm).  The
    violation of a verdict is what is left of sums that cancel, so its tolerance is large relative to it: the ratios are printed."""
    from scipy import sparse
    A = sparse.csr_matrix((lp["values"], lp["colind"], lp["rowptr"]), shape=(lp["m"], lp["n"]))
    AT = sparse.csr_matrix(A.T)
    AT.sort_indices()
    inp = unit_inputs(lp, (AT.indptr, AT.indices, AT.data))
    ds, ys = (np.zeros(lp["n"]), np.asarray(ray, np.float64)) if kind == 1 else (np.asarray(ray, np.float64), np.zeros(lp["m"]))
    want = evaluate_rays(*inp, ds, ys)
    allow = caller_units_allowance(inp[0], inp[1], inp[2], ds, ys, K_ENTRY + 2, K_SIDE + 2)
    out = {}
    for field, got, name in (("objective", objective, "D" if kind == 1 else "cd"), ("violation", violation, "V" if kind == 1 else "W")):
        v, b = want[name]
        tol = TOL_FACTOR * b + allow[name]
        out[field] = ratio(got, (v, tol))
        print("certificate", label, field, "%.17g" % got, "reference %.17g" % float(v), "difference / tolerance %.3g" % out[field],
              "(tolerance %.3g: bound %.3g, allowance %.3g)" % (float(tol), float(b), float(allow[name])))
    assert all(r <= 1.0 for r in out.values()), (label, out)
    return out
