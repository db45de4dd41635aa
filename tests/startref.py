"""High-precision reference of the WARM START (DESIGN.md "Warm start"): the map of a caller's point into the scaled, projected
iteration state and the iteration-0 evaluation of it, with a derived bound on what any correct FP64 evaluation may differ by.  A
plain module in the style of tests/evalref.py, whose rules (R), (S), (M) and "continuous across the branch" argument it uses: no
fixtures.  Everything is in SCALED units on the solver's own read-back data (evalref.solver_inputs / batched_member_inputs).

What is formed (kernels.hip: start_in_body, StartColEpi, StartRowEpi; batched.hip: kb_start_seed, kb_start_spmm<true|false>;
hpr_rules.h: assemble_residuals):

    xs_j = clamp((x0_j col_norm_j) / b_scale, l_j, u_j)                    into x, x_hat, x_bar, last_x
    ys_i = (y0_i row_norm_i) / c_scale, then min(ys_i, 0) where AL_i is not finite, then max(ys_i, 0) where AU_i is not finite
                                                                           into y, y_bar, last_y
    s = A^T ys,  w = c - s,  z_bar_j = w_j where (w_j > 0 and l_j finite) or (w_j < 0 and u_j finite), else 0
    S_CX = sum c_j xs_j
    S_XZ = sum f_j(z_bar_j),  f_j(z) = l_j z for z > 0, u_j z for z < 0      (the bound each multiplier leans on, NOT x_bar . z_bar)
    q = A xs,  y_obj_i = AL_i where ys_i > 0, AU_i where ys_i < 0, clamp(q_i, AL_i, AU_i) where ys_i = 0
    S_YOBJ_Y = sum y_obj_i ys_i
    primal_obj = b_scale c_scale S_CX        dual_obj = b_scale c_scale (S_YOBJ_Y + S_XZ)
    gap = |primal_obj - dual_obj| / (1 + |primal_obj| + |dual_obj|)

THE MAP AND THE PROJECTION are IEEE-exact operations on FP64 inputs (one product, one quotient, min / max): start_map() forms them
in float64 in the device's operation order and the device must give the SAME NUMBERS (np.array_equal; the sign of a zero is not
compared, fmin / fmax do not define it).  A null x0 / y0 is the zero vector: it still goes through the clamp, so a column with
l_j > 0 starts at l_j.

THE BOUND (u = 2^-53, first order, no assumption on the order of any sum; the tolerance is TOL_FACTOR = 2 x the bound):

  w_j:  s_j is a row sum of A^T by (R): e_row_j = (len_j + 1) u sum_i |a_ij ys_i|; the subtraction is taken against the magnitudes of
        its operands: e(w_j) = e_row_j + 2 u (|c_j| + |s_j|).
  z_bar_j: as a function of w it is w or 0 on each side of 0 (which of the two depends on the finiteness of l_j, u_j alone):
        continuous and piecewise linear with slopes <= 1.  So |z(w) - z(w')| <= |w - w'| WHICHEVER branch the device takes:
        e(z_bar_j) = e(w_j).
  S_CX: u |t_j| per term, then (S).
  S_XZ: f_j(z(w)) is continuous at 0 with slopes at most L_j = max(|l_j|, |u_j|) over the FINITE sides (an infinite side has z = 0
        on its side of 0); the product adds u |term|: e_j = L_j e(z_bar_j) + u |term_j|, then (S).
  y_obj_i: ys_i is exact (above), so the branch on its sign is exact: AL_i resp. AU_i bit for bit (the projection leaves ys_i > 0
        only where AL_i is finite).  Where ys_i = 0: the clamp is 1-Lipschitz, e = e_row_i = (len_i + 1) u sum_j |a_ij xs_j|.
  S_YOBJ_Y: e_i = |ys_i| e(y_obj_i) + u |t_i|  (the first term vanishes: e(y_obj_i) > 0 only where ys_i = 0), then (S).
  primal_obj: two (M).  dual_obj: the addition of its two sums u (|S_YOBJ_Y| + |S_XZ|), two (M).  gap: as evalref.evaluate.

On the batched device an infinite bound is +-kInfReplacement; evalref.panel_bounds_to_inf maps a read-back bound panel to the
infinities this module tests with np.isfinite.
"""
import numpy as np

import evalref as E
from evalref import LD, U, TOL_FACTOR, HAVE_LD   # noqa: F401  (the same constants: one tolerance for every value module)

VECTORS = ("x", "y", "z_bar", "y_obj")
SUMS = ("S_CX", "S_XZ", "S_YOBJ_Y")
RESULTS = ("primal_obj", "dual_obj", "gap")
SCALARS = SUMS + RESULTS
QUANTITIES = VECTORS + SCALARS

# deliberately wrong starts (tests/test_startref.py shows each outside the tolerance): name -> what is wrong
MUTANTS = {
    "wrong-side": "the dual completion leans on u for w > 0 and on l for w < 0",
    "ignores-finiteness": "the dual completion is w whether or not the bound is finite",
    "AL-AU-swapped": "y_obj is AU for y > 0 and AL for y < 0",
    "no-clamp": "y_obj is the activity itself where y = 0",
    "x-dot-z": "S_XZ is x_bar . z_bar",
    "free-rows-unprojected": "y keeps its value on rows without sides",
    "clamp-before-scaling": "x0 is clamped into [l, u] before it is scaled",
}


def start_map(data, scalars, x0, y0, mutant=None):
    """(xs, ys) in float64, the operation order of start_in_body; x0 / y0 None: zeros.  data: l, u, AL, AU, col_norm, row_norm
    (scaled, as read back); scalars: b_scale, c_scale."""
    f = lambda k: np.asarray(data[k], np.float64)
    l, u, AL, AU, cn, rn = (f(k) for k in ("l", "u", "AL", "AU", "col_norm", "row_norm"))
    bs, cs = np.float64(scalars["b_scale"]), np.float64(scalars["c_scale"])
    x0 = np.zeros(len(l)) if x0 is None else np.asarray(x0, np.float64)
    y0 = np.zeros(len(AL)) if y0 is None else np.asarray(y0, np.float64)
    if mutant == "clamp-before-scaling":
        xs = (np.minimum(np.maximum(x0, l), u) * cn) / bs
    else:
        xs = np.minimum(np.maximum((x0 * cn) / bs, l), u)
    ys = (y0 * rn) / cs
    no_lo, no_hi = ~np.isfinite(AL), ~np.isfinite(AU)
    if mutant == "free-rows-unprojected":
        free = no_lo & no_hi
        no_lo, no_hi = no_lo & ~free, no_hi & ~free
    ys = np.where(no_lo, np.minimum(ys, 0.0), ys)
    ys = np.where(no_hi, np.maximum(ys, 0.0), ys)
    return xs, ys


def _elements(dt, data, xs, ys, s, q, mutant):
    """The elementwise parts in the arithmetic of dtype dt from the row sums s = A^T ys and q = A xs:
    (w, z_bar, terms of S_CX, terms of S_XZ, the slopes L_j, y_obj, the mask ys == 0, terms of S_YOBJ_Y)."""
    a = lambda k: np.asarray(data[k], dtype=dt)
    c, l, u, AL, AU = (a(k) for k in ("c", "l", "u", "AL", "AU"))
    xs, ys = np.asarray(xs, dtype=dt), np.asarray(ys, dtype=dt)
    fin, zero = np.isfinite, dt(0)
    w = c - s
    lo, hi = (u, l) if mutant == "wrong-side" else (l, u)      # the side w > 0 resp. w < 0 leans on
    if mutant == "ignores-finiteness":
        z = w.copy()
    else:
        z = np.where(((w > 0) & fin(lo)) | ((w < 0) & fin(hi)), w, zero)
    t_cx = c * xs
    with np.errstate(invalid="ignore"):
        t_xz = np.where((z > 0) & fin(lo), lo * z, np.where((z < 0) & fin(hi), hi * z, zero))
    if mutant == "x-dot-z":
        t_xz = xs * z
    slope = np.maximum(np.where(fin(l), np.abs(l), zero), np.where(fin(u), np.abs(u), zero))
    at_zero = ys == 0
    pos, neg = (AU, AL) if mutant == "AL-AU-swapped" else (AL, AU)
    clamped = q if mutant == "no-clamp" else np.minimum(np.maximum(q, AL), AU)
    yo = np.where(ys > 0, pos, np.where(ys < 0, neg, clamped))
    with np.errstate(invalid="ignore"):
        t_yy = np.where(at_zero, zero, yo * ys)      # (0 x an infinite y_obj of a free row with y = 0 is 0 on the device too: the clamp is finite)
    return w, z, t_cx, t_xz, slope, yo, at_zero, t_yy


def _results(dt, scalars, S_cx, S_yy, S_xz):
    obj_scale = dt(scalars["b_scale"]) * dt(scalars["c_scale"])
    p = obj_scale * S_cx
    d = obj_scale * (S_yy + S_xz)
    with np.errstate(invalid="ignore"):      # (a deliberately wrong start may sum infinities)
        return obj_scale, p, d, abs(p - d) / (1 + abs(p) + abs(d))


def evaluate_start(A, AT, data, scalars, xs, ys, drop_A=None, drop_AT=None, mutant=None):
    """Every quantity of the iteration-0 evaluation of the projected start (xs, ys), each as (value, bound) in np.longdouble
    (vectors: arrays of values and of bounds); "x" and "y" are the inputs with zero bounds.  out["y_zero"]: the rows with ys = 0
    (where y_obj carries a bound; elsewhere it is a row side bit for bit).  drop_A / drop_AT: one stored entry left out; mutant:
    one of MUTANTS -- deliberately wrong evaluations, with the bounds of the right one."""
    s, s_abs, s_len = E._row_sums(AT, ys, drop_AT)
    q, q_abs, q_len = E._row_sums(A, xs, drop_A)
    w, z, t_cx, t_xz, slope, yo, at_zero, t_yy = _elements(LD, data, xs, ys, s, q, mutant)
    c = np.asarray(data["c"], dtype=LD)
    e_z = (s_len + 1) * U * s_abs + 2 * U * (np.abs(c) + np.abs(s))
    e_yo = np.where(at_zero, (q_len + 1) * U * q_abs, LD(0))
    out = {"x": (np.asarray(xs, dtype=LD), np.zeros(len(xs), dtype=LD)), "y": (np.asarray(ys, dtype=LD), np.zeros(len(ys), dtype=LD)),
           "z_bar": (z, e_z), "y_obj": (yo, e_yo), "y_zero": at_zero, "w": (w, e_z)}
    out["S_CX"] = E._sum(t_cx, U * np.abs(t_cx))
    out["S_XZ"] = E._sum(t_xz, slope * e_z + U * np.abs(t_xz))
    out["S_YOBJ_Y"] = E._sum(t_yy, np.abs(np.asarray(ys, dtype=LD)) * e_yo + U * np.abs(t_yy))
    (S0, d0), (S1, d1), (S2, d2) = out["S_CX"], out["S_YOBJ_Y"], out["S_XZ"]
    obj_scale, p, d, gap = _results(LD, scalars, S0, S1, S2)
    e_p = obj_scale * d0 + 2 * U * abs(p)
    e_d = obj_scale * (d1 + d2 + U * (abs(S1) + abs(S2))) + 2 * U * abs(d)
    out["primal_obj"], out["dual_obj"] = (p, e_p), (d, e_d)
    N, D = abs(p - d), 1 + abs(p) + abs(d)
    out["gap"] = (gap, (e_p + e_d + U * N) / D + gap * (e_p + e_d + 2 * U * D) / D + U * gap)
    return out


def evaluate_start_f64(A, AT, data, scalars, xs, ys, drop_A=None, drop_AT=None, row_sums=None, total=None, mutant=None):
    """The same quantities in plain FP64 numpy, as the device forms them.  row_sums(csr, v, drop) and total(terms) replace numpy's
    summation orders by another FP64 order; mutant: one of MUTANTS (those of the map belong to start_map)."""
    if row_sums is None:
        row_sums = lambda csr, v, drop: E._row_sums(csr, v, drop, np.float64)[0]
    if total is None:
        total = np.sum
    s, q = row_sums(AT, ys, drop_AT), row_sums(A, xs, drop_A)
    _, z, t_cx, t_xz, _, yo, _, t_yy = _elements(np.float64, data, xs, ys, s, q, mutant)
    out = {"x": np.asarray(xs, np.float64), "y": np.asarray(ys, np.float64), "z_bar": z, "y_obj": yo,
           "S_CX": float(total(t_cx)), "S_XZ": float(total(t_xz)), "S_YOBJ_Y": float(total(t_yy))}
    _, out["primal_obj"], out["dual_obj"], out["gap"] = _results(np.float64, scalars, out["S_CX"], out["S_YOBJ_Y"], out["S_XZ"])
    return out


def reference(A, AT, data, scalars, x0, y0):
    """evaluate_start of start_map: the whole start from the caller's point"""
    xs, ys = start_map(data, scalars, x0, y0)
    return evaluate_start(A, AT, data, scalars, xs, ys)


def restatement(A, AT, data, scalars, x0, y0, mutant=None, **kw):
    xs, ys = start_map(data, scalars, x0, y0, mutant)
    return evaluate_start_f64(A, AT, data, scalars, xs, ys, mutant=mutant, **kw)


def vector_ratio(got, ref):
    """The largest |got - value| / bound over the elements of a vector (0 where they agree, so a zero bound asks for the same
    number); inf where an element of `got`, of the value or of the bound is not finite on one side only or is a NaN, so that a NaN
    never compares as within bounds.  An infinite element equal on both sides (a row side) agrees."""
    v, b = ref
    got = np.asarray(got, dtype=LD)
    v, b = np.asarray(v, dtype=LD), np.broadcast_to(np.asarray(b, dtype=LD), np.shape(v))
    if got.shape != v.shape:
        return np.inf
    same = got == v                               # (+-inf == +-inf: True; NaN: False; -0.0 == +0.0: True)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(got - v)
        r = np.where(same, LD(0), np.where(np.isfinite(d) & np.isfinite(b) & (b > 0), d / np.where(b > 0, b, LD(1)), LD(np.inf)))
    return float(r.max()) if r.size else 0.0


def ratio(got, ref):
    return vector_ratio(got, ref) if np.ndim(ref[0]) else E.ratio(got, ref)


def ratios(got, ref, names=QUANTITIES):
    return {k: ratio(got[k], ref[k]) for k in names}


def all_within(r):
    return E.all_within(r)


def sensitivity_drops(A, AT, data, xs, ys):
    """(drop_A, drop_AT): an entry of A in a row whose y_obj IS its activity (ys = 0, the activity strictly inside the sides),
    and an entry of A^T in a column with both bounds finite (z_bar = w there whatever its sign)."""
    q = E._row_sums(A, xs, None, np.float64)[0]
    AL, AU, l, u = (np.asarray(data[k], np.float64) for k in ("AL", "AU", "l", "u"))
    rows_ok = (np.asarray(ys) == 0) & (q > AL) & (q < AU)
    cols_ok = np.isfinite(l) & np.isfinite(u)
    return E.pick_entry(A, xs, rows_ok=rows_ok), E.pick_entry(AT, ys, rows_ok=cols_ok)


def caller_units_z_allowance(AT, c, y, z, curtis_reid=False):
    """Per column, what the returned z = (z_bar col_norm) c_scale may differ by from the dual completion formed ON THE CALLER'S
    MODEL from the returned y, from the roundings of scale() and of the maps alone -- evalref.caller_units_allowance's rule per
    element: K_ENTRY u per product a_ij y_i, K_SIDE u on c_j, and the two products of the map back on z_j.  With Curtis-Reid on,
    scale() has one stage more (tests/scaleref.py: S <= 12): two roundings more per entry, one more per norm and per side."""
    extra = 1 if curtis_reid else 0
    k_entry, k_side = E.K_ENTRY + 4 * extra, E.K_SIDE + 2 * extra
    _, s_abs, _ = E._row_sums(AT, y)
    return k_entry * U * s_abs + k_side * U * np.abs(np.asarray(c, dtype=LD)) + 2 * U * np.abs(np.asarray(z, dtype=LD))


# ---- starts for the tests --------------------------------------------------------------------------------------------------------
def case_start(lp, seed):
    """(x0, y0) in the caller's units for an LP of evalcases.all_bounds_lp: the planted point plus normal noise (scale 2 and 1, as
    tests/test_gpu_warm.py), with x0 = l resp. x0 = u on every eighth group of eight columns (where that bound is finite: each
    column kind is in each group) and y0 = -0.0 on every eighth group of five rows.  tests/test_startref.py confirms on the CPU
    what these starts reach."""
    rng = np.random.default_rng(seed)
    n, m, l, u = lp["n"], lp["m"], lp["l"], lp["u"]
    x0 = lp["x_star"] + rng.normal(scale=2.0, size=n)
    y0 = lp["y_star"] + rng.normal(scale=1.0, size=m)
    group = (np.arange(n) // 8) % 8
    x0 = np.where((group == 1) & np.isfinite(l), l, np.where((group == 2) & np.isfinite(u), u, x0))
    y0[(np.arange(m) // 5) % 8 == 1] = -0.0
    return x0, y0


def case_seed(case_index):
    return 500 + case_index


# ---- a solver's own numbers against the reference --------------------------------------------------------------------------------
def check_vectors(got, want, label=""):
    """z_bar per element within TOL_FACTOR x its bound; y_obj the row side's bits where y != 0 and within TOL_FACTOR x its bound
    where y = 0.  Returns the two largest ratios."""
    r = {"z_bar": vector_ratio(got["z_bar"], want["z_bar"])}
    yo, (v, b), zero = np.asarray(got["y_obj"], np.float64), want["y_obj"], want["y_zero"]
    assert np.array_equal(yo[~zero], np.asarray(v[~zero], np.float64)), (label, "y_obj where y != 0")
    r["y_obj"] = vector_ratio(yo[zero], (v[zero], b[zero]))
    assert all_within(r), (label, r)
    return r
