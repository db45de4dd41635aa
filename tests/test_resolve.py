"""Re-solve of a resident model, the part that needs no GPU (include/hprlp_amd.h hprlp_solver_set_data / hprlp_solver_resolve /
hprlp_solver_data_seconds, DESIGN.md "Re-solve"): the entry points exist with the header's signatures, the rule that scales new
data by the model's cumulative row / column factors is pinned against the CPU oracle's own scaling of the changed LP, and a
NULL solver is refused with a message.  tests/test_gpu_resolve.py imports the LPs, the changes and the rule from here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen
from oracle import oracle as O

SEEDS = (11, 12, 13, 14)
# finite entries of two scalings of the same data agree to this (relative); derived in the docstring of
# test_rule_reproduces_the_oracles_scaling_of_the_changed_lp, not measured
ULPS = 64
BOUND = ULPS * 2.0 ** -53


def base_lp(seed):
    return lpgen.planted_lp(300, 400, 2400, seed, values="network")


def changed(lp, change):
    """The three changes of the issue: a new dict, the matrix untouched."""
    m, n = lp["m"], lp["n"]
    if change == "c1e-3":
        return dict(lp, c=lp["c"] * (1 + 1e-3 * np.random.default_rng(7).normal(size=n)))
    if change == "rows1e-3":
        f = 1 + 1e-3 * np.random.default_rng(8).normal(size=m)
        return dict(lp, AL=lp["AL"] * f, AU=lp["AU"] * f)
    if change == "kinds":
        AL, u = lp["AL"].copy(), lp["u"].copy()
        both = np.flatnonzero(np.isfinite(lp["AL"]) & np.isfinite(lp["AU"]))
        AL[both[::5]] = -np.inf
        boxed = np.flatnonzero(np.isfinite(lp["l"]) & np.isfinite(lp["u"]) & (lp["x_star"] < lp["u"]))
        u[boxed[::5]] = np.inf
        return dict(lp, AL=AL, u=u)
    raise ValueError(change)


def bnorm(AL, AU):
    a = np.where(np.isinf(AL), 0.0, AL)
    b = np.where(np.isinf(AU), 0.0, AU)
    return float(np.sqrt(np.sum(np.maximum(np.abs(a), np.abs(b)) ** 2)))


def rule(lp, row_norm, col_norm, use_bc=True):
    """Section 1 of the issue restated: the scaled vectors and the six scalars of `lp`'s data under given cumulative factors."""
    out = dict(norm_b_org=1 + bnorm(lp["AL"], lp["AU"]), norm_c_org=1 + float(np.linalg.norm(lp["c"])))
    AL, AU, c = lp["AL"] / row_norm, lp["AU"] / row_norm, lp["c"] / col_norm
    l, u = lp["l"] * col_norm, lp["u"] * col_norm
    bs = 1 + bnorm(AL, AU) if use_bc else 1.0
    cs = 1 + float(np.linalg.norm(c)) if use_bc else 1.0
    AL, AU, l, u, c = AL * (1 / bs), AU * (1 / bs), l * (1 / bs), u * (1 / bs), c * (1 / cs)
    out.update(AL=AL, AU=AU, l=l, u=u, c=c, b_scale=bs, c_scale=cs, norm_b=bnorm(AL, AU), norm_c=float(np.linalg.norm(c)))
    return out


def worst_ulps(a, b):
    """Largest relative difference of two arrays (or numbers) in units of 2^-53; infinities must sit in the same places with the
    same sign (inf is returned if they do not)."""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    if a.shape != b.shape or np.isnan(a).any() or np.isnan(b).any():
        return np.inf
    fin = np.isfinite(a)
    if not np.array_equal(fin, np.isfinite(b)) or not np.array_equal(a[~fin], b[~fin]):
        return np.inf
    den = np.maximum(np.abs(a[fin]), np.abs(b[fin]))
    d = np.abs(a[fin] - b[fin])
    rel = np.divide(d, den, out=np.zeros_like(d), where=den > 0)
    return float(rel.max() / 2.0 ** -53) if rel.size else 0.0


def oracle_scaled(lp, **switches):
    return O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                      params=O.Params.default(**switches))


@pytest.mark.parametrize("change", ["c1e-3", "rows1e-3", "kinds"])
@pytest.mark.parametrize("seed", SEEDS)
def test_rule_reproduces_the_oracles_scaling_of_the_changed_lp(seed, change):
    """The oracle scales the base LP and the changed LP from scratch; the rule, fed the BASE LP's row_norm / col_norm and the
    changed data, must give the changed LP's scaled vectors, b_scale, c_scale and norms to ULPS * 2^-53 relative.

    The count behind ULPS = 64 (half-ulps, i.e. units of 2^-53, from Solver::scale() / the oracle's scaling, which round alike):
    a fresh scaling takes AL, AU, l, u, c through one Curtis-Reid product, ten Ruiz and one Pock-Chambolle division and the
    b / c product: 13 roundings.  row_norm / col_norm collect the same twelve factors: 12 roundings.  The rule adds one division by
    them and the b / c product: 2.  So the vectors before the b / c product differ by at most 12 + 13 = 25, b_scale / c_scale
    (1 + the root of a same-order sum of squares of those, the square doubling and the root halving the relative error, plus the
    roundings of root, sum and reciprocal) by at most 25 + 3, and the final vectors by 13 + 14 + 28 = 55 -- the issue counts 57;
    either is below 64, which is what is asserted, with no further margin.  The matrix does not change, so the two row_norm /
    col_norm are the same bits (asserted)."""
    lp = base_lp(seed)
    lp2 = changed(lp, change)
    S, F = oracle_scaled(lp), oracle_scaled(lp2)
    assert np.array_equal(S.row_norm, F.row_norm) and np.array_equal(S.col_norm, F.col_norm)
    got = rule(lp2, S.row_norm, S.col_norm)
    worst = {k: worst_ulps(got[k], getattr(F, k)) for k in ("AL", "AU", "l", "u", "c")}
    worst.update({k: worst_ulps(got[k], getattr(F.sc, k)) for k in ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org")})
    print("seed", seed, change, "worst half-ulps", {k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= ULPS, worst


def test_rule_without_bc_scaling():
    lp = base_lp(11)
    lp2 = changed(lp, "rows1e-3")
    S, F = oracle_scaled(lp, use_bc_scaling=0), oracle_scaled(lp2, use_bc_scaling=0)
    got = rule(lp2, S.row_norm, S.col_norm, use_bc=False)
    assert F.sc.b_scale == 1.0 and F.sc.c_scale == 1.0 and got["b_scale"] == 1.0
    assert max(worst_ulps(got[k], getattr(F, k)) for k in ("AL", "AU", "l", "u", "c")) <= ULPS


def test_changes_are_the_issues():
    lp = base_lp(11)
    assert (int(np.sum(lp["AL"] == lp["AU"])), int(np.sum(np.isinf(lp["AL"]) & np.isfinite(lp["AU"])))) == (162, 138)
    assert (int(np.sum(np.isfinite(lp["l"]) & np.isfinite(lp["u"]))), int(np.sum(np.isfinite(lp["l"]) & np.isinf(lp["u"])))) == (80, 320)
    k = changed(lp, "kinds")
    assert np.sum(np.isinf(k["AL"])) > np.sum(np.isinf(lp["AL"])) and np.sum(np.isinf(k["u"])) > np.sum(np.isinf(lp["u"]))
    assert np.array_equal(k["c"], lp["c"]) and np.array_equal(changed(lp, "c1e-3")["AL"], lp["AL"])


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
CTYPE_OF = {"hprlp_solver *": C.c_void_p, "const double *": hprlp.c_dbl_p, "double *": hprlp.c_dbl_p, "double": C.c_double,
            "int": C.c_int, "int *": hprlp.c_int_p, "HPRLP_results *": C.POINTER(hprlp.CResults),
            "hprlp_trace_row *": C.POINTER(hprlp.CTraceRow)}
WANT = {
    "hprlp_solver_set_data": ["hprlp_solver *"] + ["const double *"] * 6,
    "hprlp_solver_resolve": ["hprlp_solver *", "double", "const double *", "const double *", "HPRLP_results *", "hprlp_trace_row *",
                             "int", "int *"],
    "hprlp_solver_data_seconds": ["hprlp_solver *", "double *"],
}


def header_prototypes():
    """name -> list of parameter types of include/hprlp_amd.h (comments and preprocessor lines removed, as tests/test_abi.py)."""
    text = open(os.path.join(ROOT, "include", "hprlp_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    out = {}
    for mm in re.finditer(r"\b(int|long|double|void)\s+([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", text):
        params = []
        for p in mm.group(3).split(","):
            p = re.sub(r"\[\d*\]", "*", " ".join(p.split()))          # double out[3] -> double out*
            p = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*\s*(\**)$", r"\1", p)   # drop the parameter's name
            params.append(re.sub(r"\s*\*", " *", p).strip())
        out[mm.group(2)] = (mm.group(1), params)
    return out


@pytest.mark.parametrize("name", sorted(WANT))
def test_entry_points_are_exported_with_the_headers_signatures(name):
    protos = header_prototypes()
    assert name in protos, sorted(protos)
    ret, params = protos[name]
    assert ret == "int" and params == WANT[name], (ret, params)
    fn = getattr(hprlp.lib(), name)   # (AttributeError: not exported)
    assert list(fn.argtypes) == [CTYPE_OF[p] for p in params], fn.argtypes
    assert fn.restype is C.c_int


def test_python_solver_has_the_sequence_methods():
    for f in ("prepare", "set_data", "resolve", "data_seconds"):
        assert callable(getattr(hprlp.Solver, f)), f


def test_null_solver_is_refused_with_a_message():
    L = hprlp.lib()
    c = np.zeros(4)
    assert L.hprlp_solver_set_data(None, c.ctypes.data_as(hprlp.c_dbl_p), None, None, None, None, None) == -1
    assert "null solver" in hprlp.last_error()
    res = hprlp.CResults()
    assert L.hprlp_solver_resolve(None, -1.0, None, None, C.byref(res), None, 0, None) == -1
    assert "null solver" in hprlp.last_error()
    out = np.zeros(3)
    assert L.hprlp_solver_data_seconds(None, out.ctypes.data_as(hprlp.c_dbl_p)) == -1
    assert "null solver" in hprlp.last_error()
