"""The LPs the scaling tests run on (tests/test_scaleref.py, tests/test_gpu_scaling.py): the patterns and hook sets of
tests/evalcases.py, each under two value laws, with the Curtis-Reid reference of tests/scaleref.py formed once per process.
A plain module: no fixtures.

Which CrEpi instantiation (kernels.hip: launch_cr_log_update) the 40 Curtis-Reid passes of a case run -- INSTANTIATION below; the
test asserts the form from describe().

Value laws:
  general  evalcases.case_lp unchanged: N(0,1) 10^U(-1,1), logs within +-2.3, nothing near a clamp.
  wide     the same pattern and bound kinds (evalcases.all_bounds_lp) with values N(0,1) 10^U(-6,6); three stored zeros, one of
           them its row's only entry (fmax(|a|, 1e-300): exponent ~690, clamped; the row then is all zero and the norm passes that
           follow give it 1); one short row times 1e-40 (factor clamped at 1e30) and one short column times 1e35 (clamped at 1e-30).
           Where the pattern has no row of one entry, one short row is cut down to its first entry (no other line changes)."""
import numpy as np
from scipy import sparse

import evalcases as C
import scaleref as R

# case -> (hook set's name in tests/test_gpu_detect.py: FORM_ENV, further hooks, iterate tolerance (rtol, atol) or None = bits);
# evalcases.CASES, with the tile width of the two fused cases pinned to 2048 columns (whatever Solver::choose_sb_rows would pick for
# the band) so that "tiled-narrow" is the one case on k_tiled_fused<CrEpi, false, false, true>.
CASES = dict(C.CASES)
CASES["tiled"] = ("tiled", {"HPRLP_TILE_COLS": "2048"}, C.CASES["tiled"][2])
CASES["tiled-rounds"] = ("tiled", {"HPRLP_TILE_ROWS": "64", "HPRLP_TILE_COLS": "2048"}, C.CASES["tiled-rounds"][2])
CASES["tiled-narrow"] = ("tiled", {"HPRLP_TILE_COLS": "1024"}, C.CASES["tiled"][2])
PATTERN = {"tiled-narrow": "tiled"}     # (a case on another case's LP)
LAWS = ("general", "wide")

INSTANTIATION = {
    "small": "k_spmv_fused<CrEpi>, stream mode (rows of at most 64 entries, added in CSR order)",
    "stream-short": "k_spmv_fused<CrEpi>, stream mode",
    "stream-rows": "k_spmv_fused<CrEpi>: stream mode, VECTOR mode (rows of 65, 350 entries: the 8-wide, 4-wide and masked-tail loops, the "
                   "log term in term<Epi>) and SPLIT rows (4097 and 5000 entries in A, 4097 in A^T: long_partial, k_long_finish<CrEpi>; "
                   "the 4097th entry is alone in its chunk); empty rows and an empty column",
    "tiled": "k_tiled_fused<CrEpi, true> (tiled.repeats: describe() says `repeats`), on the copy's -log|a| values",
    "tiled-rounds": "k_tiled_fused<CrEpi, false> (64-row super-blocks: no tile has a second step), 625 super-blocks over 512 slots",
    "tiled-narrow": "k_tiled_fused<CrEpi, false, false, true>: tiles of 1024 columns",
    "pieces": "cr_runs_tiled() false (piece form): k_spmv_fused<CrEpi> over the CSR arrays of a matrix that HAS a tiled copy; "
              "refresh_tiled picks the scaled values up afterwards",
    "all-remainder": "k_pb_fused<CrEpi, false> with launch_far_products<true> (n_groups > 0)",
    "tiled-aside": "cr_runs_tiled() false (side_nblk != 0): k_spmv_fused<CrEpi> and k_long_finish<CrEpi> (rows of 1100 and 4200 entries) "
                   "over the CSR arrays of a matrix that has a tiled copy",
}
REPEATS = {"tiled": True, "tiled-rounds": False}     # what describe() must say of the two fused cases
HAS_TILED_COPY = tuple(k for k, v in CASES.items() if v[0] in ("tiled", "pieces", "all-remainder"))
CHUNK = 4096        # entries per chunk of a split row (kernels.hip: long_partial)

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _wide_lp(name, lpgen):
    base = C.case_lp(name, lpgen)
    A0 = sparse.csr_matrix(base["A"])
    m, n = A0.shape
    rp, ci = A0.indptr.astype(np.int64), A0.indices.astype(np.int64)
    rng = np.random.default_rng(7000 + list(CASES).index(name))
    facts = base["facts"]
    lens_r, lens_c = np.diff(rp), np.bincount(ci, minlength=n)
    row_free = np.ones(m, dtype=bool)
    row_free[list(facts.get("rows", {})) + list(facts.get("empty_rows", []))] = False
    col_free = np.ones(n, dtype=bool)
    col_free[list(facts.get("cols", {})) + list(facts.get("empty_cols", []))] = False
    # short rows (2..16 entries) none of whose columns is a special line, from the middle of the matrix on
    touches = np.zeros(m, dtype=bool)
    touches[np.repeat(np.arange(m), lens_r)[~col_free[ci]]] = True
    cand = np.flatnonzero(row_free & (lens_r >= 2) & (lens_r <= 16) & ~touches)
    cand = np.roll(cand, -int(np.searchsorted(cand, m // 2)))
    ones = np.flatnonzero(row_free & (lens_r == 1) & ~touches)
    keep = np.ones(len(ci), dtype=bool)
    if len(ones):
        zero_row, rest = int(ones[len(ones) // 2]), cand
    else:
        zero_row, rest = int(cand[0]), cand[1:]
        keep[rp[zero_row] + 1:rp[zero_row + 1]] = False      # cut down to its first entry
    z2, z3, tiny_row = (int(r) for r in rest[:3])
    rows_of = np.repeat(np.arange(m), lens_r)[keep]
    ci = ci[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows_of, minlength=m))]).astype(np.int64)
    lens_r, lens_c = np.diff(rp), np.bincount(ci, minlength=n)
    special_rows = np.zeros(m, dtype=bool)
    special_rows[[zero_row, z2, z3, tiny_row]] = True
    col_hits = np.bincount(ci, weights=special_rows[rows_of].astype(float), minlength=n) > 0
    cols = np.flatnonzero(col_free & (lens_c >= 2) & (lens_c <= 16) & ~col_hits)
    big_col = int(cols[np.searchsorted(cols, n // 2) % len(cols)])
    val = rng.normal(size=len(ci)) * 10.0 ** rng.uniform(-6, 6, size=len(ci))
    assert (val != 0).all()
    zeros = [int(rp[zero_row]), int(rp[z2]), int(rp[z3] + 1)]
    val[zeros] = 0.0
    val[rp[tiny_row]:rp[tiny_row + 1]] *= 1e-40
    val[ci == big_col] *= 1e35
    A = sparse.csr_matrix((val, ci.astype(np.int32), rp.astype(np.int32)), shape=(m, n))
    lp = C.all_bounds_lp(A, 300 + list(CASES).index(name))
    assert len(lp["values"]) == len(val) and np.array_equal(lp["values"], val) and np.array_equal(lp["rowptr"], rp)   # stored zeros kept
    lp["facts"] = dict(facts, zero_row=zero_row, zero_rows=[zero_row, z2, z3], zeros=zeros, tiny_row=tiny_row, big_col=big_col)
    return lp


def case_lp(name, law, lpgen):
    """The LP of a case under a value law (built once per process; callers leave it unchanged)."""
    name = PATTERN.get(name, name)
    if law == "general":
        return C.case_lp(name, lpgen)
    assert law == "wide", law
    return _cached(("lp", name), lambda: _wide_lp(name, lpgen))


def pattern_T(name, law, lpgen):
    lp = case_lp(name, law, lpgen)
    return _cached(("T", PATTERN.get(name, name), law), lambda: R.transpose_pattern(lp["m"], lp["n"], lp["rowptr"], lp["colind"]))


def reference(name, law, lpgen, drop=None):
    """scaleref.cr_reference of a case's LP (once per process; values only where an entry is dropped)."""
    lp = case_lp(name, law, lpgen)
    return _cached(("ref", PATTERN.get(name, name), law, drop),
                   lambda: R.cr_reference(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], pattern_T(name, law, lpgen), drop=drop,
                                          with_bounds=drop is None))


def drops(name, law, lpgen):
    """{label: index of a stored entry of A} for the sensitivity checks: the entry with the largest |term| (the last pass of the
    reference) of the longest row, of the LAST CHUNK of a split row where the case has one (the 4097th entry of the 4097-entry
    row is that chunk's only one), and of a short row next to the middle of the matrix."""
    lp = case_lp(name, law, lpgen)
    rp = np.asarray(lp["rowptr"], np.int64)
    lens = np.diff(rp)
    term = np.asarray(reference(name, law, lpgen)["term"], np.float64)
    best = lambda lo, hi: int(lo + np.argmax(term[lo:hi]))
    i = int(np.argmax(lens))
    out = {"longest row (%d entries)" % lens[i]: best(rp[i], rp[i + 1])}
    split = np.flatnonzero(lens > CHUNK)
    if len(split):
        i = int(split[np.argmin(lens[split])])
        out["last chunk of the %d-entry row" % lens[i]] = best(rp[i] + CHUNK * ((lens[i] - 1) // CHUNK), rp[i + 1])
    skip = list(lp["facts"].get("zero_rows", [])) + [lp["facts"][k] for k in ("tiny_row",) if k in lp["facts"]]      # (clamped: a drop does not show)
    short = np.flatnonzero((lens >= 2) & (lens <= 16) & ~np.isin(np.arange(lp["m"]), skip))
    i = int(short[np.searchsorted(short, lp["m"] // 3) % len(short)])
    out["short row (%d entries)" % lens[i]] = best(rp[i], rp[i + 1])
    return out
