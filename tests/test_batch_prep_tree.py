"""CPU: the "tree" norm rule of the device-resident batches (csrc/batch_prep.h, DESIGN.md "Device-resident batches"), through
hprlp_batched_prepare_host_rule -- the host twin of kb_data_in / kb_data_bc, which the GPU tests compare the kernels with.

* Rule 1 against a numpy restatement written here, bit for bit: every term v * v rounded to float64 before it is added, the lane
  sums of a segment in increasing row, the fold by halving strides, the segment sums in increasing segment; the rest is
  prepare_batch's order of operations as tests/test_batch_prep.py restates it.
* Rule 1 against rule 0 (the reference's long double sums) within a bound that follows from the two orders (below).
* Rule 0 through the new entry is the old entry, bit for bit.

The bound.  u = 2^-53.  All terms are non-negative, so a sum's relative error is at most u times the number of roundings on the
longest path from a term to the total (first order).  Rule 1: one for the term, SEG / LANES - 1 lane additions (the first one adds
to 0.0: exact), log2(LANES) folds, nseg - 1 segment additions; the root halves that and adds one, "1 +" adds one more.  Rule 0:
(rows + 1) * 2^-64 for the long double sum, one for the cast, the root and "1 +" as before -- 10.5 u at the longest vector here.
The two together stay below BOUND(nseg) = (SEG / LANES + log2(LANES) + nseg + 3) u for norm_b_org, norm_c_org, b_scale and
c_scale, which the two rules compute from the same values.  norm_b and norm_c are computed from vectors that were divided by the
two rules' own scales, so their worst case is that bound twice over; they are held to the single BOUND all the same (the sums
are nowhere near their worst case).  A scaled entry is one division by such a scale, rounded once under either rule:
BOUND + 2 u; entries that no scale touches (AL, AU, C, l, u without use_bc_scaling) are equal.  sigma is a quotient of two
norms: 2 BOUND + 2 u.
"""
import functools
import math

import numpy as np
import pytest

from conftest import hprlp

INF = np.inf
SEG, LANES = hprlp.NORM_SEG, hprlp.NORM_LANES
U = 2.0 ** -53
# (m, n): every length of the issue's list as a row count and as a column count
SHAPES = [(1, LANES - 1), (LANES - 1, 1), (SEG, SEG + 1), (SEG + 1, 2 * SEG + 37), (2 * SEG + 37, SEG)]
BATCHES = [1, 3, 33]
VECTORS = ("C", "AL", "AU", "l", "u")
NORMS = ("b_scale", "c_scale", "norm_b", "norm_c", "norm_b_org", "norm_c_org")


def bound(rows):
    nseg = -(-rows // SEG)
    return (SEG // LANES + int(math.log2(LANES)) + nseg + 3) * U


@functools.lru_cache(maxsize=None)
def scalings(m, n):
    rng = np.random.default_rng(11)
    return rng.uniform(0.3, 3.1, m), rng.uniform(0.3, 3.1, n)


@functools.lru_cache(maxsize=None)
def make_batch(m, n, B):
    """Infinite row sides and bounds of both signs in every member; the last member has C = 0 (sigma 1)."""
    rng = np.random.default_rng(1000 * B + m % 997)
    Cm = rng.normal(size=(n, B)) * 10.0 ** rng.integers(-2, 3, (n, B))
    AL = rng.normal(size=(m, B)) * 3.0
    AU = AL + np.abs(rng.normal(size=(m, B))) * 5.0
    l = rng.normal(size=(n, B))
    u = l + np.abs(rng.normal(size=(n, B))) * 4.0
    AL[rng.random((m, B)) < 0.3] = -INF
    AU[rng.random((m, B)) < 0.3] = INF
    l[rng.random((n, B)) < 0.3] = -INF
    u[rng.random((n, B)) < 0.3] = INF
    AL[0, :], u[0, :] = -INF, INF  # (whatever the draws gave; a row side infinite on one side keeps the other finite side's value)
    if m > 1:
        AU[1, :] = INF
    if n > 1:
        l[1, :] = -INF
    Cm[:, B - 1] = 0.0
    return Cm, AL, AU, l, u


def tree_sum(T):
    """The tree rule for the columns of T (rows x B) of terms, every operation a float64 one."""
    rows, B = T.shape
    total = np.zeros(B)
    for s in range(-(-rows // SEG)):
        seg = T[s * SEG:min(rows, (s + 1) * SEG)]
        a = np.zeros((LANES, B))
        for r in range(0, len(seg), LANES):      # lane j: rows s * SEG + j, + LANES, ... in increasing order
            part = seg[r:r + LANES]
            a[:len(part)] = a[:len(part)] + part
        stride = LANES // 2
        while stride >= 1:                       # a[j] += a[j + stride]
            a[:stride] = a[:stride] + a[stride:2 * stride]
            stride //= 2
        total = total + a[0]                     # segments in increasing s
    return total


def bound_norm(AL, AU):
    lo = np.where(AL == -INF, 0.0, np.abs(AL))
    hi = np.where(AU == INF, 0.0, np.abs(AU))
    v = np.maximum(lo, hi)
    return np.sqrt(tree_sum(v * v))


def column_norm(X):
    return np.sqrt(tree_sum(X * X))


def restate(rn, cn, Cm, AL, AU, l, u, bc):
    """prepare_batch (csrc/batch_prep.cpp) with the tree rule, operation for operation."""
    B = Cm.shape[1]
    norm_b_org, norm_c_org = 1.0 + bound_norm(AL, AU), 1.0 + column_norm(Cm)
    AL, AU = AL / rn[:, None], AU / rn[:, None]
    Cm, l, u = Cm / cn[:, None], l * cn[:, None], u * cn[:, None]
    b_scale, c_scale = np.ones(B), np.ones(B)
    if bc:
        b_scale, c_scale = 1.0 + bound_norm(AL, AU), 1.0 + column_norm(Cm)
        AL, AU = AL / b_scale, AU / b_scale
        Cm, l, u = Cm / c_scale, l / b_scale, u / b_scale
    norm_b, norm_c = bound_norm(AL, AU), column_norm(Cm)
    AL, l = np.where(AL == -INF, -1e100, AL), np.where(l == -INF, -1e100, l)
    AU, u = np.where(AU == INF, 1e100, AU), np.where(u == INF, 1e100, u)
    ok = (norm_b > 1e-8) & (norm_c > 1e-8)
    sigma = np.where(ok, norm_b / np.where(ok, norm_c, 1.0), 1.0)
    return dict(C=Cm, AL=AL, AU=AU, l=l, u=u, b_scale=b_scale, c_scale=c_scale, norm_b=norm_b, norm_c=norm_c, norm_b_org=norm_b_org,
                norm_c_org=norm_c_org, sigma=sigma)


@functools.lru_cache(maxsize=None)
def prepared(shape, B, bc, rule):
    """The library's answer for one case under one rule (None: the entry without a rule); shared, left alone by the tests."""
    rn, cn = scalings(*shape)
    kw = {} if rule is None else dict(norm_rule=rule)
    return hprlp.batched_prepare_host(rn, cn, *make_batch(*shape, B), use_bc_scaling=bc, **kw)


@pytest.mark.parametrize("bc", [True, False])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_tree_rule_equals_the_restatement_bit_for_bit(shape, B, bc):
    got = prepared(shape, B, bc, 1)
    ref = restate(*scalings(*shape), *make_batch(*shape, B), bc)
    for key in hprlp.BATCH_SCALARS + VECTORS:
        bad = np.argwhere(got[key] != ref[key])
        assert np.array_equal(got[key], ref[key]), (key, "first difference at", bad[0].tolist(), "of", len(bad))
    # the cases the issue names are in the batch: infinite entries of both signs, and the member with C = 0
    _, AL, AU, l, u = make_batch(*shape, B)
    for key, src, big in (("AL", AL, -1e100), ("AU", AU, 1e100), ("l", l, -1e100), ("u", u, 1e100)):
        if src.shape[0] > 1:
            assert np.isinf(src).any(), key
        assert np.array_equal(got[key] == big, np.isinf(src)) and np.isfinite(got[key]).all(), key
    assert got["sigma"][B - 1] == 1.0 and got["norm_c"][B - 1] == 0.0
    if not bc:
        assert (got["b_scale"] == 1.0).all() and (got["c_scale"] == 1.0).all()


@pytest.mark.parametrize("bc", [True, False])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_tree_rule_against_the_long_double_rule(shape, B, bc):
    m, n = shape
    tree, ref = prepared(shape, B, bc, 1), prepared(shape, B, bc, 0)
    rows_of = dict(b_scale=m, norm_b=m, norm_b_org=m, AL=m, AU=m, c_scale=n, norm_c=n, norm_c_org=n, C=n)
    worst = {}
    for key in NORMS:
        rel = np.abs(tree[key] - ref[key]) / np.maximum(np.abs(ref[key]), np.finfo(float).tiny)
        worst[key] = rel.max() / U
        assert (rel <= bound(rows_of[key])).all(), (key, rel.max() / U, "u; bound", bound(rows_of[key]) / U, "u")
    # a scaled entry: one division by a scale that differs by at most BOUND, rounded once on either side
    scale_rows = dict(AL=m, AU=m, l=m, u=m, C=n)  # l, u are divided by b_scale (m rows), C by c_scale (n rows)
    for key in VECTORS:
        a, b = tree[key], ref[key]
        if not bc:
            assert np.array_equal(a, b), key
            continue
        tol = bound(scale_rows[key]) + 2 * U
        rel = np.abs(a - b) / np.maximum(np.abs(b), np.finfo(float).tiny)
        assert (rel <= tol).all(), (key, rel.max() / U, "u; bound", tol / U, "u")
        assert np.array_equal(np.abs(a) == 1e100, np.abs(b) == 1e100), key
    tol = bound(m) + bound(n) + 2 * U
    rel = np.abs(tree["sigma"] - ref["sigma"]) / np.abs(ref["sigma"])
    assert (rel <= tol).all(), ("sigma", rel.max() / U, "u")
    print("shape", shape, "B", B, "bc", bc, "worst difference of the norms in u:", {k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("bc", [True, False])
@pytest.mark.parametrize("shape,B", [(SHAPES[0], 3), (SHAPES[3], 3), (SHAPES[4], 33)])
def test_rule_0_is_the_entry_without_a_rule(shape, B, bc):
    old, new = prepared(shape, B, bc, None), prepared(shape, B, bc, 0)
    rn, cn = scalings(*shape)
    L = hprlp.lib()
    raw = {k: np.zeros_like(v) for k, v in old.items() if k in VECTORS}
    scal = np.zeros((7, B))
    P = lambda a: a.ctypes.data_as(hprlp.c_dbl_p)
    keep = [np.asfortranarray(a) for a in make_batch(*shape, B)]
    o = hprlp.CBatchedPrepared(scalars=P(scal), **{k: P(v) for k, v in raw.items()})
    # ... and through the new symbol itself with rule 0 (the wrapper calls the old symbol for rule 0)
    rc = L.hprlp_batched_prepare_host_rule(shape[0], shape[1], B, P(rn), P(cn), *[P(a) for a in keep], None,
                                           None, int(bc), 0, o)
    assert rc == 0, hprlp.last_error()
    for key in VECTORS:
        assert np.array_equal(old[key], new[key]) and np.array_equal(old[key], raw[key]), key
    for i, key in enumerate(hprlp.BATCH_SCALARS):
        assert np.array_equal(old[key], new[key]) and np.array_equal(old[key], scal[i]), key


def test_an_unknown_rule_is_refused():
    rn, cn = scalings(*SHAPES[0])
    with pytest.raises(RuntimeError, match="norm rule"):
        hprlp.batched_prepare_host(rn, cn, *make_batch(*SHAPES[0], 1), norm_rule=2)
