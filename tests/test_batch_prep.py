"""CPU: the host side of solve_batched that needs no device (csrc/batch_prep.h), through hprlp_batched_prepare_host.

* The per-member scaling of a batch's vectors against a numpy restatement written here, bit for bit: float64 throughout, numpy's
  longdouble (the C code's 80-bit long double on this platform) for the accumulation of the two norms, and the C code's
  parentheses -- (x * cn) / b_scale is not x * (cn / b_scale), and rn / cn are no powers of two, so a reordering would show.
* The panel layout: column-major -> device panel -> column-major, the padding, and panel_index against the formula in the header
  comment of csrc/batched.hip.
* The solution map undoes the start map to within the roundings of the two.
"""
import functools

import numpy as np
import pytest

from conftest import hprlp

INF = np.inf
M, N = 5, 7
LD = np.longdouble
# (B, HPRLP_BATCH_CHUNK or None, member with c = 0 or None, member with every row side infinite or None) -> (Bp, Bc)
CASES = {
    (1, None, None, None): (1, 1),
    (1, None, 0, None): (1, 1),
    (1, None, None, 0): (1, 1),
    (3, None, 0, 1): (4, 4),        # pads to a power of two
    (64, None, 5, 9): (64, 64),     # a single chunk
    (70, 8, 3, 68): (128, 8),       # 16 chunks
    (70, None, 3, 68): (128, 64),
}


def scalings(pow2):
    rng = np.random.default_rng(11)
    if pow2:
        return 2.0 ** rng.integers(-3, 4, M), 2.0 ** rng.integers(-3, 4, N)
    return rng.uniform(0.3, 3.1, M), rng.uniform(0.3, 3.1, N)


def make_batch(B, zero_c, inf_rows):
    """Members with infinite row sides and bounds on both sides, one with c = 0, one whose row sides are all infinite."""
    rng = np.random.default_rng(100 + B)
    C = rng.normal(size=(N, B)) * 10.0 ** rng.integers(-2, 3, (N, B))
    AL = rng.normal(size=(M, B)) * 3.0
    AU = AL + np.abs(rng.normal(size=(M, B))) * 5.0
    AL[rng.random((M, B)) < 0.3] = -INF
    AU[rng.random((M, B)) < 0.3] = INF
    l = rng.normal(size=(N, B))
    u = l + np.abs(rng.normal(size=(N, B))) * 4.0
    l[rng.random((N, B)) < 0.3] = -INF
    u[rng.random((N, B)) < 0.3] = INF
    AL[0, 0], AU[1, 0], l[0, 0], u[1, 0] = -INF, INF, -INF, INF  # (whatever the draws gave)
    if zero_c is not None:
        C[:, zero_c] = 0.0
    if inf_rows is not None:
        AL[:, inf_rows], AU[:, inf_rows] = -INF, INF
    X0 = rng.normal(size=(N, B)) * 7.0
    Y0 = rng.normal(size=(M, B)) * 0.3
    return C, AL, AU, l, u, X0, Y0


def bound_norm(lo, hi):
    s = LD(0.0)
    for a, b in zip(lo, hi):
        v = max(0.0 if a == -INF else abs(a), 0.0 if b == INF else abs(b))
        s += LD(v) * LD(v)
    return np.sqrt(np.float64(s))


def column_norm(x):
    s = LD(0.0)
    for v in x:
        s += LD(v) * LD(v)
    return np.sqrt(np.float64(s))


def restate(rn, cn, C, AL, AU, l, u, X0, Y0, bc):
    """What csrc/batch_prep.cpp prepare_batch / start_to_scaled / point_to_caller compute, operation for operation."""
    C, AL, AU, l, u = (np.array(a, dtype=np.float64) for a in (C, AL, AU, l, u))
    B = C.shape[1]
    cols = range(B)
    norm_b_org = np.array([1.0 + bound_norm(AL[:, k], AU[:, k]) for k in cols])
    norm_c_org = np.array([1.0 + column_norm(C[:, k]) for k in cols])
    AL, AU = AL / rn[:, None], AU / rn[:, None]
    C, l, u = C / cn[:, None], l * cn[:, None], u * cn[:, None]
    b_scale, c_scale = np.ones(B), np.ones(B)
    if bc:
        b_scale = np.array([1.0 + bound_norm(AL[:, k], AU[:, k]) for k in cols])
        c_scale = np.array([1.0 + column_norm(C[:, k]) for k in cols])
        AL, AU = AL / b_scale, AU / b_scale
        C, l, u = C / c_scale, l / b_scale, u / b_scale
    norm_b = np.array([bound_norm(AL[:, k], AU[:, k]) for k in cols])
    norm_c = np.array([column_norm(C[:, k]) for k in cols])
    AL, l = np.where(AL == -INF, -1e100, AL), np.where(l == -INF, -1e100, l)
    AU, u = np.where(AU == INF, 1e100, AU), np.where(u == INF, 1e100, u)
    sigma = np.array([norm_b[k] / norm_c[k] if norm_b[k] > 1e-8 and norm_c[k] > 1e-8 else 1.0 for k in cols])
    X0s, Y0s = (X0 * cn[:, None]) / b_scale, (Y0 * rn[:, None]) / c_scale
    return dict(C=C, AL=AL, AU=AU, l=l, u=u, b_scale=b_scale, c_scale=c_scale, norm_b=norm_b, norm_c=norm_c, norm_b_org=norm_b_org,
                norm_c_org=norm_c_org, sigma=sigma, X0=X0s, Y0=Y0s, X_back=(X0s / cn[:, None]) * b_scale,
                Y_back=(Y0s / rn[:, None]) * c_scale, z_back=(C * cn[:, None]) * c_scale)


@functools.lru_cache(maxsize=None)
def prepared(case, bc, pow2):
    """(inputs, the library's answer, the restatement) of one case; shared by the tests, which leave them alone."""
    B, chunk, zero_c, inf_rows = case
    rn, cn = scalings(pow2)
    batch = make_batch(B, zero_c, inf_rows)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("HPRLP_BATCH_CHUNK", raising=False)
        if chunk:
            mp.setenv("HPRLP_BATCH_CHUNK", str(chunk))
        got = hprlp.batched_prepare_host(rn, cn, *batch, use_bc_scaling=bc, pad=-7.5)
    return (rn, cn) + batch, got, restate(rn, cn, *batch, bc)


@pytest.mark.parametrize("bc", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_scaled_batch_equals_the_restatement_bit_for_bit(case, bc):
    _, got, ref = prepared(case, bc, False)
    for key in ("C", "AL", "AU", "l", "u") + hprlp.BATCH_SCALARS + ("X0", "Y0", "X_back", "Y_back", "z_back"):
        assert np.array_equal(got[key], ref[key]), key
    B, _, zero_c, inf_rows = case
    for k in (zero_c, inf_rows):  # the sigma = 1 branch
        if k is not None:
            assert got["sigma"][k] == 1.0 and (got["norm_c"][k] == 0.0 or got["norm_b"][k] == 0.0)
    assert (got["sigma"] != 1.0).sum() >= B - 2
    if not bc:
        assert (got["b_scale"] == 1.0).all() and (got["c_scale"] == 1.0).all()
    # infinite sides and bounds are +-1e100 and nothing else is
    (_, _, _, AL, AU, l, u, _, _) = prepared(case, bc, False)[0]
    for key, src, big in (("AL", AL, -1e100), ("AU", AU, 1e100), ("l", l, -1e100), ("u", u, 1e100)):
        assert np.array_equal(got[key] == big, np.isinf(src)) and np.isinf(src).any() and np.isfinite(got[key]).all(), key


@pytest.mark.parametrize("case", CASES)
def test_panel_round_trip_padding_and_index(case):
    _, got, _ = prepared(case, True, False)
    B = case[0]
    Bp, Bc = CASES[case]
    assert (got["Bp"], got["Bc"]) == (Bp, Bc)
    panel, C = got["panel"], got["C"]
    assert panel.shape == (N * Bp,)
    assert np.array_equal(got["panel_back"], C)
    i, k = np.meshgrid(np.arange(N), np.arange(B), indexing="ij")
    index = ((k // Bc) * N + i) * Bc + k % Bc  # csrc/batched.hip, "Layout": element (row j, problem k) of a panel of `rows` rows
    assert np.array_equal(got["panel_index"], index)
    assert np.array_equal(panel[index], C)
    padding = np.ones(N * Bp, dtype=bool)
    padding[index.ravel()] = False
    assert padding.sum() == N * (Bp - B) and (panel[padding] == -7.5).all()


@pytest.mark.parametrize("bc,pow2", [(False, True), (True, True), (True, False), (False, False)])
@pytest.mark.parametrize("case", CASES)
def test_solution_map_undoes_the_start_map(case, bc, pow2):
    (_, _, _, _, _, _, _, X0, Y0), got, _ = prepared(case, bc, pow2)
    if pow2 and not bc:  # every factor a power of two: both maps are exact
        assert np.array_equal(got["X_back"], X0) and np.array_equal(got["Y_back"], Y0)
    else:  # two roundings on the way there, two on the way back
        eps = np.finfo(np.float64).eps
        np.testing.assert_allclose(got["X_back"], X0, rtol=4 * eps, atol=0)
        np.testing.assert_allclose(got["Y_back"], Y0, rtol=4 * eps, atol=0)
