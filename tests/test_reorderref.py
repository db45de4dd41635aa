"""CPU: the host path of the locality ordering (csrc/reorder.cpp through hprlp_reorder_steps / hprlp_tiling_share /
hprlp_locality_ordering) against the rules restated in numpy (tests/reorderref.py), exactly; the reference's own invariants; and
every rule of the reference dropped in turn, which at least one case must see.  The same cases run through the device kernels in
tests/test_gpu_reorder_steps.py."""
import numpy as np
import pytest

import bench_helpers as bh
import reorderref as R
from conftest import hprlp

OUTPUTS = ("lab_r", "lab_c", "pos0_r", "pos0_c", "pos_r", "pos_c", "row_new2old", "col_new2old")
SWEEPS = (0, 1, 3)


def host_steps(c, sweeps, monkeypatch):
    monkeypatch.setenv("HPRLP_REORDER_CLUSTER", str(c["cluster"]))
    return hprlp.reorder_steps(c["m"], c["n"], c["rowptr"], c["colind"], device=False, sweeps=sweeps)


def assert_same(got, want, where, names=OUTPUTS):
    for k in names:
        assert got[k].dtype == want[k].dtype or got[k].dtype.kind == want[k].dtype.kind, (where, k)
        assert np.array_equal(got[k], want[k]), (where, k, int((got[k] != want[k]).sum()), np.flatnonzero(got[k] != want[k])[:5])


def assert_edge_features(c):
    f, rp, ci, m, n = c["facts"], c["rowptr"], c["colind"], c["m"], c["n"]
    lr, lc = np.diff(rp), np.bincount(ci, minlength=n)
    assert m - 1 in f["empty_rows"] and n - 1 in f["empty_cols"] and f["seed_row"] in f["empty_rows"]
    assert f["seed_row"] in R.seed_rows(m, c["K"])
    assert (lr[f["empty_rows"]] == 0).all() and (lc[f["empty_cols"]] == 0).all()
    assert tuple(lr[f["long_rows"]]) == R.SPECIAL_LENGTHS and tuple(lc[f["long_cols"]]) == R.SPECIAL_LENGTHS
    rows = np.repeat(np.arange(m), lr)
    in_block = np.isin(rows, f["block_rows"])
    assert np.array_equal(in_block, np.isin(ci, f["block_cols"])) and in_block.sum() == 2 * f["B"] - 1     # joined only to each other
    assert not np.isin(f["block_rows"], R.seed_rows(m, c["K"])).any()
    u = ci[rp[f["unsorted_row"]]:rp[f["unsorted_row"] + 1]]
    assert (np.diff(u) <= 0).all() and (np.diff(u) < 0).any()
    dups = sum(int((np.diff(ci[rp[i]:rp[i + 1]]) == 0).sum()) for i in range(m))
    assert dups >= f["duplicates"]


@pytest.mark.parametrize("name", R.BAND_CASES)
def test_host_path_equals_the_restated_rules(name, monkeypatch):
    """Labels, cluster positions, positions after 0 / 1 / 3 sweeps, permutations and both tiling shares of the host path equal the
    reference's, bit for bit.  The BFS must be over within the host's 12 synchronous levels (asserted): past them the host's queue
    may break ties differently."""
    c = R.case(name, bh.gen_banded)
    if name.startswith("edges"):
        assert_edge_features(c)
    assert 100 <= c["K"] <= 1000
    for sweeps in SWEEPS:
        got = host_steps(c, sweeps, monkeypatch)
        assert got["clusters"] == c["K"] and 1 <= got["bfs_levels"] <= R.HOST_LEVELS, (got["clusters"], got["bfs_levels"])
        want = R.ordering(c["m"], c["n"], c["rowptr"], c["colind"], c["K"], got, sweeps)
        assert want["bfs_levels"] == got["bfs_levels"]
        assert_same(got, want, "%s, %d sweeps" % (name, sweeps))
        assert got["share_before"] == want["share_before"] and got["share_after"] == want["share_after"]
        assert got["components"] >= 1
    if name.startswith("edges"):
        f = c["facts"]
        assert (got["lab_r"][f["block_rows"]] == -1).all() and (got["lab_c"][f["block_cols"]] == -1).all()
        assert (got["lab_r"][f["empty_rows"]] == -1).sum() >= len(f["empty_rows"]) - 1     # (the empty seed row keeps its own label)
        assert got["lab_r"][f["seed_row"]] >= 0
        assert (got["lab_r"][f["long_rows"]] >= 0).all() and (got["lab_c"][f["long_cols"]] >= 0).all()


def test_locality_ordering_outputs_equal_the_reference(monkeypatch):
    """hprlp_locality_ordering (gates on): a small pattern passes the tiling test in any order, so it reports the given order's
    share -- the reference's -- and declines; with the gates out of the way (hprlp_reorder_steps, default sweeps from
    HPRLP_REORDER_SWEEPS unset = 3) the permutations are the reference's (test above)."""
    c = R.case("band", bh.gen_banded)
    monkeypatch.setenv("HPRLP_REORDER_CLUSTER", str(c["cluster"]))
    pr, pc = np.full(c["m"], -7, np.int32), np.full(c["n"], -7, np.int32)
    out = np.zeros(6)
    L = hprlp.lib()
    ip = lambda a: a.ctypes.data_as(hprlp.c_int_p)
    L.hprlp_locality_ordering.argtypes = [hprlp.C.c_int, hprlp.C.c_int] + [hprlp.c_int_p] * 4 + [hprlp.c_dbl_p]
    assert L.hprlp_locality_ordering(c["m"], c["n"], ip(c["rowptr"]), ip(c["colind"]), ip(pr), ip(pc), out.ctypes.data_as(hprlp.c_dbl_p)) == 0
    share, counts = R.tiling_share(c["m"], c["n"], c["rowptr"], c["colind"])
    assert out[0] == 0.0 and out[1] == share == 1.0 and counts.min() >= R.DENSE_MIN
    assert (pr == -7).all() and (pc == -7).all()


@pytest.mark.parametrize("perm", ["given", "swapped", "reversed"])
def test_host_tiling_share_at_the_threshold(perm):
    """(super-block, tile) pairs of 0, 1, 255, 256, 257 and thousands of entries, ragged last super-block and tile: the share counts
    exactly the pairs from 256 on -- by construction, by the reference and by the host."""
    m, n, rp, ci, counts = R.tile_count_pattern()
    pr, pc, want_counts = tile_perms(perm, m, n, counts)
    share, got_counts = R.tiling_share(m, n, rp, ci, pr, pc)
    if want_counts is not None:
        assert np.array_equal(got_counts.reshape(3, 3), want_counts)
        assert share == int(counts[counts >= 256].sum()) / int(counts.sum()) and 0.5 < share < 1.0
        assert R.tiling_share(m, n, rp, ci, pr, pc, R.Rules(dense_at_least=False))[0] < share
    assert hprlp.tiling_share(m, n, rp, ci, pr, pc, device=False) == share


def tile_perms(kind, m, n, counts):
    """None / super-blocks 0 and 1 swapped wholesale with the rows shuffled inside each and the columns shuffled inside each tile
    (the pair counts move with them) / both orders reversed (ragged boundaries move: the reference alone says what comes out)."""
    rng = np.random.default_rng(11)
    if kind == "given":
        return None, None, counts
    if kind == "reversed":
        return np.arange(m - 1, -1, -1, dtype=np.int32), np.arange(n - 1, -1, -1, dtype=np.int32), None
    blocks = [rng.permutation(np.arange(s * R.TILE_ROWS, min(m, (s + 1) * R.TILE_ROWS))) for s in range(3)]
    pr = np.concatenate([blocks[1], blocks[0], blocks[2]]).astype(np.int32)          # new -> old
    pc = np.concatenate([rng.permutation(np.arange(t * R.TILE_COLS, min(n, (t + 1) * R.TILE_COLS))) for t in range(3)]).astype(np.int32)
    return pr, pc, counts[[1, 0, 2]]


def test_reference_invariants():
    """The outputs are permutations; positions are ranks; an unlabelled component keeps its relative index order (0, 1 and 3
    sweeps: the block is bidiagonal in index order, so every centre is monotone in the index); a node without neighbours keeps
    its label and value."""
    c = R.case("edges", bh.gen_banded)
    m, n, rp, ci, K, f = c["m"], c["n"], c["rowptr"], c["colind"], c["K"], c["facts"]
    trp, tci = R.transpose_pattern(m, n, rp, ci)
    # the transpose is the pattern's: same multiset of (row, column), rows ascending inside a column
    rows = np.repeat(np.arange(m), np.diff(rp))
    cols_t = np.repeat(np.arange(n), np.diff(trp))
    assert np.array_equal(np.sort(rows * n + ci), np.sort(tci.astype(np.int64) * n + cols_t))
    assert all((np.diff(tci[trp[j]:trp[j + 1]]) >= 0).all() for j in range(0, n, 97))
    lab_r, lab_c, levels = R.labels(m, n, rp, ci, trp, tci, K)
    assert 1 <= levels <= R.HOST_LEVELS
    assert (lab_r[f["block_rows"]] == -1).all() and (lab_c[f["block_cols"]] == -1).all()
    assert lab_r.max() < K and lab_c.max() < K and (lab_r >= 0).sum() > 0.99 * m - 30
    cpos = (np.random.default_rng(1).permutation(K) + 0.5) / K
    p0r, p0c = R.start_positions(lab_r, cpos), R.start_positions(lab_c, cpos)
    assert p0r[m - 1] == (m - 0.5) / m and p0c[n - 1] == (n - 0.5) / n              # empty last row / column: own index
    for sweeps in (0, 1, 3):
        pos_r, pos_c, pr, pc = R.refine(m, n, rp, ci, trp, tci, p0r, p0c, sweeps)
        assert np.array_equal(np.sort(pr), np.arange(m)) and np.array_equal(np.sort(pc), np.arange(n))
        assert np.array_equal(pos_r[pr], (np.arange(m) + 0.5) / m) and np.array_equal(pos_c[pc], (np.arange(n) + 0.5) / n)
        r_old2new = np.empty(m, np.int64); r_old2new[pr] = np.arange(m)
        c_old2new = np.empty(n, np.int64); c_old2new[pc] = np.arange(n)
        assert (np.diff(r_old2new[f["block_rows"]]) > 0).all() and (np.diff(c_old2new[f["block_cols"]]) > 0).all(), sweeps
    # permuted copy: permuting back gives the input (values carry the entry's index)
    val = np.arange(len(ci), dtype=np.float64)
    prp, pci, pv, src = R.permuted_csr(m, n, rp, ci, val, pr, pc)
    assert np.array_equal(np.diff(prp), np.diff(rp)[pr]) and np.array_equal(pv, src.astype(np.float64))
    assert all((np.diff(pci[prp[i]:prp[i + 1]]) >= 0).all() for i in range(m))
    inv_r = np.empty(m, np.int32); inv_r[pr] = np.arange(m, dtype=np.int32)
    inv_c = np.empty(n, np.int32); inv_c[pc] = np.arange(n, dtype=np.int32)
    brp, bci, bv, _ = R.permuted_csr(m, n, prp, pci, pv, inv_r, inv_c)
    assert np.array_equal(brp, rp)
    srt = np.lexsort((np.arange(len(ci)), ci, rows))            # the input with every row's columns ascending, duplicates in order
    assert np.array_equal(bci, ci[srt]) and np.array_equal(bv, val[srt])


DROPPED = {
    "sampling len instead of 32": R.Rules(sample=10 ** 9),
    "the last labelled neighbour instead of the first": R.Rules(first_neighbour=False),
    "majority ties to the largest label": R.Rules(ties_smallest=False),
    "no trimming of the centre": R.Rules(trim=False),
    "an unstable sort on equal keys": R.Rules(stable=False),
    "ranks by a product with 1 / n": R.Rules(divide=False),
}


@pytest.mark.parametrize("rule", list(DROPPED))
def test_a_dropped_rule_is_seen(rule, monkeypatch):
    """The reference with one rule dropped differs from the host path on at least one case and output -- so the exact comparisons
    above (and the device's, tests/test_gpu_reorder_steps.py) would see a kernel that dropped it."""
    seen = []
    for name in R.BAND_CASES:
        c = R.case(name, bh.gen_banded)
        got = host_steps(c, 3, monkeypatch)
        bad = R.ordering(c["m"], c["n"], c["rowptr"], c["colind"], c["K"], got, 3, DROPPED[rule])
        seen += [(name, k) for k in OUTPUTS if not np.array_equal(got[k], bad[k])]
    assert seen, rule
    if rule == "sampling len instead of 32":
        assert all(name.startswith("edges") for name, _ in seen), seen       # only the cases with rows of more than 32 entries
    print(rule, "->", seen[:6])


def test_dropped_rules_of_the_tiling_share_and_the_permuted_copy_are_seen():
    m, n, rp, ci, counts = R.tile_count_pattern()
    assert R.tiling_share(m, n, rp, ci, rules=R.Rules(dense_at_least=False))[0] == int(counts[counts > 256].sum()) / int(counts.sum())
    assert R.tiling_share(m, n, rp, ci)[0] != R.tiling_share(m, n, rp, ci, rules=R.Rules(dense_at_least=False))[0]
    c = R.case("edges", bh.gen_banded)
    rng = np.random.default_rng(2)
    pr, pc = rng.permutation(c["m"]).astype(np.int32), rng.permutation(c["n"]).astype(np.int32)
    val = np.arange(len(c["colind"]), dtype=np.float64)
    a = R.permuted_csr(c["m"], c["n"], c["rowptr"], c["colind"], val, pr, pc)
    b = R.permuted_csr(c["m"], c["n"], c["rowptr"], c["colind"], val, pr, pc, R.Rules(stable=False))
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])      # same columns, the duplicates' values swapped
