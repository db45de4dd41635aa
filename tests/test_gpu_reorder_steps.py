"""GPU: the device kernels of the locality ordering (csrc/reorder_dev.hip) step by step at small shapes, every comparison exact:
k_pull_labels / k_majority (labels), k_cluster_edge_keys + the run lengths through cluster_order and k_cluster_pos (positions before
refinement), k_centre_sweep + the rank normalisation (positions after 0, 1 and 3 sweeps), the final argsorts, k_tile_keys /
k_sum_dense_runs (tiling share) and k_entry_keys / k_permuted_entries (the permuted copy) -- against the rules restated in numpy
(tests/reorderref.py) and against the host path (csrc/reorder.cpp), which tests/test_reorderref.py holds to the same reference
without a GPU.  Host and device owe the same bits wherever the Voronoi BFS is over within the host's 12 synchronous levels; the
grid case is past them and is compared with the reference alone."""
import numpy as np
import pytest

import bench_helpers as bh
import reorderref as R
from conftest import hprlp
from test_reorderref import OUTPUTS, SWEEPS, assert_edge_features, assert_same, tile_perms

pytestmark = pytest.mark.gpu


def steps(c, device, sweeps, monkeypatch):
    monkeypatch.setenv("HPRLP_REORDER_CLUSTER", str(c["cluster"]))
    return hprlp.reorder_steps(c["m"], c["n"], c["rowptr"], c["colind"], device=device, sweeps=sweeps)


@pytest.mark.parametrize("name", R.BAND_CASES)
def test_device_ordering_equals_reference_and_host(gpu, name, monkeypatch):
    """9001 x 12 007 and 12 007 x 9001 permuted bands with far entries (no multiple of 256, m != n, a few hundred clusters), plain
    and with empty rows / columns (the last ones, a seed row), lines of 1, 32, 33, 64 and 300 entries (the sampled paths), a block
    without a seed, duplicates and an unsorted row.  Device = reference = host for the labels, the positions before refinement and
    after 0, 1 and 3 sweeps, the permutations and both tiling shares."""
    c = R.case(name, bh.gen_banded)
    if name.startswith("edges"):
        assert_edge_features(c)
    for sweeps in SWEEPS:
        dev = steps(c, True, sweeps, monkeypatch)
        assert dev["clusters"] == c["K"] and 100 <= c["K"] <= 1000
        assert 1 <= dev["bfs_levels"] <= R.HOST_LEVELS, dev["bfs_levels"]      # the condition of the host comparison: asserted, not skipped on
        want = R.ordering(c["m"], c["n"], c["rowptr"], c["colind"], c["K"], dev, sweeps)
        assert want["bfs_levels"] == dev["bfs_levels"]
        assert_same(dev, want, "%s, %d sweeps, device against the reference" % (name, sweeps))
        assert dev["share_before"] == want["share_before"] and dev["share_after"] == want["share_after"]
        host = steps(c, False, sweeps, monkeypatch)
        assert_same(dev, host, "%s, %d sweeps, device against the host" % (name, sweeps))
        for k in ("clusters", "components", "bfs_levels", "share_before", "share_after"):
            assert dev[k] == host[k], (k, dev[k], host[k])
    if name.startswith("edges"):
        f = c["facts"]
        assert (dev["lab_r"][f["block_rows"]] == -1).all() and (dev["lab_c"][f["block_cols"]] == -1).all()


def test_device_ordering_on_a_grid_past_the_hosts_levels(gpu, monkeypatch):
    """A permuted five-point grid of 150 x 150 with three clusters: the device needs more than 12 levels (asserted), where the host
    finishes with a queue and may break ties differently -- the one permitted difference.  Device against the reference only."""
    c = R.case("grid", bh.gen_banded)
    assert c["K"] == 3
    for sweeps in (0, 3):
        dev = steps(c, True, sweeps, monkeypatch)
        assert dev["bfs_levels"] > R.HOST_LEVELS, dev["bfs_levels"]
        want = R.ordering(c["m"], c["n"], c["rowptr"], c["colind"], c["K"], dev, sweeps)
        assert want["bfs_levels"] == dev["bfs_levels"]
        assert_same(dev, want, "grid, %d sweeps" % sweeps)
        assert dev["share_before"] == want["share_before"] and dev["share_after"] == want["share_after"]
        assert (dev["lab_r"] >= 0).all() and (dev["lab_c"] >= 0).all()


@pytest.mark.parametrize("perm", ["given", "swapped", "reversed"])
def test_device_tiling_share_at_the_threshold(gpu, perm):
    """20 000 x 5000, 3 super-blocks x 3 tiles with a ragged last of each, pairs of 0, 1, 255, 256, 257 and thousands of entries:
    device, host and reference give the same double, with and without permutations."""
    m, n, rp, ci, counts = R.tile_count_pattern()
    pr, pc, want_counts = tile_perms(perm, m, n, counts)
    share, _ = R.tiling_share(m, n, rp, ci, pr, pc)
    if want_counts is not None:
        assert share == int(counts[counts >= 256].sum()) / int(counts.sum())
    dev = hprlp.tiling_share(m, n, rp, ci, pr, pc, device=True)
    host = hprlp.tiling_share(m, n, rp, ci, pr, pc, device=False)
    assert dev == share and host == share, (dev, host, share)
    if want_counts is not None:       # (a pair of exactly 256 entries is in play: `>` instead of `>=` would give another double)
        assert R.tiling_share(m, n, rp, ci, pr, pc, R.Rules(dense_at_least=False))[0] != share


def _entries(m, n, per_row, seed):
    """m rows of per_row entries with duplicates and unsorted columns; values = the entry's index (every value distinct)."""
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, n, size=m * per_row).astype(np.int32)
    ci[1::per_row] = ci[0::per_row]                                   # a duplicate in every row
    rp = (np.arange(m + 1) * per_row).astype(np.int32)
    return rp, ci, np.arange(m * per_row, dtype=np.float64)


@pytest.mark.parametrize("m", [4096, 4097, 1])
def test_device_permuted_copy(gpu, m):
    """device_permute_csr at the row_bits boundary (m = 4096: 12 bits, 4097: 13, 1: the minimum): the three arrays equal the
    reference's (rows in the new order, a row's entries by new column, duplicates in their old order -- the values are the entry
    indices, so a swapped pair of duplicates is seen), and permuting back gives the input."""
    n = 5003
    rp, ci, val = _entries(m, n, 6, 40 + m)
    rng = np.random.default_rng(m)
    pr, pc = rng.permutation(m).astype(np.int32), rng.permutation(n).astype(np.int32)
    want = R.permuted_csr(m, n, rp, ci, val, pr, pc)
    got = hprlp.permute_csr_device(m, n, rp, ci, val, pr, pc)
    for g, w, what in zip(got, want, ("rowptr", "colind", "values")):
        assert np.array_equal(g, w), (what, int((g != w).sum()))
    assert not np.array_equal(want[2], R.permuted_csr(m, n, rp, ci, val, pr, pc, R.Rules(stable=False))[2])
    inv_r = np.empty(m, np.int32); inv_r[pr] = np.arange(m, dtype=np.int32)
    inv_c = np.empty(n, np.int32); inv_c[pc] = np.arange(n, dtype=np.int32)
    back = hprlp.permute_csr_device(m, n, *got, inv_r, inv_c)
    rows = np.repeat(np.arange(m), np.diff(rp))
    srt = np.lexsort((np.arange(len(ci)), ci, rows))                  # the input, every row's columns ascending, duplicates in order
    assert np.array_equal(back[0], rp) and np.array_equal(back[1], ci[srt]) and np.array_equal(back[2], val[srt])


def test_device_permuted_copy_of_the_edge_pattern(gpu, monkeypatch):
    """The permuted copy of the edge-feature pattern (empty rows, a row of 300, duplicates, the unsorted row) under the ordering the
    device itself finds for it."""
    c = R.case("edges", bh.gen_banded)
    dev = steps(c, True, 3, monkeypatch)
    val = np.arange(len(c["colind"]), dtype=np.float64)
    want = R.permuted_csr(c["m"], c["n"], c["rowptr"], c["colind"], val, dev["row_new2old"], dev["col_new2old"])
    got = hprlp.permute_csr_device(c["m"], c["n"], c["rowptr"], c["colind"], val, dev["row_new2old"], dev["col_new2old"])
    for g, w, what in zip(got, want, ("rowptr", "colind", "values")):
        assert np.array_equal(g, w), (what, int((g != w).sum()))
