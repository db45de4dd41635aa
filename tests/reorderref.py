"""The rules of the set-up time locality ordering (csrc/reorder.cpp's header, csrc/reorder_dev.hip) restated in plain numpy: what
tests/test_reorderref.py holds the host path against and tests/test_gpu_reorder_steps.py / test_gpu_reorder_small.py the device
kernels.  Whole-array operations on padded sample tables, no shared code with the library.  The spectral order of the clusters
(cluster_order) is NOT restated: host and device call the same function, and the reference takes the cluster positions from the
side under test (cluster_positions_of) after checking that they are one value per label.

Every rule that a kernel could drop has a switch here (Rules), so the tests can show that a dropped rule is seen.
A plain module: no fixtures; the test patterns are built here too (cases), once per process."""
import numpy as np

TILE_ROWS, TILE_COLS, DENSE_MIN = 8192, 2048, 256
HOST_LEVELS = 12          # the host's synchronous BFS levels; after them it finishes with a queue (may break ties differently)


class Rules:
    """The rules as stated (defaults) or with one of them dropped."""

    def __init__(self, sample=32, first_neighbour=True, ties_smallest=True, trim=True, stable=True, dense_at_least=True, divide=True):
        self.sample = sample                    # at most this many evenly sampled neighbours
        self.first_neighbour = first_neighbour  # BFS: the FIRST labelled neighbour in adjacency order (else the last)
        self.ties_smallest = ties_smallest      # majority: ties to the smallest label (else the largest)
        self.trim = trim                        # centre: mean of [take // 5, take - take // 5) (else of everything)
        self.stable = stable                    # sorts keep equal keys in index order (else reverse them)
        self.dense_at_least = dense_at_least    # a tile counts from 256 entries on (else from 257)
        self.divide = divide                    # ranks (i + 0.5) / n (else (i + 0.5) * (1 / n))


STATED = Rules()


def transpose_pattern(m, n, rp, ci):
    """Pattern of A^T, stable in row order."""
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    trp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return trp, rows[order].astype(np.int32)


def cluster_count(m, n, per_cluster=16384):
    per_cluster = max(64, int(per_cluster))
    return int(max(2, min(65536, m, (m + n) // per_cluster + 1)))


def seed_rows(m, K):
    return (np.arange(K, dtype=np.int64) * m) // K


def _pick_in_rows(mask, xp, last=False):
    """Per row of the CSR pointer xp: index of the first (last) entry with mask set, -1 where there is none."""
    nnz = len(mask)
    lens = np.diff(xp)
    rows = np.repeat(np.arange(len(lens)), lens)
    out = np.full(len(lens), -1, np.int64)
    hit = np.flatnonzero(mask)
    if last:
        out[rows[hit]] = hit                    # (ascending: the last assignment of a row wins)
    else:
        out[rows[hit[::-1]]] = hit[::-1]
    assert nnz == xp[-1]
    return out


def pull_labels(xp, xi, src, dst, rules=STATED):
    """An unlabelled node of dst takes the label of its first labelled neighbour (adjacency order) in src.  Returns the number of
    nodes that changed."""
    at = _pick_in_rows(src[xi] >= 0, xp, last=not rules.first_neighbour)
    take = (dst < 0) & (at >= 0)
    dst[take] = src[xi[at[take]]]
    return int(take.sum())


def voronoi_labels(m, n, rp, ci, trp, tci, K, rules=STATED, max_levels=None):
    """Level-synchronous multi-source BFS from the seed rows k * m // K: columns pull from rows, then rows from the columns just
    labelled, until a level changes nothing.  Returns (lab_r, lab_c, levels run, the last one -- which changed nothing -- included)."""
    lab_r, lab_c = np.full(m, -1, np.int32), np.full(n, -1, np.int32)
    lab_r[seed_rows(m, K)] = np.arange(K, dtype=np.int32)
    levels = 0
    while max_levels is None or levels < max_levels:
        ch = pull_labels(trp, tci, lab_r, lab_c, rules)
        ch += pull_labels(rp, ci, lab_c, lab_r, rules)
        levels += 1
        if ch == 0:
            break
    return lab_r, lab_c, levels


def _samples(xp, xi, rows, width, sample):
    """Table (len(rows), width) of the sampled entry indices k0 + q * len // want, want = min(len, sample); -1 past want."""
    k0 = xp[rows].astype(np.int64)
    ln = (xp[rows + 1] - xp[rows]).astype(np.int64)
    want = np.minimum(ln, sample)
    q = np.arange(width, dtype=np.int64)[None, :]
    idx = k0[:, None] + (q * ln[:, None]) // np.maximum(want, 1)[:, None]
    return np.where(q < want[:, None], idx, -1), want


def _row_groups(xp, sample):
    """Rows by the width their sample table needs: the short ones together, the (few) long ones at their own width."""
    ln = np.diff(xp)
    short = np.flatnonzero(ln <= 32)
    long_ = np.flatnonzero(ln > 32)
    groups = [(short, 32)] if len(short) else []
    if len(long_):
        groups.append((long_, int(min(sample, ln[long_].max()))))
    return groups


def majority(xp, xi, src, own, rules=STATED):
    """The most frequent label among at most 32 evenly sampled neighbours, ties to the smallest; without a labelled neighbour the
    node keeps its own label."""
    out = own.copy()
    big = np.iinfo(np.int64).max
    for rows, width in _row_groups(xp, rules.sample):
        idx, _ = _samples(xp, xi, rows, width, rules.sample)
        lab = np.where(idx >= 0, src[xi[np.maximum(idx, 0)]], -1).astype(np.int64)
        lab = np.sort(np.where(lab >= 0, lab, big), axis=1)                    # ascending, the invalid ones last
        if not rules.ties_smallest:
            lab = np.where(lab == big, -1, lab)
            lab = -np.sort(-lab, axis=1)                                       # descending: the largest label first
            lab = np.where(lab < 0, big, lab)
        votes = (lab[:, :, None] == lab[:, None, :]).sum(axis=2)
        votes = np.where(lab == big, 0, votes)
        best = np.argmax(votes, axis=1)                                        # the first maximum
        some = votes.max(axis=1) > 0
        out[rows[some]] = lab[np.flatnonzero(some), best[some]].astype(own.dtype)
    return out


def majority_rounds(rp, ci, trp, tci, lab_r, lab_c, rules=STATED, rounds=2):
    for _ in range(rounds):
        lab_c = majority(trp, tci, lab_r, lab_c, rules)
        lab_r = majority(rp, ci, lab_c, lab_r, rules)
    return lab_r, lab_c


def labels(m, n, rp, ci, trp, tci, K, rules=STATED):
    """(lab_r, lab_c, BFS levels) after the two majority rounds; -1 = unlabelled."""
    lab_r, lab_c, levels = voronoi_labels(m, n, rp, ci, trp, tci, K, rules)
    lab_r, lab_c = majority_rounds(rp, ci, trp, tci, lab_r, lab_c, rules)
    return lab_r, lab_c, levels


def cluster_positions_of(lab, pos0, K):
    """The position of every cluster as the side under test assigned it (NaN for a cluster without nodes here); asserts that it is
    one value per label and a rank (q + 0.5) / K."""
    cpos = np.full(K, np.nan)
    seen = lab >= 0
    cpos[lab[seen]] = pos0[seen]
    assert np.array_equal(cpos[lab[seen]], pos0[seen]), "two nodes of one cluster at different positions"
    have = cpos[~np.isnan(cpos)]
    q = np.rint(have * K - 0.5)
    assert np.array_equal((q + 0.5) / K, have) and len(np.unique(q)) == len(q) and q.min() >= 0 and q.max() < K
    return cpos


def start_positions(lab, cpos):
    """A node starts at its cluster's position; an unlabelled one keeps its own relative index (i + 0.5) / count."""
    count = len(lab)
    own = (np.arange(count, dtype=np.float64) + 0.5) / count
    return np.where(lab >= 0, cpos[np.maximum(lab, 0)], own)


def _argsort(keys, rules):
    if rules.stable:
        return np.argsort(keys, kind="stable")
    n = len(keys)
    return (n - 1 - np.argsort(keys[::-1], kind="stable"))       # equal keys in descending index order


def rank_normalise(pos, rules=STATED):
    n = len(pos)
    order = _argsort(pos, rules)
    out = np.empty(n)
    i = np.arange(n, dtype=np.float64)
    out[order] = (i + 0.5) / float(n) if rules.divide else (i + 0.5) * (1.0 / float(n))
    return out, order


def centre_sweep(xp, xi, src, own, rules=STATED):
    """Robust centre of src over at most 32 evenly sampled neighbours: ascending sort, mean of [take // 5, take - take // 5) summed
    left to right; a node without neighbours keeps its value."""
    out = own.copy()
    for rows, width in _row_groups(xp, rules.sample):
        idx, take = _samples(xp, xi, rows, width, rules.sample)
        v = np.sort(np.where(idx >= 0, src[xi[np.maximum(idx, 0)]], np.inf), axis=1)
        lo = take // 5 if rules.trim else np.zeros_like(take)
        hi = take - lo
        total = np.zeros(len(rows))
        for q in range(width):                                     # left to right, one addition at a time
            inside = (q >= lo) & (q < hi)
            total = np.where(inside, total + np.where(inside, v[:, q], 0.0), total)
        some = take > 0
        out[rows[some]] = total[some] / (hi[some] - lo[some]).astype(np.float64)
    return out


def refine(m, n, rp, ci, trp, tci, pos0_r, pos0_c, sweeps, rules=STATED):
    """Ranks of pos_r; `sweeps` x (columns from rows, ranks, rows from columns, ranks); the permutations are the stable argsorts.
    Returns (pos_r, pos_c, row_new2old, col_new2old)."""
    pos_r, _ = rank_normalise(pos0_r, rules)
    pos_c = pos0_c.copy()
    for _ in range(sweeps):
        pos_c, _ = rank_normalise(centre_sweep(trp, tci, pos_r, pos_c, rules), rules)
        pos_r, _ = rank_normalise(centre_sweep(rp, ci, pos_c, pos_r, rules), rules)
    if sweeps <= 0:
        pos_c, _ = rank_normalise(pos_c, rules)
    return pos_r, pos_c, _argsort(pos_r, rules).astype(np.int32), _argsort(pos_c, rules).astype(np.int32)


def tiling_share(m, n, rp, ci, row_new2old=None, col_new2old=None, rules=STATED):
    """Entries in (row // 8192, column // 2048) pairs holding at least 256 entries, divided by nnz."""
    nnz = int(rp[m])
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    cols = ci.astype(np.int64)
    if row_new2old is not None:
        r_old2new = np.empty(m, np.int64); r_old2new[row_new2old] = np.arange(m)
        c_old2new = np.empty(n, np.int64); c_old2new[col_new2old] = np.arange(n)
        rows, cols = r_old2new[rows], c_old2new[cols]
    ntile = (n + TILE_COLS - 1) // TILE_COLS
    counts = np.bincount((rows // TILE_ROWS) * ntile + cols // TILE_COLS)
    dense = counts >= DENSE_MIN if rules.dense_at_least else counts > DENSE_MIN
    return int(counts[dense].sum()) / nnz, counts


def permuted_csr(m, n, rp, ci, val, row_new2old, col_new2old, rules=STATED):
    """P A Q: rows in the new order, the entries of a row by new column, duplicates in their old order.  Returns (rowptr, colind,
    values, source entry of every new entry)."""
    r_old2new = np.empty(m, np.int64); r_old2new[row_new2old] = np.arange(m)
    c_old2new = np.empty(n, np.int64); c_old2new[col_new2old] = np.arange(n)
    rows = r_old2new[np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))]
    cols = c_old2new[ci]
    k = np.arange(len(ci), dtype=np.int64)
    order = np.lexsort((k if rules.stable else -k, cols, rows))
    new_rp = np.concatenate([[0], np.cumsum(np.diff(rp)[row_new2old])]).astype(np.int32)
    return new_rp, cols[order].astype(np.int32), np.asarray(val)[order], order


def ordering(m, n, rp, ci, K, cpos_from, sweeps, rules=STATED):
    """The whole method but the spectral order.  cpos_from: dict with lab_r, lab_c, pos0_r, pos0_c of the side under test (only
    the position of every cluster is taken from it).  Returns a dict shaped like hprlp.reorder_steps()."""
    trp, tci = transpose_pattern(m, n, rp, ci)
    lab_r, lab_c, levels = labels(m, n, rp, ci, trp, tci, K, rules)
    cpos = np.full(K, np.nan)
    for lab, pos0 in ((cpos_from["lab_r"], cpos_from["pos0_r"]), (cpos_from["lab_c"], cpos_from["pos0_c"])):
        part = cluster_positions_of(lab, pos0, K)
        both = ~np.isnan(part) & ~np.isnan(cpos)
        assert np.array_equal(part[both], cpos[both]), "rows and columns of one cluster at different positions"
        cpos = np.where(np.isnan(cpos), part, cpos)
    pos0_r, pos0_c = start_positions(lab_r, cpos), start_positions(lab_c, cpos)
    pos_r, pos_c, pr, pc = refine(m, n, rp, ci, trp, tci, pos0_r, pos0_c, sweeps, rules)
    return dict(lab_r=lab_r, lab_c=lab_c, pos0_r=pos0_r, pos0_c=pos0_c, pos_r=pos_r, pos_c=pos_c, row_new2old=pr, col_new2old=pc,
                clusters=K, bfs_levels=levels, share_before=tiling_share(m, n, rp, ci, rules=rules)[0],
                share_after=tiling_share(m, n, rp, ci, pr, pc, rules)[0])


# ---- the test patterns ------------------------------------------------------------------------------------------------------------
CLUSTER = 64            # HPRLP_REORDER_CLUSTER of the band cases: a few hundred clusters at these shapes
SPECIAL_LENGTHS = (1, 32, 33, 64, 300)
_cache = {}


def _csr_of(m, r, c):
    """CSR of the entries in the order given (stable by row: duplicates and the order inside a row are kept)."""
    order = np.argsort(r, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int32)
    return rp, c[order].astype(np.int32)


def permuted_band(m, n, per_row, seed, gen_banded):
    """A band with far entries (bench.py's generator) under random row and column numberings; columns ascending inside a row."""
    rp, ci, _ = gen_banded(m, n, per_row, max(n // 40, 8), seed)
    rng = np.random.default_rng(seed)
    pr, pc = rng.permutation(m), rng.permutation(n)
    r = pr[np.repeat(np.arange(m), np.diff(rp))]
    c = pc[ci]
    order = np.lexsort((c, r))
    return r[order], c[order]


def with_edge_features(m, n, r, c, seed, K):
    """The band's entries with: empty rows and columns (the last ones and a seed row among them), rows and columns of 1, 32, 33, 64
    and 300 entries, a block of rows and columns joined only to each other that holds no seed, duplicate entries, one row with
    descending columns.  Returns (r, c, facts)."""
    rng = np.random.default_rng(seed + 1000)
    seeds = seed_rows(m, K)
    free_r = np.setdiff1d(np.arange(m - 1), seeds)
    pick_r = rng.choice(free_r, size=2 + 5 + 20 + 1, replace=False)
    pick_c = rng.choice(n - 1, size=2 + 5 + 20, replace=False)
    empty_r = np.concatenate([[m - 1, seeds[K // 3]], pick_r[:2]])
    empty_c = np.concatenate([[n - 1], pick_c[:2]])
    long_r, long_c = pick_r[2:7], pick_c[2:7]
    block_r, block_c = np.sort(pick_r[7:27]), np.sort(pick_c[7:27])
    unsorted_row = int(pick_r[27])
    gone_r = np.concatenate([empty_r, long_r, block_r])
    gone_c = np.concatenate([empty_c, long_c, block_c])
    keep = ~np.isin(r, gone_r) & ~np.isin(c, gone_c)
    r, c = r[keep], c[keep]
    plain_r = np.setdiff1d(np.arange(m), np.concatenate([gone_r, [unsorted_row]]))
    plain_c = np.setdiff1d(np.arange(n), gone_c)
    add_r, add_c = [], []
    for j, L in zip(long_c, SPECIAL_LENGTHS):
        add_r.append(rng.choice(plain_r, size=L, replace=False)); add_c.append(np.full(L, j))
    for i, L in zip(long_r, SPECIAL_LENGTHS):
        add_r.append(np.full(L, i)); add_c.append(rng.choice(plain_c, size=L, replace=False))
    B = len(block_r)                      # bidiagonal: row q holds columns q and q + 1, the last row its own column alone
    add_r += [block_r, block_r[:-1]]; add_c += [block_c, block_c[1:]]
    dup = rng.choice(np.flatnonzero(np.isin(r, plain_r)), size=60, replace=False)
    add_r.append(r[dup]); add_c.append(c[dup])
    r, c = np.concatenate([r] + add_r), np.concatenate([c] + add_c)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    at = np.flatnonzero(r == unsorted_row)
    assert len(at) >= 3 and len(np.unique(c[at])) >= 3
    c[at] = c[at][::-1]
    facts = dict(empty_rows=empty_r, empty_cols=empty_c, long_rows=long_r, long_cols=long_c, block_rows=block_r, block_cols=block_c,
                 unsorted_row=unsorted_row, seed_row=int(seeds[K // 3]), duplicates=len(dup), B=B)
    return r, c, facts


def case(name, gen_banded):
    """name -> dict(m, n, rowptr, colind, K, cluster (the hook's value), facts).  Built once per process; callers leave it unchanged.
    band / band-T: 9001 x 12 007 and 12 007 x 9001, 8 per row; edges / edges-T: the same with the edge features; grid: a permuted
    five-point grid of 150 x 150 with three clusters (more than 12 BFS levels)."""
    if name in _cache:
        return _cache[name]
    facts = {}
    if name == "grid":
        g = 150
        m = n = g * g
        idx = np.arange(n).reshape(g, g)
        nb = [idx, np.roll(idx, 1, 0), np.roll(idx, -1, 0), np.roll(idx, 1, 1), np.roll(idx, -1, 1)]
        rng = np.random.default_rng(5)
        pr, pc = rng.permutation(m), rng.permutation(n)
        r = pr[np.concatenate([idx.ravel()] * 5)]
        c = pc[np.concatenate([x.ravel() for x in nb])]
        order = np.lexsort((c, r))
        r, c = r[order], c[order]
        cluster = m                       # (m + n) // m + 1 = 3 clusters
    else:
        m, n = (12007, 9001) if name.endswith("-T") else (9001, 12007)
        cluster = CLUSTER
        r, c = permuted_band(m, n, 8, 17 if name.endswith("-T") else 16, gen_banded)
        if name.startswith("edges"):
            r, c, facts = with_edge_features(m, n, r, c, 3, cluster_count(m, n, cluster))
    rp, ci = _csr_of(m, r, c)
    out = dict(name=name, m=m, n=n, rowptr=rp, colind=ci, K=cluster_count(m, n, cluster), cluster=cluster, facts=facts)
    _cache[name] = out
    return out


BAND_CASES = ("band", "band-T", "edges", "edges-T")


def tile_count_pattern(seed=7):
    """20 000 x 5000: 3 super-blocks x 3 tiles with a ragged last of each; entries per (super-block, tile) pair set by construction
    to 0, 1, 255, 256, 257 and some thousands.  Returns (m, n, rowptr, colind, counts (3 x 3))."""
    m, n = 20000, 5000
    counts = np.array([[0, 1, 255], [256, 257, 3000], [5000, 256, 255]])
    rng = np.random.default_rng(seed)
    rs, cs = [], []
    for sb in range(3):
        r0, r1 = sb * TILE_ROWS, min(m, (sb + 1) * TILE_ROWS)
        for t in range(3):
            c0, c1 = t * TILE_COLS, min(n, (t + 1) * TILE_COLS)
            k = int(counts[sb, t])
            rs.append(rng.integers(r0, r1, size=k)); cs.append(rng.integers(c0, c1, size=k))
    # the corners of the ragged last super-block and tile are hit
    rs[-1][0], cs[-1][0] = m - 1, n - 1
    r, c = np.concatenate(rs), np.concatenate(cs)
    order = np.lexsort((c, r))
    rp, ci = _csr_of(m, r[order], c[order])
    return m, n, rp, ci, counts
