"""The batches, rays and targets of the batched ray test's value checks (tests/test_gpu_batched_ray_values.py on the GPU,
tests/test_batched_rayref.py without one).  A plain module: no fixtures, no GPU.

The matrices.  "long" and "short" are matrix() / batch() of tests/test_gpu_batched_kernels.py (123 x 205 with a row of 150 entries,
a column of 90 and empty rows and columns; 121 x 207 with at most 6 entries per line and a last row and column that are not empty).
"wrapped" is 8203 x 8209 with about 3 entries per row: at a chunk width of 64 a workgroup covers 4 rows and the grid is capped at
2048 row blocks, so every row loop of the ray kernels wraps above 8192 rows and kb_finalize adds 2048 producer blocks (32 trips of
its four load chains; 2048 is a multiple of 64, so its tail loop does not run there).  "mid" is 403 x 807: 101 and 202 row blocks at
a chunk width of 64, so kb_finalize runs its four-chain loop once to three times AND its tail, on some waves only.  The small
matrices have 31 and 52 row blocks at that width (fewer at smaller ones): the tail, and one trip of the loop on four waves.

The shared matrix in scaled units is the oracle's scaling of it with zero vectors, Curtis-Reid and b / c scaling off, which the
device's passes equal bit for bit (tests/test_gpu_scaling.py; the GPU module asserts the read-back norms' bits against these).

A TARGETED step gives different members the arg-max of a slot on different lines.  A member's target is of one of two types:
  form: boosted random rays (evalref.boosted) put |d| and d (DN, WD) on column j and |y| and y (YN, VY) on row i, four times the
        rest.  The lines are taken as they are: an empty line has an element like any other in kb_ray_form.
  spmm: ys = -(column j of the scaled A) and ds = +(row i) put z_j = cn_j c_scale sum a^2 (VZ) and q_i = rn_i b_scale sum a^2 (WQ)
        on lines that store an entry (the nearest such line).
The lines: 0, the last, one inside the last ragged row block, with more than 8192 lines the two around the wrap, the longest (the
150-entry row, the 90-entry column), lines of 1 to 5 entries (the tail of the four-in-flight loop; where a matrix has no line of
that length, one with the same length modulo 4), the neighbours of an empty line.  The members: first the first and the last
lane of the first chunk, member B - 1 (the last before the padding) and the first member of a second chunk, then the others in
order; a batch with fewer members than targets takes several steps.
The bound kind a target needs comes through that step's batch input: -inf for the lower bound of a spmm column (z_j > 0 counts as a
violation), a finite upper side for a spmm row and a finite upper bound for a form column, no lower side for a form row.  A line
that shares entries with a short spmm line can come close to it: such rivals (above 0.4 of the target on the scaled matrix; the
member's positive scales cancel in the comparison) get both column bounds finite resp. a free row for that member and step.  Every
step therefore has its own input, and the GPU module solves once per step; no iterate is compared there.
"""
import functools

import numpy as np

import evalref as E
from oracle import oracle as O

INF = np.inf
KINDS = ("long", "short", "mid", "wrapped")
GENERATED = {"mid": (403, 807, 814), "wrapped": (8203, 8209, 813)}
GENERATED_B = 64
WRAP = 8192          # rows above which a row loop wraps at a chunk width of 64: 2048 row blocks x 4 rows


def _generated(kind):
    from scipy import sparse
    m, n, seed = GENERATED[kind]
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.repeat(np.arange(m), 2), rng.integers(0, m, size=n)])
    cols = np.concatenate([rng.integers(0, n, size=2 * m), np.arange(n)])      # two per row and one per column: about 3 per row
    A = sparse.csr_matrix((rng.normal(size=len(rows)), (rows, cols)), shape=(m, n))
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    B = GENERATED_B
    ck = rng.integers(0, 4, size=(n, B))            # columns: 0 both finite, 1 lower only, 2 upper only, 3 free
    L = np.where((ck == 2) | (ck == 3), -INF, -rng.uniform(0.5, 1.5, size=(n, B)))
    U = np.where((ck == 1) | (ck == 3), INF, rng.uniform(0.5, 2.0, size=(n, B)))
    rk = rng.integers(0, 5, size=(m, B))            # rows: 0 both finite, 1 lower only, 2 upper only, 3 free, 4 equality
    mid = 0.2 * rng.normal(size=(m, B))
    AL = np.where((rk == 2) | (rk == 3), -INF, np.where(rk == 4, mid, mid - np.abs(rng.normal(size=(m, B)))))
    AU = np.where((rk == 1) | (rk == 3), INF, np.where(rk == 4, mid, mid + np.abs(rng.normal(size=(m, B)))))
    return dict(m=m, n=n, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), values=A.data.copy(),
                C=rng.normal(size=(n, B)), AL=AL, AU=AU, L=L, U=U)


@functools.lru_cache(maxsize=None)
def shared(kind):
    """The matrix, its largest batch (C, AL, AU, L, U: (rows, members)) and the scaled shared matrix: A, AT = (rowptr, colind,
    values), row_norm, col_norm.  Built once per process and left unchanged."""
    if kind in GENERATED:
        b = _generated(kind)
    else:
        import test_gpu_batched_kernels as K
        b = dict(K.batch(kind))
    m, n = b["m"], b["n"]
    sl = O.ScaledLP(m, n, b["rowptr"], b["colind"], b["values"], np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(n),
                    O.Params.default(use_CR_scaling=0, use_bc_scaling=0))
    b.update(A=(sl.Arp, sl.Aci, sl.Av), AT=(sl.ATrp, sl.ATci, sl.ATv), row_norm=sl.row_norm, col_norm=sl.col_norm)
    return b


def base_inputs(kind, B):
    s = shared(kind)
    return {k: s[k][:, :B].copy() for k in ("C", "AL", "AU", "L", "U")}


def member_seed(k, salt=0):
    return 1000 * (salt + 1) + k


def random_step(kind, B, salt=0):
    """(DS (n, B), YS (m, B)): evalref.random_rays with a different seed per member"""
    s = shared(kind)
    rays = [E.random_rays(s["m"], s["n"], member_seed(k, salt)) for k in range(B)]
    return np.stack([r[0] for r in rays], axis=1), np.stack([r[1] for r in rays], axis=1)


def lines_of_interest(lens):
    """the target lines of the module docstring for lines of these lengths, in that order, each once"""
    lens = np.asarray(lens)
    last = len(lens) - 1
    want = [0, last, last - 1] + ([WRAP - 1, WRAP] if last >= WRAP else []) + [int(np.argmax(lens))]
    for length in range(1, 6):
        idx = np.flatnonzero(lens == length)
        if not len(idx):
            idx = np.flatnonzero((lens > 0) & (lens % 4 == length % 4))
        idx = [int(i) for i in idx if int(i) not in want]
        if idx:
            want.append(idx[0])
    empty = np.flatnonzero(lens == 0)
    if len(empty):
        want += [int(empty[0]) - 1, int(empty[0]) + 1]
    out = []
    for k in want:
        k = min(max(k, 0), last)
        if k not in out:
            out.append(k)
    return out


def nonempty_near(lens, k):
    """the line nearest to k (k itself first, then k + 1, k - 1, ...) that stores an entry"""
    for step in range(len(lens)):
        for cand in (k + step, k - step):
            if 0 <= cand < len(lens) and lens[cand] > 0:
                return int(cand)
    raise AssertionError("no stored entry")


def member_order(B, Bw):
    """the first and the last lane of the first chunk, member B - 1, the first member of a second chunk, then the rest"""
    special = []
    for k in (0, min(Bw, B) - 1, B - 1, Bw):
        if 0 <= k < B and k not in special:
            special.append(k)
    return special + [k for k in range(B) if k not in special]


def targets_of(kind):
    """[(type, column j, row i)]: form and spmm alternate over the lines of interest"""
    s = shared(kind)
    clen, rlen = np.diff(s["AT"][0]), np.diff(s["A"][0])
    cols, rows = lines_of_interest(clen), lines_of_interest(rlen)
    out = []
    for t in range(max(len(cols), len(rows))):
        j, i = cols[t % len(cols)], rows[t % len(rows)]
        out.append(("form", j, i))
        out.append(("spmm", nonempty_near(clen, j), nonempty_near(rlen, i)))
    return out


def _finite_above(hi, lo):
    """hi where it is finite, else a finite value above lo"""
    return hi if np.isfinite(hi) else (lo + 1.0 if np.isfinite(lo) else 1.0)


def _finite_below(lo, hi):
    return lo if np.isfinite(lo) else (hi - 1.0 if np.isfinite(hi) else -1.0)


def targeted_steps(kind, B, Bw, limit=None):
    """The targeted steps of a batch of B members in chunks of Bw: a list of dicts with `inputs` (that step's C, AL, AU, L, U), DS,
    YS (members without a target: random rays) and `targets` {member: [(slot, line, drop)]}, drop = {} or the drop_A / drop_AT
    of evalref.evaluate_rays that leaves out the line's largest entry.  limit: only the first `limit` targets."""
    s = shared(kind)
    m, n, A, AT, rn, cn = s["m"], s["n"], s["A"], s["AT"], s["row_norm"], s["col_norm"]
    todo = targets_of(kind)[:limit]
    order = member_order(B, Bw)
    steps = []
    for first in range(0, len(todo), B):
        inp = base_inputs(kind, B)
        DS, YS = random_step(kind, B, salt=1 + first)
        targets = {}
        for pos, (typ, j, i) in enumerate(todo[first:first + B]):
            k = order[pos]
            AL, AU, L, U = (inp[name][:, k] for name in ("AL", "AU", "L", "U"))      # (views: the step's input changes)
            if typ == "form":
                DS[:, k], YS[:, k] = E.boosted(DS[:, k], cn, j, 1.0), E.boosted(YS[:, k], rn, i, 1.0)
                U[j] = _finite_above(U[j], L[j])
                AL[i] = -INF
                targets[k] = [("WD", j, {}), ("DN", j, {}), ("VY", i, {}), ("YN", i, {})]
                continue
            DS[:, k], YS[:, k] = E.line_of(A, i, n, 1.0), E.line_of(AT, j, m, -1.0)
            L[j] = -INF
            AU[i] = _finite_above(AU[i], AL[i])
            z = -cn * E._row_sums(AT, YS[:, k], None, np.float64)[0]
            q = rn * E._row_sums(A, DS[:, k], None, np.float64)[0]
            fin = np.isfinite
            vz = np.where((z > 0) & ~fin(L), z, np.where((z < 0) & ~fin(U), -z, 0.0))
            wq = np.maximum(np.where(fin(AL), -q, 0.0), np.where(fin(AU), q, 0.0))
            assert vz[j] > 0 and wq[i] > 0, (kind, k, j, i)
            rc, rr = np.flatnonzero(vz > 0.4 * vz[j]), np.flatnonzero(wq > 0.4 * wq[i])
            rc, rr = rc[rc != j], rr[rr != i]
            assert len(rc) <= 16 and len(rr) <= 16, (kind, k, j, i, len(rc), len(rr))
            for c in rc:
                L[c], U[c] = _finite_below(L[c], U[c]), _finite_above(U[c], L[c])
            AL[rr], AU[rr] = -INF, INF
            targets[k] = [("VZ", j, dict(drop_AT=E.largest_entry(AT, j))), ("WQ", i, dict(drop_A=E.largest_entry(A, i)))]
        steps.append(dict(inputs=inp, DS=DS, YS=YS, targets=targets))
    return steps


def frozen_mask(B):
    """the members a frozen step leaves out: every third one from member 1, never the first and never the last"""
    active = np.ones(B, dtype=np.intc)
    active[1:B - 1:3] = 0
    return active
