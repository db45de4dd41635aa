"""The BATCHED infeasibility detection's ray test BY VALUE in every panel geometry (GPU): the nine device scalars per member of
kb_ray_form (six), kb_ray_col (two) and kb_ray_row (one) of hpr-lp-c_amd/csrc/batched.hip, through the max accumulators of
block_store_per_problem and the max mask of kb_finalize that only they use, behind hprlp_batched_solver_ray_step -- the loop's own
ray_step / fetch / slot reads on the panels a solve left -- against tests/evalref.py's evaluate_rays per member ON THE SOLVER'S OWN
READ-BACK panels, norms and scales, within 2 x the derived bound of that module and nothing wider.  kb_ray_product's z (the
certificates') is held to 2 x (len + 1) u sum|a_ij ys_i| per element.  The scaled shared matrix is the oracle's (Curtis-Reid off:
the device's scaling passes equal it bit for bit); the read-back norms must be its bits.

Geometries (padded_batch / choose_chunk: Bp = padded batch, Bw = chunk width; a lane follows one member, 64 / Bw rows per wave):
  B = 1, 2, 3 -> Bw = 1, 2, 4;  B = 5, 12, 24 -> Bw = 8, 16, 32;  B = 64 -> Bw = 64, one chunk each;
  B = 70 -> two chunks of 64 with 58 dead columns;  B = 130 -> three chunks;  B = 70 with HPRLP_BATCH_CHUNK = 8, 16, 32;
on the "long" matrix all of them, on "short" five.  B = 64 on "wrapped" (8203 x 8209): every row loop of the ray kernels wraps
(it does so only above 2048 x rows_per_block rows, 8192 at Bw = 64, the one width where that is reachable in seconds) and
kb_finalize adds 2048 producer blocks in 32 trips of its four load chains (2048 is a multiple of 64: no tail there); B = 64 on
"mid" (403 x 807: 101 and 202 row blocks): its four-chain loop AND its tail, each on some waves only (the small matrices have 31
and 52 row blocks at that width: the tail, and one trip of the loop on four waves).  HPRLP_BATCH_GRID caps only the half-steps' grids, not these kernels': it is
not a parameter here.

Per geometry (tests/batched_ray_cases.py has the rays and the targets; tests/test_batched_rayref.py shows on the CPU that they
keep the reference alone inside the caps):
  1. the start: a step before any stored iterate is refused; with restart it only stores, and ray_prev_x / ray_prev_y are
     X_bar / Y_bar bit for bit;
  2. random rays, another seed per member: ray_d, ray_y and the stored iterate are the numpy subtraction's bits, all fifteen numbers
     of every member are within tolerance, the evaluator with the wrong bound side is not (first member of every chunk), X_bar /
     Y_bar and the five data panels keep their bits, and ray_z is right by value for every member;
  3. frozen members: with some active[k] = 0 those members are reported as not tested and their ray_d, ray_y and stored columns
     keep their bits, the active members' numbers are those of the step with all active, bit for bit, and the padding columns of
     the raw DS / YS panels are still zero at the end;
  4. targeted rays: different members get the arg-max of a slot on different lines in one step (a solve per step: every step has
     its own bound kinds); the reference shows the line as the arg-max with the runner-up at most half of it, and the evaluator
     without that line, or without its largest entry, is farther than the tolerance from the GPU's number;
  5. later solves on the handle -- with detection, without, and with carry where nothing was written -- give the bits of a handle
     that never stepped; carry after a write of X_bar / Y_bar is refused with a message.  test_later_tensor_solves_* does the same
     for the tensor entry.

The whole module takes 16 s on one MI355X (12 s of it the first tensor test's import of torch; the "wrapped" case 1.4 s, every
other case at most 0.4 s).  Largest observed-difference / bound ratio per slot and geometry, MI355X (the tolerance is 2; the
module prints the rows, "LARGEST RATIOS"):

| geometry | DY | CD | VY | WD | YN | DN | DZ | VZ | WQ | D | V | cd | W | yn | dn | ray_z |
|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|
| long B = 1 | 0.0148 | 0.00871 | 0.492 | 0.75 | 0.492 | 0.663 | 0.0121 | 0.18 | 0.149 | 0.0116 | 0.219 | 0.00871 | 0.509 | 0.492 | 0.663 | 0.564 |
| long B = 2 | 0.0129 | 0.0132 | 0.492 | 0.654 | 0.492 | 0.654 | 0.00813 | 0.202 | 0.184 | 0.0105 | 0.219 | 0.0132 | 0.321 | 0.492 | 0.654 | 0.564 |
| long B = 3 | 0.0135 | 0.0088 | 0.487 | 0.75 | 0.362 | 0.524 | 0.0107 | 0.207 | 0.0566 | 0.011 | 0.207 | 0.0088 | 0.0566 | 0.362 | 0.524 | 0.564 |
| long B = 5 | 0.0205 | 0.0127 | 0.487 | 0.6 | 0.48 | 0.6 | 0.0121 | 0.156 | 0.149 | 0.0116 | 0.156 | 0.0127 | 0.149 | 0.48 | 0.6 | 0.564 |
| long B = 12 | 0.0181 | 0.00843 | 0.622 | 0.581 | 0.678 | 0.581 | 0.00973 | 0.207 | 0.252 | 0.0104 | 0.207 | 0.00843 | 0.252 | 0.678 | 0.581 | 0.564 |
| long B = 24 | 0.0181 | 0.00815 | 0.694 | 0.678 | 0.678 | 0.678 | 0.0135 | 0.154 | 0.178 | 0.00938 | 0.154 | 0.00815 | 0.178 | 0.678 | 0.678 | 0.564 |
| long B = 64 | 0.0189 | 0.0103 | 0.724 | 0.678 | 0.76 | 0.678 | 0.0119 | 0.154 | 0.178 | 0.0106 | 0.154 | 0.0103 | 0.178 | 0.76 | 0.678 | 0.564 |
| long B = 70 | 0.0143 | 0.0156 | 0.724 | 0.679 | 0.76 | 0.679 | 0.0119 | 0.154 | 0.214 | 0.0112 | 0.154 | 0.0156 | 0.214 | 0.76 | 0.679 | 0.564 |
| long B = 130 | 0.0144 | 0.0156 | 0.724 | 0.865 | 0.859 | 0.865 | 0.0119 | 0.167 | 0.214 | 0.0112 | 0.167 | 0.0156 | 0.214 | 0.859 | 0.865 | 0.57 |
| long B = 70, chunks of 8 | 0.0189 | 0.00463 | 0.771 | 0.679 | 0.76 | 0.726 | 0.0138 | 0.173 | 0.178 | 0.00762 | 0.173 | 0.00463 | 0.178 | 0.76 | 0.726 | 0.564 |
| long B = 70, chunks of 16 | 0.0189 | 0.00592 | 0.771 | 0.679 | 0.76 | 0.679 | 0.00883 | 0.304 | 0.209 | 0.00754 | 0.304 | 0.00592 | 0.209 | 0.76 | 0.679 | 0.564 |
| long B = 70, chunks of 32 | 0.0171 | 0.0092 | 0.771 | 0.679 | 0.76 | 0.726 | 0.012 | 0.154 | 0.214 | 0.0116 | 0.154 | 0.0092 | 0.214 | 0.76 | 0.726 | 0.564 |
| short B = 3 | 0.0131 | 0.00477 | 0.42 | 0.712 | 0.42 | 0.662 | 0.0067 | 0.21 | 0.344 | 0.00598 | 0.21 | 0.00477 | 0.371 | 0.42 | 0.662 | 0.582 |
| short B = 12 | 0.0112 | 0.00895 | 0.713 | 0.675 | 0.713 | 0.675 | 0.00706 | 0.228 | 0.344 | 0.00814 | 0.228 | 0.00895 | 0.675 | 0.713 | 0.675 | 0.582 |
| short B = 64 | 0.0148 | 0.0138 | 0.721 | 0.64 | 0.877 | 0.665 | 0.0128 | 0.256 | 0.344 | 0.00841 | 0.256 | 0.0138 | 0.631 | 0.877 | 0.665 | 0.582 |
| short B = 70 | 0.0148 | 0.00614 | 0.721 | 0.636 | 0.877 | 0.665 | 0.0128 | 0.256 | 0.344 | 0.00929 | 0.256 | 0.00614 | 0.631 | 0.877 | 0.665 | 0.582 |
| short B = 70, chunks of 16 | 0.0108 | 0.0105 | 0.721 | 0.636 | 0.877 | 0.665 | 0.0107 | 0.256 | 0.344 | 0.00857 | 0.256 | 0.0105 | 0.631 | 0.877 | 0.665 | 0.582 |
| mid B = 64 | 0.00683 | 0.00338 | 0.704 | 0.689 | 0.704 | 0.77 | 0.00384 | 0.271 | 0.223 | 0.00389 | 0.591 | 0.00338 | 0.689 | 0.704 | 0.77 | 0.614 |
| wrapped B = 64 | 0.000334 | 0.000207 | 0.704 | 0.689 | 0.831 | 0.689 | 0.000334 | 0.199 | 0.415 | 0.000246 | 0.642 | 0.000207 | 0.689 | 0.831 | 0.689 | 0.626 |
| worst | 0.0205 | 0.0156 | 0.771 | 0.865 | 0.877 | 0.865 | 0.0138 | 0.304 | 0.415 | 0.0116 | 0.642 | 0.0156 | 0.689 | 0.877 | 0.865 | 0.626 |
"""
import math

import numpy as np
import pytest

import batched_ray_cases as R
import evalref as E
from conftest import hprlp

pytestmark = pytest.mark.gpu

# (matrix, B, HPRLP_BATCH_CHUNK or 0, the chunk width that gives)
CASES = [("long", B, 0, Bw) for B, Bw in ((1, 1), (2, 2), (3, 4), (5, 8), (12, 16), (24, 32), (64, 64), (70, 64), (130, 64))]
CASES += [("long", 70, c, c) for c in (8, 16, 32)]
CASES += [("short", B, 0, Bw) for B, Bw in ((3, 4), (12, 16), (64, 64), (70, 64))] + [("short", 70, 16, 16)]
CASES += [("mid", 64, 0, 64), ("wrapped", 64, 0, 64)]
IDS = ["%s-B%d%s" % (k, B, "-CHUNK=%d" % c if c else "") for k, B, c, _ in CASES]
DATA_PANELS = ("C", "AL", "AU", "L", "U")
WRAPPED_TARGETS = 12     # of the "wrapped" case: lines 0, last, last - 1, the two around the wrap and the longest
RESULT_FIELDS = ("x", "y", "z", "iter", "primal_obj", "residuals", "gap")


def model_of(kind):
    s = R.shared(kind)
    m, n = s["m"], s["n"]
    return hprlp.Model.from_csr(m, n, s["rowptr"], s["colind"], s["values"], np.zeros(m), np.zeros(m), np.zeros(n), np.zeros(n), np.zeros(n))


def params(max_iter=25):
    return hprlp.Parameters(max_iter=max_iter, stop_tol=1e-12, check_iter=10, use_CR_scaling=False, use_presolve=False)


def solve(bs, monkeypatch, chunk, inp, detect=True, **kw):
    """one short solve: evaluations at 0, 10 and 20, so the loop itself stores an iterate and tests once"""
    with monkeypatch.context() as mp:
        if chunk:
            mp.setenv("HPRLP_BATCH_CHUNK", str(chunk))
        eps = dict(eps_primal=1e-8, eps_dual=1e-8) if detect else {}
        return bs.solve(inp["C"], inp["AL"], inp["AU"], inp["L"], inp["U"], **eps, **kw)


def same_results(a, b, label):
    assert a["status"] == b["status"], label
    for f in RESULT_FIELDS:
        assert np.array_equal(np.asarray(a[f]), np.asarray(b[f])), (label, f)


def write_rays(bs, DS, YS):
    """X_bar = stored + DS, Y_bar = stored + YS; returns the stored iterate"""
    px, py = bs.get_panel("ray_prev_x"), bs.get_panel("ray_prev_y")
    bs.set_panel("X_bar", px + DS)
    bs.set_panel("Y_bar", py + YS)
    return px, py


def read_back(bs):
    return {k: bs.get_panel(k) for k in DATA_PANELS + ("ray_d", "ray_y")}


def check_sums(got):
    for g in got:
        if g is not None:
            for a, b in (("D", g["DY"] + g["DZ"]), ("V", max(g["VY"], g["VZ"])), ("cd", g["CD"]), ("W", max(g["WD"], g["WQ"])),
                         ("yn", g["YN"]), ("dn", g["DN"])):
                assert g[a] == b, a


@pytest.mark.parametrize("kind,B,chunk,Bw", CASES, ids=IDS)
def test_batched_ray_slots_by_value_in_every_geometry(gpu, monkeypatch, kind, B, chunk, Bw):
    s = R.shared(kind)
    m, n, A, AT = s["m"], s["n"], s["A"], s["AT"]
    model = model_of(kind)
    bs = hprlp.BatchedSolver(model, params())
    base = R.base_inputs(kind, B)
    tag = "%s B %d chunk %d" % (kind, B, chunk)
    worst = {}

    def note(w):
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)

    with pytest.raises(RuntimeError, match="successful solve"):
        bs.ray_step(restart=True)
    first = solve(bs, monkeypatch, chunk, base)
    info = bs.info()
    assert (info["Bc"], info["Bp"]) == (Bw, 64 * -(-B // 64) if B > 64 else 1 << (B - 1).bit_length()), info
    norms = (bs.get_panel("row_norm"), bs.get_panel("col_norm"))
    assert np.array_equal(norms[0], s["row_norm"]) and np.array_equal(norms[1], s["col_norm"])
    scal = bs.scalars()

    # 1. the start
    with pytest.raises(RuntimeError, match="no stored iterate"):
        bs.ray_step()
    with pytest.raises(RuntimeError, match="unknown panel"):
        bs.get_panel("Z_hat")
    with pytest.raises(RuntimeError, match="cannot be written"):
        bs.set_panel("C", base["C"])
    assert bs.ray_step(restart=True) is None
    xb, yb = bs.get_panel("X_bar"), bs.get_panel("Y_bar")
    assert xb.shape == (n, B) and yb.shape == (m, B) and np.abs(xb).max() > 0 and np.abs(yb).max() > 0
    assert np.array_equal(bs.get_panel("ray_prev_x"), xb) and np.array_equal(bs.get_panel("ray_prev_y"), yb)

    def step(DS, YS, inp, label, active=None):
        """the rays written, one ray_step: the rays and the stored iterate by bits, the fifteen numbers of every tested member by
        value, X_bar / Y_bar and the data panels untouched"""
        px, py = write_rays(bs, DS, YS)
        before = {k: bs.get_panel(k) for k in DATA_PANELS + ("X_bar", "Y_bar")}
        got = bs.ray_step(active=active)
        assert got is not None and len(got) == B
        after = {k: bs.get_panel(k) for k in DATA_PANELS + ("X_bar", "Y_bar")}
        for k in before:
            assert np.array_equal(before[k], after[k]), (label, k)
        on = np.ones(B, dtype=bool) if active is None else np.asarray(active) != 0
        assert [g is not None for g in got] == list(on), label
        rd = read_back(bs)
        # one subtraction is the same bits anywhere
        assert np.array_equal(rd["ray_d"][:, on], (after["X_bar"] - px)[:, on]) and np.array_equal(rd["ray_y"][:, on], (after["Y_bar"] - py)[:, on]), label
        assert np.array_equal(bs.get_panel("ray_prev_x")[:, on], after["X_bar"][:, on]), label
        assert np.array_equal(bs.get_panel("ray_prev_y")[:, on], after["Y_bar"][:, on]), label
        check_sums(got)
        res, w = E.check_batched_rays(A, AT, rd, norms, bs.scalars(), inp, got, tag + " " + label)
        note(w)
        return got, res, rd

    # 2. random rays
    DS0, YS0 = R.random_step(kind, B)
    got_all, res, rd = step(DS0, YS0, base, "random rays")
    assert all(abs(g[k]) > 0 for g in got_all for k in ("DY", "YN", "DN", "DZ", "WQ")), tag
    for k in range(0, B, Bw):      # the first member of every chunk: a sum with the wrong bound side is seen
        inp_k, ds, ys, want, _ = res[k]
        bad = E.ratios(got_all[k], E.evaluate_rays(*inp_k, ds, ys, swap_sides=True), ("DY", "DZ", "D"))
        assert min(bad.values()) > E.TOL_FACTOR, (tag, k, bad)
    # ... and the certificates' product z = A^T ys of every member (kb_ray_product)
    z = bs.get_panel("ray_z")
    assert z.shape == (n, B)
    zmax = 0.0
    for k in range(B):
        want_z, bound = E.ray_product(AT, rd["ray_y"][:, k])
        diff = np.abs(z[:, k].astype(E.LD) - want_z)
        assert np.isfinite(z[:, k]).all() and (diff <= E.TOL_FACTOR * bound).all(), (tag, "ray_z", k, int(np.argmax(diff - E.TOL_FACTOR * bound)))
        nz = bound > 0
        zmax = max(zmax, float((diff[nz] / bound[nz]).max()))
        assert np.abs(z[:, k]).max() > 0
    note({"ray_z": zmax})

    # 3. frozen members, from the state the random step started from: X_bar / Y_bar back, a restart, the same rays
    active = R.frozen_mask(B)
    off = active == 0
    bs.set_panel("X_bar", xb)
    bs.set_panel("Y_bar", yb)
    assert bs.ray_step(restart=True) is None
    write_rays(bs, DS0, YS0)
    names = ("ray_d", "ray_y", "ray_prev_x", "ray_prev_y")
    before = {k: bs.get_panel(k) for k in names}
    got = bs.ray_step(active=active)
    assert [g is None for g in got] == list(off), tag
    for k in range(B):
        if got[k] is not None:
            assert got[k] == got_all[k], (tag, "member %d with others frozen" % k)
    after = {k: bs.get_panel(k) for k in names}
    for k in names:
        assert np.array_equal(before[k][:, off], after[k][:, off]), (tag, k)
        if k in ("ray_d", "ray_y"):
            assert np.array_equal(after[k][:, ~off], rd[k][:, ~off]), (tag, k)
    assert B < 3 or (off.any() and not off[0] and not off[B - 1])

    # 4. targeted rays: a solve per step
    for t, st in enumerate(R.targeted_steps(kind, B, Bw, WRAPPED_TARGETS if kind == "wrapped" else None)):
        solve(bs, monkeypatch, chunk, st["inputs"])
        assert bs.ray_step(restart=True) is None
        label = "targeted step %d" % t
        got, res, _ = step(st["DS"], st["YS"], st["inputs"], label)
        for k, tg in st["targets"].items():
            inp_k, ds, ys, want, _ = res[k]
            for slot, line, drop in tg:
                E.dominated(want, got[k], inp_k, ds, ys, slot, line, "%s %s member %d" % (tag, label, k), **drop)

    # the padding columns of the rays' panels were never written
    if info["Bp"] > B:
        for name, rows in (("raw:ray_d", n), ("raw:ray_y", m)):
            raw = bs.get_panel(name).reshape(info["Bp"] // Bw, rows, Bw)
            pad = np.array([k >= B for k in range(info["Bp"])]).reshape(info["Bp"] // Bw, 1, Bw)
            assert raw.shape[0] * raw.shape[2] == info["Bp"] and not (raw * pad).any(), (tag, name)
            assert np.array_equal(raw[0, :, 0], bs.get_panel(name[4:])[:, 0])

    # 5. later solves are those of a handle that never stepped; carry after a write is refused
    with pytest.raises(RuntimeError, match="written by name"):
        solve(bs, monkeypatch, chunk, base, carry=True)
    fresh = hprlp.BatchedSolver(model, params())
    ref = solve(fresh, monkeypatch, chunk, base)
    same_results(first, ref, tag + " first solve")
    same_results(solve(bs, monkeypatch, chunk, base), ref, tag + " detecting solve after steps")
    assert bs.ray_step(restart=True) is None and bs.ray_step() is not None          # (steps that write nothing: carry is allowed)
    same_results(solve(bs, monkeypatch, chunk, base, carry=True), solve(fresh, monkeypatch, chunk, base, carry=True), tag + " carry after steps")
    assert bs.ray_step(restart=True) is None
    same_results(solve(bs, monkeypatch, chunk, base, detect=False), solve(fresh, monkeypatch, chunk, base, detect=False), tag + " plain solve after a step")
    a, b = bs.info(), fresh.info()
    assert a["panel_allocations"] == b["panel_allocations"], (a, b)
    print("batched rays", tag, "LARGEST RATIOS", " | ".join("%s %.3g" % (k, worst[k]) for k in E.RAY_NAMES + ("ray_z",)))
    assert all(math.isfinite(v) and v <= E.TOL_FACTOR for v in worst.values()), worst
    bs.close(); fresh.close(); model.free()


def test_a_step_on_a_handle_that_never_detected_allocates_as_a_detecting_solve(gpu, monkeypatch):
    """The last solve ran without detection: the step allocates the detection's panels (one allocation, as a detecting solve's),
    the ray_* names are unknown before it, and the numbers are those of the same step after a detecting solve."""
    kind, B = "short", 12
    s = R.shared(kind)
    model = model_of(kind)
    base = R.base_inputs(kind, B)
    DS, YS = R.random_step(kind, B)
    out = []
    for detect in (False, True):
        bs = hprlp.BatchedSolver(model, params())
        solve(bs, monkeypatch, 0, base, detect=detect)
        allocs = bs.info()["panel_allocations"]
        if not detect:
            with pytest.raises(RuntimeError, match="does not exist"):
                bs.get_panel("ray_d")
        assert bs.ray_step(restart=True) is None
        assert bs.info()["panel_allocations"] == allocs + (0 if detect else 1)
        write_rays(bs, DS, YS)
        got = bs.ray_step()
        E.check_batched_rays(s["A"], s["AT"], read_back(bs), (bs.get_panel("row_norm"), bs.get_panel("col_norm")), bs.scalars(), base, got)
        out.append(got)
        solve(bs, monkeypatch, 0, base)
        assert bs.info()["panel_allocations"] == allocs + (0 if detect else 1)
        bs.close()
    assert out[0] == out[1]
    model.free()


@pytest.mark.parametrize("kind,B,chunk", [("long", 5, 0), ("long", 70, 16), ("short", 70, 0)])
def test_later_tensor_solves_are_those_of_a_handle_that_never_stepped(gpu, monkeypatch, kind, B, chunk):
    import torch
    model = model_of(kind)
    base = R.base_inputs(kind, B)
    dev = {k: torch.tensor(v, dtype=torch.float64, device="cuda:0") for k, v in base.items()}
    DS, YS = R.random_step(kind, B)

    def tsolve(bs, detect, **kw):
        with monkeypatch.context() as mp:
            if chunk:
                mp.setenv("HPRLP_BATCH_CHUNK", str(chunk))
            eps = dict(eps_primal=1e-8, eps_dual=1e-8) if detect else {}
            r = bs.solve_tensors(dev["C"], dev["AL"], dev["AU"], dev["L"], dev["U"], **eps, **kw)
        return dict(r, **{f: r[f].cpu().numpy() for f in ("x", "y", "z")})

    stepped, fresh = hprlp.BatchedSolver(model, params()), hprlp.BatchedSolver(model, params())
    same_results(tsolve(stepped, True), tsolve(fresh, True), "first")
    assert stepped.ray_step(restart=True) is None and stepped.ray_step() is not None
    same_results(tsolve(stepped, True, carry=True), tsolve(fresh, True, carry=True), "carry after steps without a write")
    assert stepped.ray_step(restart=True) is None
    write_rays(stepped, DS, YS)
    assert all(g is not None for g in stepped.ray_step())
    with pytest.raises(RuntimeError, match="written by name"):
        tsolve(stepped, True, carry=True)
    same_results(tsolve(stepped, True), tsolve(fresh, True), "detecting solve after a written step")
    assert stepped.ray_step(restart=True) is None
    same_results(tsolve(stepped, False), tsolve(fresh, False), "plain solve after a step")
    assert stepped.info()["graph_captures"] == fresh.info()["graph_captures"]
    stepped.close(); fresh.close(); model.free()
