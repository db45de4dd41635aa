"""The inputs of the batched ray test's value checks (tests/batched_ray_cases.py) on the CPU: they keep the reference ALONE inside
the caps that tests/test_gpu_batched_ray_values.py holds the GPU to.  On the "long" and "short" matrices, with every member's
data scaled by hprlp.batched_prepare_host (the host code of solve_batched) and the shared norms of the oracle's scaling
(Curtis-Reid off):
  * evaluate_rays_f64 in numpy's order, in reversed sequential order and in a pairwise tree order is within the bound of
    evaluate_rays for every member of the B = 130 batch, and with the wrong bound side it is not;
  * for every targeted step of every panel geometry of the GPU module the chosen line is the arg-max with the runner-up at most
    half of it, and the left-out line and the dropped entry are outside 2 x bound;
  * the +-1e100 <-> +-inf mapping of evalref.check_batched_rays rejects a panel with a finite value where the caller passed an
    infinity, and the reverse."""
import numpy as np
import pytest

import batched_ray_cases as R
import evalref as E
from conftest import hprlp

KINDS = ("long", "short")
# (B, chunk width) of the GPU module's geometries: one chunk below 64, chunks of 64 from there, HPRLP_BATCH_CHUNK = 8, 16, 32
GEOMETRIES = [(1, 1), (2, 2), (3, 4), (5, 8), (12, 16), (24, 32), (64, 64), (70, 64), (130, 64), (70, 8), (70, 16), (70, 32)]
_cache = {}


def prepared(kind, inputs):
    """(panels with +-inf restored, norms, scalars) of a batch input through the host side of solve_batched"""
    s = R.shared(kind)
    p = hprlp.batched_prepare_host(s["row_norm"], s["col_norm"], inputs["C"], inputs["AL"], inputs["AU"], inputs["L"], inputs["U"])
    panels = dict(C=p["C"], AL=p["AL"], AU=p["AU"], L=p["l"], U=p["u"])
    for name in E.BOUND_PANELS:
        panels[name] = E.panel_bounds_to_inf(panels[name], inputs[name], name)
    return panels, (s["row_norm"], s["col_norm"]), dict(b_scale=p["b_scale"], c_scale=p["c_scale"])


def whole_batch(kind):
    if kind not in _cache:
        B = R.shared(kind)["C"].shape[1]
        _cache[kind] = (B, prepared(kind, R.base_inputs(kind, B)), R.random_step(kind, B))
    return _cache[kind]


def _sequential_reversed(p):
    return np.cumsum(p[::-1])[-1] if len(p) else 0.0


def _tree(p):
    p = np.asarray(p, np.float64)
    if not len(p):
        return 0.0
    while len(p) > 1:
        if len(p) % 2:
            p = np.append(p, 0.0)
        p = p[0::2] + p[1::2]
    return p[0]


def _row_sums_by(total):
    def row_sums(csr, v, drop):
        rp, ci, val = csr
        p = np.asarray(val, np.float64) * np.asarray(v, np.float64)[ci]
        return np.array([total(p[rp[i]:rp[i + 1]]) for i in range(len(rp) - 1)])
    return row_sums


@pytest.mark.parametrize("kind", KINDS)
def test_fp64_in_three_orders_is_within_bounds_for_every_member_and_the_wrong_side_is_not(kind):
    s = R.shared(kind)
    B, (panels, norms, scalars), (DS, YS) = whole_batch(kind)
    assert B == 130
    worst = {}
    for k in range(B):
        inp = E.batched_member_inputs(s["A"], s["AT"], panels, norms, scalars, k)
        ds, ys = DS[:, k], YS[:, k]
        want = E.evaluate_rays(*inp, ds, ys)
        for order, kw in (("numpy", {}), ("reversed", dict(row_sums=_row_sums_by(_sequential_reversed), total=_sequential_reversed)),
                          ("tree", dict(row_sums=_row_sums_by(_tree), total=_tree))):
            r = E.ratios(E.evaluate_rays_f64(*inp, ds, ys, **kw), want, E.RAY_NAMES)
            assert E.all_within(r), (kind, k, order, r)
            for name, v in r.items():
                worst[name] = max(worst.get(name, 0.0), v)
        bad = E.ratios(E.evaluate_rays_f64(*inp, ds, ys, swap_sides=True), want, ("DY", "DZ", "D"))
        assert min(bad.values()) > E.TOL_FACTOR, (kind, k, bad)
    print(kind, "largest ratios", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("kind", KINDS)
def test_every_bound_kind_meets_both_signs_in_the_batch(kind):
    """over the members, every row and every column has a finite and an infinite side on either side, and the random rays have
    exact zeros: the branches of the kernels are all taken somewhere on every line"""
    s = R.shared(kind)
    B, (panels, _, _), (DS, YS) = whole_batch(kind)
    fin = np.isfinite
    for name in E.BOUND_PANELS:
        assert fin(panels[name]).any(axis=1).all() and (~fin(panels[name])).any(axis=1).all(), name
    assert (DS == 0).sum() >= DS.size // 16 and (YS == 0).sum() >= YS.size // 16
    assert len({DS[:, k].tobytes() for k in range(B)}) == B     # a different seed per member


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,Bw", GEOMETRIES)
def test_targeted_lines_dominate_and_their_faults_are_outside_the_bound(kind, B, Bw):
    s = R.shared(kind)
    todo = R.targets_of(kind)
    steps = R.targeted_steps(kind, B, Bw)
    assert sum(len(st["targets"]) for st in steps) == len(todo) and len(steps) == -(-len(todo) // B)
    order = R.member_order(B, Bw)
    assert order[0] == 0 and order[:4].count(B - 1) == 1 and (Bw >= B or Bw in order[:4]) and sorted(order) == list(range(B))
    seen = set()
    for st in steps:
        panels, norms, scalars = prepared(kind, st["inputs"])
        for k, tg in st["targets"].items():
            inp = E.batched_member_inputs(s["A"], s["AT"], panels, norms, scalars, k)
            ds, ys = st["DS"][:, k], st["YS"][:, k]
            want = E.evaluate_rays(*inp, ds, ys)
            got = E.evaluate_rays_f64(*inp, ds, ys)
            assert E.all_within(E.ratios(got, want, E.RAY_NAMES))
            for slot, line, drop in tg:
                E.dominated(want, got, inp, ds, ys, slot, line, "%s B %d member %d" % (kind, B, k), **drop)
                seen.add((slot, line))
    # every maximum slot is targeted at line 0 and at the last line that can hold it
    rl, cl = np.diff(s["A"][0]), np.diff(s["AT"][0])
    for slot in ("WD", "DN"):
        assert {(slot, 0), (slot, s["n"] - 1)} <= seen
    for slot in ("VY", "YN"):
        assert {(slot, 0), (slot, s["m"] - 1)} <= seen
    assert {("VZ", R.nonempty_near(cl, 0)), ("VZ", R.nonempty_near(cl, s["n"] - 1)), ("VZ", int(np.argmax(cl)))} <= seen
    assert {("WQ", R.nonempty_near(rl, 0)), ("WQ", R.nonempty_near(rl, s["m"] - 1)), ("WQ", int(np.argmax(rl)))} <= seen


def test_the_lines_of_interest_are_what_the_docstring_says():
    s = R.shared("long")
    rl, cl = np.diff(s["A"][0]), np.diff(s["AT"][0])
    rows, cols = R.lines_of_interest(rl), R.lines_of_interest(cl)
    assert rows[:4] == [0, 122, 121, 17] and cols[:4] == [0, 204, 203, 101] and rl[17] >= 150 and cl[101] >= 90
    assert {59, 61} <= set(rows) and {32, 34} <= set(cols)                       # the neighbours of the empty row 60 / column 33
    for lens, lines in ((rl, rows), (cl, cols)):
        assert {int(lens[k]) % 4 for k in lines if lens[k] > 0} == {0, 1, 2, 3}  # every tail of the four-in-flight loop
    s = R.shared("short")
    rl, cl = np.diff(s["A"][0]), np.diff(s["AT"][0])
    for lens in (rl, cl):
        have = {int(lens[k]) for k in R.lines_of_interest(lens)}
        assert set(range(1, 6)) & set(int(v) for v in lens) <= have              # every length from 1 to 5 that the matrix has
    assert R.lines_of_interest(np.ones(R.WRAP + 9, dtype=int))[:5] == [0, R.WRAP + 8, R.WRAP + 7, R.WRAP - 1, R.WRAP]


@pytest.mark.parametrize("kind", ["mid", "wrapped"])
def test_targeted_lines_dominate_on_the_generated_matrices(kind):
    """the B = 64 batch of the two generated matrices, the targets the GPU module uses"""
    s = R.shared(kind)
    assert s["m"] % 4 and s["n"] % 4 and (kind != "wrapped" or min(s["m"], s["n"]) > R.WRAP)
    assert kind != "wrapped" or 2.5 <= len(s["values"]) / s["m"] <= 3.5
    (st,) = R.targeted_steps(kind, R.GENERATED_B, 64, 12 if kind == "wrapped" else None)
    panels, norms, scalars = prepared(kind, st["inputs"])
    lines = set()
    for k, tg in st["targets"].items():
        inp = E.batched_member_inputs(s["A"], s["AT"], panels, norms, scalars, k)
        ds, ys = st["DS"][:, k], st["YS"][:, k]
        want = E.evaluate_rays(*inp, ds, ys)
        got = E.evaluate_rays_f64(*inp, ds, ys)
        for slot, line, drop in tg:
            E.dominated(want, got, inp, ds, ys, slot, line, "%s member %d" % (kind, k), **drop)
            lines.add(line)
    if kind == "wrapped":
        assert {0, R.WRAP - 1, R.WRAP, s["m"] - 1, s["n"] - 1} <= lines


def test_the_infinity_mapping_rejects_a_wrong_panel():
    caller = np.array([[1.0, np.inf], [-np.inf, 2.0]])
    good = np.array([[0.5, E.K_INF], [-E.K_INF, 0.25]])
    out = E.panel_bounds_to_inf(good, caller)
    assert np.array_equal(out, np.array([[0.5, np.inf], [-np.inf, 0.25]]))
    for i, j, value in ((0, 1, 3.0), (0, 1, 0.999 * E.K_INF), (0, 1, -E.K_INF), (0, 0, E.K_INF), (1, 1, -E.K_INF), (1, 0, E.K_INF),
                        (0, 0, np.inf), (0, 0, np.nan)):
        bad = good.copy()
        bad[i, j] = value
        with pytest.raises(AssertionError):
            E.panel_bounds_to_inf(bad, caller)
    # through check_batched_rays: a finite bound where the caller passed an infinity fails before anything is evaluated
    s = R.shared("short")
    inputs = R.base_inputs("short", 3)
    panels, norms, scalars = prepared("short", inputs)
    DS, YS = R.random_step("short", 3)
    back = lambda p: np.where(p == np.inf, E.K_INF, np.where(p == -np.inf, -E.K_INF, p))
    read = dict(panels, ray_d=DS, ray_y=YS, **{name: back(panels[name]) for name in E.BOUND_PANELS})
    got = [E.evaluate_rays_f64(*E.batched_member_inputs(s["A"], s["AT"], panels, norms, scalars, k), DS[:, k], YS[:, k]) for k in range(3)]
    res, worst = E.check_batched_rays(s["A"], s["AT"], read, norms, scalars, inputs, got)
    assert len(res) == 3 and set(worst) == set(E.RAY_NAMES)
    assert E.check_batched_rays(s["A"], s["AT"], read, norms, scalars, inputs, [got[0], None, got[2]])[0][1] is None
    i = int(np.flatnonzero(np.isinf(inputs["AL"][:, 1]))[0])
    wrong = dict(read, AL=read["AL"].copy())
    wrong["AL"][i, 1] = -3.0
    with pytest.raises(AssertionError):
        E.check_batched_rays(s["A"], s["AT"], wrong, norms, scalars, inputs, got)
    with pytest.raises(AssertionError):                                          # ... and a NaN in a slot fails
        E.check_batched_rays(s["A"], s["AT"], read, norms, scalars, inputs, [dict(got[0], VZ=np.nan)] + got[1:])


def test_the_step_level_entry_is_exported_with_the_headers_signatures_and_refuses_a_null_handle():
    import ctypes as C
    from test_resolve import header_prototypes
    protos = header_prototypes()
    want = {"hprlp_batched_solver_ray_step": ("int", ["hprlp_batched_solver *", "const int *", "int", "double *", "int *"]),
            "hprlp_batched_solver_get_panel": ("long", ["hprlp_batched_solver *", "const char *", "double *", "long"]),
            "hprlp_batched_solver_set_panel": ("int", ["hprlp_batched_solver *", "const char *", "const double *", "long"])}
    ctype_of = {"hprlp_batched_solver *": C.c_void_p, "const int *": hprlp.c_int_p, "int *": hprlp.c_int_p, "int": C.c_int,
                "double *": hprlp.c_dbl_p, "const double *": hprlp.c_dbl_p, "const char *": C.c_char_p, "long": C.c_long}
    L = hprlp.lib()
    for name, (ret, params) in want.items():
        assert protos[name] == (ret, params), protos[name]
        fn = getattr(L, name)
        assert list(fn.argtypes) == [ctype_of[p] for p in params] and fn.restype is (C.c_long if ret == "long" else C.c_int)
    v, k = np.zeros(9), np.zeros(1, dtype=np.intc)
    P, I = v.ctypes.data_as(hprlp.c_dbl_p), k.ctypes.data_as(hprlp.c_int_p)
    assert L.hprlp_batched_solver_ray_step(None, I, 1, P, I) == -1 and "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_get_panel(None, b"C", P, 9) == -1 and "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_set_panel(None, b"X_bar", P, 9) == -1 and "null solver" in hprlp.last_error()
    for f in ("ray_step", "get_panel", "set_panel"):
        assert callable(getattr(hprlp.BatchedSolver, f)), f
    assert hprlp.BatchedSolver.RAY_SLOTS == E.RAY_SLOTS
