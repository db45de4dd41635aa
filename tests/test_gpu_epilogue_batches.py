"""The batched epilogue of a super-block (kernels.hip: epilogue_rows) at the shapes where its staged loads can go wrong.

The half-steps load a batch of four rows per lane in stages -- code bytes one batch ahead, then the loads that depend on the row
alone, then the loads a code selects (branch-free: a lane without a bound to read reads the super-block's first row), rows past
the end clamped to the last row -- over a loop unrolled across two sets of code registers.  None of that may change a bit of the
results.  A batch is 4 x 512 = 2048 rows; the super-block heights (HPRLP_TILE_ROWS) make a super-block's epilogue run

  (a) less than one batch (64 rows; the last super-block is a single row),
  (b) exactly one full batch (2048 rows, every super-block),
  (c) two batches with ONE valid row in the second (height 2560, last super-block 2049 rows: the second set of code registers,
      every other lane of the batch a clamped surplus lane),
  (d) a last super-block of a single row behind full ones (height 2048),

in the fused tiled form with the hand-off between the half-steps, the same with HPRLP_NO_FAR_PUSH=1, and the all-remainder form
(k_pb_fused, which calls the same epilogue).  The LP carries every column and row bound kind cycled by index
(evalcases.all_bounds_lp: l in {+0.0, -0.0, -inf, finite}, u in {+inf, finite}; equality, one-sided, ranged and free rows), so every
code value occurs inside every wave.

Checks per case: x and y (and the other state vectors) after 1, 2 and 5 normal iterations against the stream kernel at the
tolerance evalcases.py has for the tiled forms; 5 iterations in one run = five runs of 1, bit for bit; the default path (x rebuilt
from x_hat and last_x) = HPRLP_STORE_X=1, bit for bit; one check step (the CHECK epilogues) against the stream kernel and against
the evaluator of tests/evalref.py."""
import numpy as np
import pytest

import evalcases as C
from conftest import hprlp, lpgen
from oracle import oracle as O
from test_gpu_detect import BASE_ENV, FORM_ENV, model_of
from test_gpu_evaluation import EXPECT, FORM_HOOKS, NAMES, check_evaluation

pytestmark = pytest.mark.gpu

TOL = C.CASES["tiled"][2]
assert TOL == C.CASES["all-remainder"][2] == (1e-11, 1e-13)

# name -> (HPRLP_TILE_ROWS, m, n): rows of the last super-block of A / of A^T
SHAPES = {
    "a-under-one-batch": (64, 8001, 8065),              # 1 / 1
    "b-one-full-batch": (2048, 8192, 8192),             # 2048 / 2048
    "c-one-row-in-second-batch": (2560, 7169, 9729),    # 2049 / 2049
    "d-single-row-last-block": (2048, 6145, 8193),      # 1 / 1
}
FORMS = {
    "hand-off": ("tiled", {}),
    "no-far-push": ("tiled", {"HPRLP_NO_FAR_PUSH": "1"}),
    "all-remainder": ("all-remainder", {}),
}
# every value launch_bound_codes / launch_row_codes can produce (kernels.h: +0.0 and equality exclude reading the lower side)
COL_CODES = {0, 1, 2, 3, 4, 6}
ROW_CODES = {0, 1, 2, 3, 6}
SIGMA = 0.6
_lps, _stream = {}, {}


def shape_lp(shape):
    if shape not in _lps:
        rows_sb, m, n = SHAPES[shape]
        assert (m - 1) % rows_sb == (n - 1) % rows_sb and (m - 1) % rows_sb in (0, 2047, 2048)
        lp = C.all_bounds_lp(C._banded(lpgen, m, n, 6, 1200, 11 + len(_lps)), 300 + len(_lps))
        ck, rk = _code_kinds(lp)
        for w in range(0, m - 63, 64):     # every code value inside one wave (64 consecutive rows), in every wave
            assert set(rk[w:w + 64]) == ROW_CODES
        for w in range(0, n - 63, 64):
            assert set(ck[w:w + 64]) == COL_CODES
        _lps[shape] = lp
    return _lps[shape]


def _code_kinds(lp):
    """The code bytes as kernels.h defines them (bit 0: read the lower side, bit 1: read the upper side, bit 2: +0.0 / equality)."""
    l, u, AL, AU = lp["l"], lp["u"], lp["AL"], lp["AU"]
    l_zero = (l == 0) & ~np.signbit(l)
    ck = (~(l_zero | np.isneginf(l))).astype(int) | ((~np.isposinf(u)).astype(int) << 1) | (l_zero.astype(int) << 2)
    eq = np.isfinite(AU) & (AL == AU)
    rk = (~(np.isneginf(AL) | eq)).astype(int) | ((~np.isposinf(AU)).astype(int) << 1) | (eq.astype(int) << 2)
    return ck, rk


def set_env(monkeypatch, form, **more):
    for k in FORM_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(BASE_ENV, **FORM_ENV[form], **more).items():
        monkeypatch.setenv(k, v)


def solver(lp, lam=None):
    model = model_of(lp)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    s.scale()
    if lam is None:
        lam = 1.01 * s.power_iteration()[0]
    s.init(SIGMA, lam)
    return model, s, lam


def state(s):
    return {name: s.get(name) for name in NAMES}


def stream_reference(monkeypatch, shape):
    """The stream kernel's states after 1, 2 and 5 normal iterations and after a check step (once per shape, left unchanged)."""
    if shape not in _stream:
        lp = shape_lp(shape)
        set_env(monkeypatch, "stream")
        model, s, lam = solver(lp)
        d = s.describe()
        assert EXPECT["stream"] in d and "A^T: stream kernel" in d, d
        out = {"lam": lam}
        for total, step in ((1, 1), (2, 1), (5, 3)):
            s.iterate(step, False)
            out[total] = state(s)
        s.iterate(0, True)
        out["check"] = state(s)
        s.close(); model.free()
        _stream[shape] = out
    return _stream[shape]


def assert_close(got, want, where):
    for name in NAMES:
        np.testing.assert_allclose(got[name], want[name], rtol=TOL[0], atol=TOL[1], err_msg="%s %s" % (where, name))


def assert_same_bits(a, b, where):
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), (where, name, int((a[name] != b[name]).sum()), float(np.abs(a[name] - b[name]).max()))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", list(FORMS))
def test_epilogue_batches_keep_the_results(gpu, monkeypatch, form, shape):
    rows_sb, m, n = SHAPES[shape]
    hook_form, hooks = FORMS[form]
    lp = shape_lp(shape)
    want = stream_reference(monkeypatch, shape)
    lam = want["lam"]
    hooks = dict(hooks, HPRLP_TILE_ROWS=str(rows_sb))

    # five runs of one iteration, against the stream kernel after 1, 2 and 5
    set_env(monkeypatch, hook_form, **hooks)
    model, s, _ = solver(lp, lam)
    d = s.describe()
    assert EXPECT[hook_form] in d and s.info()["tiled"] == 3 and "piece form" not in d, d
    assert "%d super-blocks" % -(-m // rows_sb) in d and "%d super-blocks" % -(-n // rows_sb) in d and "(%d rows" % rows_sb in d, d
    singles = {}
    for total in range(1, 6):
        s.iterate(1, False)
        if total in (1, 2, 5):
            singles[total] = state(s)
            assert_close(singles[total], want[total], "%s %s after %d x 1" % (form, shape, total))
    s.close()
    assert np.abs(singles[5]["x"]).max() > 0 and np.abs(singles[5]["y"]).max() > 0

    # one run of five: the same bits; then one check step
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    s.scale()
    s.init(SIGMA, lam)
    s.iterate(5, False)
    run5 = state(s)
    assert_same_bits(run5, singles[5], "%s %s: a run of 5 against five runs of 1" % (form, shape))
    s.iterate(0, True)
    assert_close(state(s), want["check"], "%s %s after the check step" % (form, shape))
    ref = O.ScaledLP(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"],
                     O.Params.default(use_CR_scaling=0))
    got = s.residuals(6, True)
    check_evaluation(s, (lp["rowptr"], lp["colind"], ref.ATrp, ref.ATci), got, SIGMA, lam, "%s %s step 6" % (form, shape))
    s.close()

    # every normal x-half reads and stores x: the same bits as the rebuild from x_hat and last_x
    set_env(monkeypatch, hook_form, HPRLP_STORE_X="1", **hooks)
    s = hprlp.Solver(model, hprlp.Parameters(use_presolve=False, use_CR_scaling=False))
    assert "HPRLP_STORE_X=1" in s.describe().split("switches:")[1]
    s.scale()
    s.init(SIGMA, lam)
    s.iterate(5, False)
    assert_same_bits(state(s), run5, "%s %s: HPRLP_STORE_X=1 against the default" % (form, shape))
    s.close(); model.free()
