"""Wide members of a group of LPs, the parts that need no GPU (include/hprlp_amd.h: hprlp_solver_set_group_wide,
hprlp_solve_many_wide, hprlp_last_many_wide_counts, hprlp_group_iteration_plan; csrc/group_table.cpp: the segments of a round's
normal iterations; DESIGN.md "Many small LPs", wide members).  What needs a GPU is in tests/test_gpu_many_wide.py."""
import os
import subprocess

import pytest

from conftest import hprlp, lpgen

SYMBOLS = ("hprlp_solver_set_group_wide", "hprlp_solve_many_wide", "hprlp_last_many_wide_counts", "hprlp_group_iteration_plan")

COUNT_VECTORS = {"all equal": [5, 5, 5, 5], "a restart and an idle member": [7, 6, 0, 7], "all zero": [0, 0, 0], "one member": [149],
                 "strictly increasing": [1, 2, 3, 10, 149]}


def test_the_host_selftest_passes_with_the_checks_of_the_segments():
    """group_table: checks 12 and 13, the iteration plan and the stage order of a round with segments."""
    assert hprlp.lib().hprlp_group_table_selftest() == 0


@pytest.mark.parametrize("name", sorted(COUNT_VECTORS))
def test_iteration_plan(name):
    counts = COUNT_VECTORS[name]
    plan = hprlp.group_iteration_plan(counts)
    distinct = sorted({c for c in counts if c > 0})
    assert plan is not None and len(plan) == len(distinct), (plan, distinct)
    assert [at for _, at in plan] == distinct
    assert all(ln > 0 for ln, _ in plan)
    for c in counts:
        # the member's segments are those whose threshold it reaches: the first ones, and their lengths add up to its count
        mine = [ln for ln, at in plan if c >= at]
        assert sum(mine) == c, (c, plan)
        assert mine == [ln for ln, _ in plan[:len(mine)]]
        if c == 0:
            assert mine == []
    if distinct:
        assert hprlp.group_iteration_plan(counts, cap=len(distinct) - 1) is None
        assert hprlp.group_iteration_plan(counts, cap=len(distinct)) == plan
    else:
        assert hprlp.group_iteration_plan(counts, cap=0) == []


def test_iteration_plan_refuses_wrong_arguments():
    L = hprlp.lib()
    assert hprlp.group_iteration_plan([3, -1, 2]) is None
    assert L.hprlp_group_iteration_plan(None, 2, None, None, 0) == -1
    assert L.hprlp_group_iteration_plan(None, -1, None, None, 0) == -1
    assert L.hprlp_group_iteration_plan(None, 0, None, None, 0) == 0


def test_the_new_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in SYMBOLS:
        assert s in names, s


def test_null_arguments_are_refused_with_a_message():
    L = hprlp.lib()
    assert L.hprlp_solver_set_group_wide(None, 1) == -1
    assert "hprlp_solver_set_group_wide" in hprlp.last_error()
    assert L.hprlp_solve_many_wide(None, 1, None, None, None, None) == -1
    assert "hprlp_solve_many_wide" in hprlp.last_error()
    assert L.hprlp_last_many_wide_counts(None) == -1
    with pytest.raises(ValueError):
        hprlp.solve_many_wide([])


def test_without_a_gpu_the_entries_fail_loudly(capfd):
    """No CPU fallback exists: every member of hprlp_solve_many_wide comes back with status ERROR and no arrays, a solver cannot be
    created to be marked wide, and the counts stay zero."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    lps = [lpgen.planted_lp(30, 50, 200, seed) for seed in (1, 2)]
    models = [hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
              for lp in lps]
    results, certs = hprlp.solve_many_wide(models, hprlp.Parameters(max_iter=100))
    assert [r.status for r in results] == ["ERROR"] * 2
    assert all(r.x is None and r.y is None and r.z is None for r in results)
    assert "hprlp_solve_many_wide: model 1" in hprlp.last_error()
    assert all(k.kind == 0 for k in certs)
    assert "model 0 failed its set-up" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        hprlp.Solver(models[0])
    assert set(hprlp.last_many_wide_counts().values()) == {0}
    for m in models:
        m.free()
