"""Group set-up of many small LPs, the parts that need no GPU (csrc/alloc.cpp: the arena's bookkeeping; include/hprlp_amd.h: the
four group entry points; csrc/env.cpp: the fall-back hook)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT, hprlp

NEW = ("hprlp_solver_create_many", "hprlp_solver_scale_many", "hprlp_solver_destroy_many", "hprlp_last_setup_many_counts")


def test_arena_bookkeeping():
    """Alignment, growth by a further block, a request larger than a block, the reference count."""
    L = hprlp.lib()
    L.hprlp_arena_selftest.restype = C.c_int
    assert L.hprlp_arena_selftest() == 0


def test_group_entry_points_are_exported_unmangled():
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lib", "libhprlp.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert set(NEW) <= exported, set(NEW) - exported
    L = hprlp.lib()
    assert all(hasattr(L, f) for f in NEW)
    assert set(hprlp.last_setup_many_counts()) == set(hprlp.SETUP_MANY_KEYS) and len(hprlp.SETUP_MANY_KEYS) == 8


def test_create_many_fails_loudly_without_gpu(model_mps_arrays):
    """No CPU fall-back: without a GPU the group creation returns -1 (or no handle at all) and says why."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    a = model_mps_arrays
    m = hprlp.Model.from_csr(a["m"], a["n"], a["rowptr"], a["colind"], a["values"], a["AL"], a["AU"], a["l"], a["u"], a["c"])
    L = hprlp.lib()
    ptrs = (C.POINTER(hprlp.CLPInfo) * 2)(m._ptr, m._ptr)
    out = (C.c_void_p * 2)()
    cp = hprlp.Parameters(use_presolve=False).to_c()
    rc = L.hprlp_solver_create_many(ptrs, 2, C.byref(cp), out)
    assert rc == -1 or (rc == 0 and not out[0] and not out[1])
    assert hprlp.last_error()
    if rc == 0:
        assert hprlp.Solver.create_many([m, m], hprlp.Parameters(use_presolve=False)) == [None, None]
        assert "hprlp_solver_create_many: model 1" in hprlp.last_error()
    m.free()


def test_refusals_need_no_gpu():
    L = hprlp.lib()
    out = (C.c_void_p * 1)()
    assert L.hprlp_solver_create_many(None, 1, None, out) == -1 and "null model list" in hprlp.last_error()
    assert L.hprlp_solver_scale_many(None, 1) == -1 and "null solver list" in hprlp.last_error()
    assert L.hprlp_solver_scale_many(out, 0) == -1 and "count must be positive" in hprlp.last_error()
    L.hprlp_solver_destroy_many(None, 3)
    assert all(v == 0 for v in hprlp.last_setup_many_counts().values())


def test_fall_back_hook_is_in_the_table_and_documented():
    L = hprlp.lib()
    n = L.hprlp_env_switches(None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.hprlp_env_switches(buf, n + 1) == n
    table = dict(ln.split("\t")[:2] for ln in buf.value.decode().splitlines())
    assert table.get("HPRLP_NO_GROUP_SETUP") == "hook"
    assert "HPRLP_NO_GROUP_SETUP" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
