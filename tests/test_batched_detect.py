"""CPU: the C ABI of the batched infeasibility detection (include/hprlp_amd.h: hprlp_batched_certificates,
hprlp_solve_batched_detect, hprlp_free_batched_certificates) and its Python mirror (hprlp.solve_batched_detect)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hprlp, lpgen

INC = os.path.join(ROOT, "include")
FIELDS = ("batch_size", "m", "n", "kind", "iter", "objective", "violation", "y", "z", "d")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "hprlp_amd.h"
#define O(f) offsetof(hprlp_batched_certificates, f)
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hprlp_batched_certificates), O(batch_size), O(m), O(n),
           O(kind), O(iter), O(objective), O(violation), O(y), O(z), O(d));
    return 0;
}
"""


@pytest.mark.parametrize("cc,std", [("gcc", "-std=c11"), ("g++", "-std=c++11")])
def test_batched_certificates_layout_equals_the_ctypes_mirror(cc, std, tmp_path):
    src = tmp_path / ("probe.c" if cc == "gcc" else "probe.cpp")
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, std, "-I", INC, str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    K = hprlp.CBatchedCertificates
    assert got == [C.sizeof(K)] + [getattr(K, f).offset for f in FIELDS]


def test_batched_detection_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", hprlp.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for s in ("hprlp_solve_batched_detect", "hprlp_free_batched_certificates", "solve_batched"):
        assert s in names, s


def _batch(B):
    lp = lpgen.planted_infeasible_lp(40, 60, 300, 3)
    rep = lambda v: np.repeat(np.asarray(v, float)[:, None], B, axis=1)
    model = hprlp.Model.from_csr(lp["m"], lp["n"], lp["rowptr"], lp["colind"], lp["values"], lp["AL"], lp["AU"], lp["l"], lp["u"], lp["c"])
    return lp, model, (rep(lp["c"]), rep(lp["AL"]), rep(lp["AU"]), rep(lp["l"]), rep(lp["u"]))


def test_solve_batched_detect_without_a_gpu_is_an_error_not_a_crash():
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    B = 3
    lp, model, (Cm, AL, AU, L, U) = _batch(B)
    for eps in (1e-8, None):  # detection on, and off (exactly solve_batched)
        r = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, None, hprlp.Parameters(max_iter=300, use_presolve=False),
                                       eps_primal=eps, eps_dual=eps)
        assert r["status"] == ["ERROR"] * B and r["x"] is None and r["batch_size"] == B
        k = r["certificates"]
        assert list(k["kind"]) == [0] * B and list(k["iter"]) == [0] * B
        assert k["y"] is None and k["z"] is None and k["d"] is None
    assert hprlp.last_error()
    model.free()


def test_negative_eps_is_an_error():
    """detection_from's check (abi_solve.cpp), on any machine: the eps are rejected before anything touches a device."""
    B = 2
    lp, model, (Cm, AL, AU, L, U) = _batch(B)
    for ep, ed in ((-1e-8, 1e-8), (1e-8, -1.0), (float("nan"), 1e-8)):
        r = hprlp.solve_batched_detect(model, Cm, AL, AU, L, U, None, hprlp.Parameters(max_iter=300, use_presolve=False),
                                       eps_primal=ep, eps_dual=ed)
        assert r["status"] == ["ERROR"] * B
        assert "eps" in hprlp.last_error()
        k = r["certificates"]
        assert list(k["kind"]) == [0] * B and k["y"] is None and k["d"] is None
    model.free()


def test_null_certificates_and_null_panels_through_the_c_entry():
    """certs may be NULL; NULL panels give "ERROR" per member and, with certs, batch_size / m / n and kind 0 for each."""
    L = hprlp.lib()
    lp, model, _ = _batch(2)
    det = hprlp.CDetection(1e-8, 1e-8)
    cc = hprlp.CBatchedCertificates()
    res = L.hprlp_solve_batched_detect(model._ptr, 2, None, None, None, None, None, None, None, C.byref(det), C.byref(cc))
    raw = C.string_at(res.status, 128)
    assert res.batch_size == 2 and not res.x and raw[:5] == b"ERROR" and raw[64:69] == b"ERROR"
    assert (cc.batch_size, cc.m, cc.n) == (2, lp["m"], lp["n"]) and [cc.kind[0], cc.kind[1]] == [0, 0]
    assert not cc.y and not cc.z and not cc.d
    L.free_batched_results(C.byref(res))
    L.hprlp_free_batched_certificates(C.byref(cc))
    assert not cc.kind and not cc.iter
    res = L.hprlp_solve_batched_detect(model._ptr, 2, None, None, None, None, None, None, None, C.byref(det), None)
    assert res.batch_size == 2
    L.free_batched_results(C.byref(res))
    model.free()
