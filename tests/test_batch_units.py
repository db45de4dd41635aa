"""csrc/batch_units.h -- the per-element maps and per-member scalar rules that batch_prep.cpp and the kernels of batched.hip share --
stays plain host code: a host compiler that knows nothing of HIP takes batch_prep.cpp, which includes it, as it stands.  The values
are held by tests/test_batch_prep.py and tests/test_batch_prep_tree.py (host) and the GPU tests of the batched solver (device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_shared_units_compile_without_hip():
    csrc = os.path.join("hpr-lp-c_amd", "csrc")
    assert '#include "batch_units.h"' in open(os.path.join(ROOT, csrc, "batch_prep.h")).read()
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Iinclude", "-I" + csrc, os.path.join(csrc, "batch_prep.cpp")], cwd=ROOT,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
