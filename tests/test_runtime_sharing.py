"""CPU: a process has ONE HIP runtime whichever of the library and torch is loaded first (hprlp._share_hip_runtime).

torch's wheel carries its own copies of libamdhip64 / libhsa-runtime64 with the system's SONAMEs, asked for by unversioned names.
Without the sharing, a torch imported after the library loads those copies beside the system's, and the second HSA runtime of the
process finds no GPU -- BatchedSolver.solve_tensors would then have no tensor to take.  Each order runs in a fresh process: what is
loaded into a process cannot be undone, and this one already holds the library.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[2])
if sys.argv[1] == "torch_first":
    import torch
from conftest import hprlp
hprlp.lib()
import torch
for key in ("libamdhip64", "libhsa-runtime64"):
    print(key, len({l.split()[-1] for l in open("/proc/self/maps") if key in l.split()[-1]}))
"""


@pytest.mark.parametrize("order", ["library_first", "torch_first"])
def test_one_hip_runtime_in_either_load_order(order):
    out = subprocess.run([sys.executable, "-c", CHILD, order, os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    counts = dict(line.split() for line in out.stdout.strip().splitlines())
    assert counts == {"libamdhip64": "1", "libhsa-runtime64": "1"}, (order, out.stdout)
