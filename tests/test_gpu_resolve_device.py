"""Device-resident re-solve on the GPU (include/hprlp_amd.h hprlp_solver_set_data_device / _resolve_device /
_set_matrix_values_device / _transfer, DESIGN.md "Device-resident re-solve"), through the C ABI via hprlp.py.  The reference of
every comparison is the host entry on a second solver prepared the same way; equality is bit for bit (status, iter, every
scalar of Results but the wall-clock times, every trace row, array_equal on x, y, z).  The cases are in
tests/resolve_device_cases.py; those that name a kernel form run in a process of their own under that form's switches."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_detect import BASE_ENV, FORM_ENV
import resolve_device_cases as cases

pytestmark = pytest.mark.gpu
SCRIPT = os.path.join(ROOT, "tests", "resolve_device_cases.py")


def run_case(form, *args, timeout=600):
    env = dict(os.environ, **BASE_ENV, **FORM_ENV[form])
    r = subprocess.run([sys.executable, SCRIPT, *args], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0 or "OK" not in r.stdout:
        pytest.fail("%s: exit %d\n%s\n%s" % (" ".join(args), r.returncode, r.stdout[-2000:], r.stderr[-3000:]), pytrace=False)
    print("\n".join(r.stdout.strip().splitlines()[-4:]))


@pytest.mark.parametrize("form", ["small", "stream"])
def test_set_data_tensors_against_set_data(gpu, form):
    """The three changes, use_bc_scaling on and off, c alone, the bounds group alone, obj_constant alone: the five vectors, the
    six scalars and the next re-solve are the host entry's bits; transfer() is 0 / 0 against (2m + 3n) * 8 or the part given."""
    run_case(form, "set_data", form)


def test_resolve_tensors_against_resolve(gpu):
    """Cold, from a start, start and results in the same tensors, a caller's sigma, z not wanted, detection on seed 11's `kinds`
    data (verdict and certificate) and back to the base data."""
    cases.case_resolve()


def test_scatter_and_gather_under_a_locality_ordering(gpu):
    """k_unscale_out's perm direction and k_data_in's / k_start_in's gathers from the caller's buffers on the one shape the
    ordering is applied to (as tests/test_gpu_warm.py, test_gpu_resolve.py); two check intervals from a start."""
    run_case("reordered", "large", "reordered")


def test_one_tiled_case(gpu):
    run_case("tiled", "large", "tiled")


@pytest.mark.parametrize("form", ["small", "stream"])
def test_set_matrix_tensors_against_set_matrix(gpu, form):
    run_case(form, "matrix", form)


def test_entries_alternate_on_one_handle(gpu):
    cases.case_alternate()


def test_refused_calls_leave_the_solver_as_it_was(gpu):
    """A host address, a hipMalloc'ed buffer one element short, an output buffer one short (raw C calls); a numpy array, a CPU
    tensor, float32, a wrong length (ValueError); a NaN in c[7], in the last entry of u, inf in x0, a NaN in values (RuntimeError
    naming vector and index).  After each: the snapshot unchanged and a resolve_tensors() with the reference's bits."""
    cases.case_refusals()


def test_inputs_produced_on_a_side_stream(gpu):
    """The contract stated: inputs produced by a torch kernel on a non-default stream, which the entry is handed."""
    cases.case_stream()
