"""Device-resident streams without a GPU (include/hprlp_amd.h hprlp_batched_solver_solve_stream_device /
hprlp_batched_solver_stream_memory, DESIGN.md "Device-resident streams"): the symbols and their documentation, the refusals that the
arguments alone decide -- with the host stream's words -- and the Python wrapper's checks, which come before the library is called.
The bits are held on the GPU by tests/test_gpu_batched_stream_device.py."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import _have_gpu, hprlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hprlp_batched_solver_solve_stream_device", "hprlp_batched_solver_stream_memory")


def test_new_symbols_are_exported_and_documented():
    L = hprlp.lib()
    for name in NEW:
        assert hasattr(L, name), name
    for name in ("solve_stream_tensors", "stream_memory"):
        assert callable(getattr(hprlp.BatchedSolver, name)), name
    header = open(os.path.join(ROOT, "include", "hprlp_amd.h")).read()
    for name in NEW:
        at = header.index(name + "(")
        doc = header[header.rindex("/*", 0, at):at]
        assert "*/" in doc and len(doc) > 200, (name, doc)   # (the comment right above the declaration)
    doc = header[header.index("device-resident streams"):header.index("hprlp_batched_solver_solve_stream_device(")]
    for word in ("hipPointerGetAttributes", "tree rule", "bit for bit", "zero columns", "carry", "non-finite"):
        assert word in doc, word
    assert "no device entry" not in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Device-resident streams" in design and "no device entry" not in design
    assert design.index("### Streamed batches") < design.index("### Device-resident streams") < design.index("### Device-resident re-solve")


def test_refusals_the_arguments_alone_decide():
    """No solver and no GPU is needed for them, and the words are the host stream's (tests/test_batched_stream.py)."""
    L = hprlp.lib()
    d = (C.c_double * 4)()
    p = C.cast(d, C.c_void_p)   # (never read: every call below is refused before a pointer is looked at)
    sc = hprlp.CBatchedScalars()

    def stream(count, width, vec=p, prm=None, out=sc, x=p):
        return L.hprlp_batched_solver_solve_stream_device(None, count, width, vec, p, p, p, p, None, None if prm is None else C.byref(prm),
                                                          None, None, None, None, None, x, p, p, C.byref(out) if out is not None else None)
    for args, word in (((0, 4), "count and width must be positive"), ((4, 0), "count and width must be positive"),
                       ((-3, 4), "count and width must be positive"), ((1, 1, None), "null C"), ((1, 1, p, None, None), "null results"),
                       ((1, 1, p, None, sc, None), "null results")):
        assert stream(*args) == -1
        assert word in hprlp.last_error() and hprlp.last_error().startswith("batched stream:"), hprlp.last_error()
    prm = hprlp.Parameters(max_iter=451, use_presolve=False).to_c()
    assert prm.check_iter == 150
    assert stream(1, 1, p, prm) == -1
    assert "multiple of check_iter" in hprlp.last_error() and "periodic event" in hprlp.last_error(), hprlp.last_error()
    assert stream(1, 1, p, hprlp.Parameters(max_iter=450, use_presolve=False).to_c()) == -1
    assert "null solver" in hprlp.last_error()
    assert L.hprlp_batched_solver_stream_memory(None, (C.c_long * 4)()) == -1 and "null solver" in hprlp.last_error()


class _Model:
    m, n = 3, 5


def _unbuilt_solver():
    """A BatchedSolver object that never reached the library: its handle is a word no call may use, so whatever gets past the
    wrapper's checks fails in ctypes or in the library, not silently."""
    s = hprlp.BatchedSolver.__new__(hprlp.BatchedSolver)
    s.model, s.device_number, s._last_B, s._h = _Model(), 0, 0, None
    return s


def test_the_wrapper_refuses_before_the_library_is_called(monkeypatch):
    torch = pytest.importorskip("torch")
    s = _unbuilt_solver()
    s._h = 1   # (not closed, as far as the wrapper can tell)
    called = []
    N = 4

    class OnDevice(torch.Tensor):   # a tensor that says it lives on the solver's device: every later check is reached without a GPU
        @property
        def device(self):
            return torch.device("cuda", 0)
    dev = lambda rows, cols=N, dtype=torch.float64: torch.zeros((rows, cols), dtype=dtype).as_subclass(OnDevice)
    good = lambda: [dev(5), dev(3), dev(3), dev(5), dev(5)]
    cases = {
        "numpy": ([np.zeros((5, N))] + good()[1:], {}, "torch tensor"),
        "numpy among tensors": ([dev(5), np.zeros((3, N))] + good()[2:], {}, "torch tensor"),
        "float32": ([dev(5, dtype=torch.float32)] + good()[1:], {}, "float64"),
        "a CPU tensor": ([dev(5), torch.zeros((3, N), dtype=torch.float64)] + good()[2:], {}, "device"),
        "rows": ([dev(4)] + good()[1:], {}, "shape"),
        "columns": ([dev(5), dev(3), dev(3, N - 1), dev(5), dev(5)], {}, "shape"),
        "a start": (good(), dict(X0=dev(3)), "shape"),
    }
    # the wrapper asks the library only whether it has the entry: a stand-in that has the two symbols, and records every call of one
    monkeypatch.setattr(hprlp, "lib", lambda: type("L", (), {n: staticmethod(lambda *a: called.append(n) or -1) for n in NEW})())
    for tag, (args, kw, word) in cases.items():
        with pytest.raises(ValueError) as e:
            s.solve_stream_tensors(*args, width=2, **kw)
        assert word in str(e.value) and "solve_stream_tensors" in str(e.value), (tag, str(e.value))
    assert not called, called
    s._h = None   # (nothing to destroy)


def test_without_a_gpu_the_call_fails_loudly():
    s = _unbuilt_solver()
    with pytest.raises(RuntimeError, match="closed"):
        s.solve_stream_tensors(None, None, None, None, None)
    if _have_gpu():
        return
    lp_model = hprlp.Model.from_csr(2, 2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 3.0, 1.0], [-np.inf] * 2, [10.0, 12.0], [0.0] * 2, [np.inf] * 2,
                                    [-3.0, -5.0])
    with pytest.raises(RuntimeError, match="GPU"):
        hprlp.BatchedSolver(lp_model)
    lp_model.free()
