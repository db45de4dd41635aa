"""Streams with parents without a GPU (include/hprlp_amd.h hprlp_batched_solver_solve_stream_parents / _device,
hprlp_stream_schedule_parents_host; DESIGN.md "Streamed batches", "Parents"): the exported symbols and the header's words; the
refusals that need no solver; the schedule -- the free slots in ascending order take the READY problems in ascending number, a
problem being ready once its parent has left -- against a heap simulation written here, on chains, a binary tree, stars, all
roots and random forests; and the stand-alone checker of the queue and the schedule under the host sanitizers."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hprlp

NEW = ("hprlp_batched_solver_solve_stream_parents", "hprlp_batched_solver_solve_stream_parents_device",
       "hprlp_batched_solver_stream_parents_info", "hprlp_stream_schedule_parents_host")


def simulate(events, width, parent):
    """The rule restated: a heap of (event at which the member ends, slot, problem), a heap of free slots and a heap of ready
    problems.  All members that end at one event leave together and make their children ready; then pass after pass, the free
    slots ascending take the ready problems ascending; a new member of length 0 leaves in the pass and is followed in the next."""
    count = len(events)
    W = min(width, count)
    children = [[] for _ in range(count)]
    for p, q in enumerate(parent):
        if q >= 0:
            children[q].append(p)
    slot, ein, eout = [-1] * count, [-1] * count, [-1] * count
    running, free, ready = [], list(range(W)), [p for p in range(count) if parent[p] < 0]
    e = 0
    while True:
        while free and ready:   # the passes of event e
            pairs = []
            while free and ready:
                pairs.append((heapq.heappop(free), heapq.heappop(ready)))
            for k, p in pairs:
                slot[p], ein[p] = k, e
                if events[p] > 0:
                    heapq.heappush(running, (e + int(events[p]), k, p))
                    continue
                eout[p] = e
                heapq.heappush(free, k)
                for c in children[p]:
                    heapq.heappush(ready, c)
            if not any(events[p] == 0 for _, p in pairs):
                break
        if not running:
            break
        e = running[0][0]
        while running and running[0][0] == e:
            _, k, p = heapq.heappop(running)
            eout[p] = e
            heapq.heappush(free, k)
            for c in children[p]:
                heapq.heappush(ready, c)
    return np.array(slot), np.array(ein), np.array(eout)


def check(events, width, parent):
    events, parent = np.asarray(events), np.asarray(parent)
    got = hprlp.stream_schedule(events, width, parent)
    want = simulate(events, width, parent)
    for g, w, name in zip(got, want, ("slot", "event_in", "event_out")):
        assert np.array_equal(g, w), (name, width, list(events), list(parent), list(g), list(w))
    s, ein, eout = got
    W = min(width, len(events))
    assert (ein >= 0).all() and np.array_equal(eout - ein, events) and s.min() >= 0 and s.max() < W
    kids = np.flatnonzero(parent >= 0)
    assert (ein[kids] >= eout[parent[kids]]).all()   # no child before its parent has left
    for e in np.unique(np.concatenate([ein, eout])):   # at most W in flight between two events; a slot holds one member at a time
        inside = np.flatnonzero((ein <= e) & (e < eout))
        assert len(inside) <= W and len(set(s[inside])) == len(inside), (e, list(inside))
    # slots taken ascending and ready problems taken ascending: an event at which no member of length 0 enters has ONE pass, and in
    # it the lower problem number has the lower slot
    for e in np.unique(ein):
        entered = np.flatnonzero(ein == e)
        if (events[entered] > 0).all():
            assert list(s[entered]) == sorted(s[entered]), (e, list(entered), list(s[entered]))
    return got


def forest(rng, count, shape):
    if shape == "chains":   # numbered period by period
        c = int(rng.integers(1, 8))
        return np.array([-1 if p < c else p - c for p in range(count)])
    if shape == "tree":     # one root, binary
        return np.array([-1 if p == 0 else (p - 1) // 2 for p in range(count)])
    if shape == "stars":
        c = int(rng.integers(1, 5))
        return np.array([-1 if p < c else p % c for p in range(count)])
    if shape == "roots":
        return np.full(count, -1)
    return np.array([int(rng.integers(-1, p)) if p else -1 for p in range(count)])   # a random forest


@pytest.mark.parametrize("shape", ["chains", "tree", "stars", "roots", "random"])
def test_schedule_with_parents_matches_a_heap_simulation(shape):
    rng = np.random.default_rng({"chains": 1, "tree": 2, "stars": 3, "roots": 4, "random": 5}[shape])
    for rep in range(60):
        count, width = int(rng.integers(1, 201)), int(rng.integers(1, 71))
        events = rng.integers(0, 31, size=count)
        events[rng.random(count) < (0.6 if rep % 3 == 0 else 0.2)] = 0   # a good share of zeros
        parent = forest(rng, count, shape)
        got = check(events, width, parent)
        if shape == "roots":   # array for array what the schedule without parents gives
            for g, w in zip(got, hprlp.stream_schedule(events, width)):
                assert np.array_equal(g, w)


def test_a_chain_takes_the_sum_of_its_lengths_whatever_the_width():
    rng = np.random.default_rng(9)
    for width in (1, 2, 7, 64):
        events = rng.integers(0, 9, size=23)
        s, ein, eout = check(events, width, np.arange(23) - 1)
        assert eout.max() == events.sum() and not s.any()   # (one root followed by a chain: always the lowest free slot)
    # ... and a child of a member of length 0 enters within the same event
    s, ein, eout = check([0, 0, 3, 0], 2, [-1, 0, 1, 0])
    assert list(ein) == [0, 0, 0, 0] and list(eout) == [0, 0, 3, 0] and list(s) == [0, 0, 0, 1]


def test_empty_slots_fill_when_children_become_ready():
    # a binary tree through 4 slots: the root alone at event 0, both children when it leaves, four grandchildren after the first child
    s, ein, eout = check([2, 3, 1, 1, 1, 1, 1], 4, [-1, 0, 0, 1, 1, 2, 2])
    assert list(ein) == [0, 2, 2, 5, 5, 3, 3] and list(s) == [0, 0, 1, 0, 1, 1, 2]


def test_refusals_without_a_gpu():
    L = hprlp.lib()
    ev = (C.c_int * 3)(1, 2, 0)
    o = [(C.c_int * 3)() for _ in range(3)]
    ok = (C.c_int * 3)(-1, 0, 0)
    assert L.hprlp_stream_schedule_parents_host(3, 1, ev, ok, *o) == 3
    for par, words in (((C.c_int * 3)(-1, 1, 0), ("parent[1] = 1",)), ((C.c_int * 3)(-1, 2, 0), ("parent[1] = 2",)),
                       ((C.c_int * 3)(-1, -2, 0), ("parent[1] = -2",)), ((C.c_int * 3)(0, -1, -1), ("parent[0] = 0",)),
                       (None, ("null parent",))):
        assert L.hprlp_stream_schedule_parents_host(3, 1, ev, par, *o) == -1
        assert all(w in hprlp.last_error() for w in words), hprlp.last_error()
    with pytest.raises(ValueError, match=r"parent\[2\] = 5"):
        hprlp.stream_schedule([1, 1, 1], 2, [-1, 0, 5])
    with pytest.raises(ValueError, match="3 entries"):
        hprlp.stream_schedule([1, 1, 1], 2, [-1, 0])
    # the two solve entries: what the arguments alone tell is refused before the solver is looked at
    d = (C.c_double * 4)()
    res = hprlp.CBatchedResults()
    sc = hprlp.CBatchedScalars()
    one = (C.c_int * 1)(-1)

    def host(count=1, width=1, vec=d, prm=None, X0=None, Y0=None, parent=one, out=res):
        return L.hprlp_batched_solver_solve_stream_parents(None, count, width, vec, d, d, d, d, None, None if prm is None else C.byref(prm),
                                                           X0, Y0, parent, None, None, C.byref(out) if out is not None else None)

    def device(count=1, width=1, vec=d, prm=None, X0=None, Y0=None, parent=one, out=sc):
        a = lambda v: None if v is None else C.cast(v, C.c_void_p)
        return L.hprlp_batched_solver_solve_stream_parents_device(None, count, width, a(vec), a(d), a(d), a(d), a(d), None,
                                                                  None if prm is None else C.byref(prm), a(X0), a(Y0), parent, None, None,
                                                                  None, a(d), a(d), a(d), C.byref(out) if out is not None else None)
    bad_prm = hprlp.Parameters(max_iter=451, use_presolve=False).to_c()
    for entry in (host, device):
        for kw, word in ((dict(count=0), "count and width must be positive"), (dict(width=0), "count and width must be positive"),
                         (dict(vec=None), "null C"), (dict(out=None), "null results"), (dict(prm=bad_prm), "multiple of check_iter"),
                         (dict(parent=None), "null parent"), (dict(X0=d), "X0 and Y0 come together"), (dict(Y0=d), "X0 and Y0 come together")):
            assert entry(**kw) == -1
            assert word in hprlp.last_error(), (entry.__name__, kw, hprlp.last_error())
        assert entry(X0=d, Y0=d) == -1 and "null solver" in hprlp.last_error(), hprlp.last_error()
        assert entry() == -1 and "null solver" in hprlp.last_error() and "_solve_stream_parents" in hprlp.last_error()
    out4 = (C.c_long * 4)()
    assert L.hprlp_batched_solver_stream_parents_info(None, out4) == -1 and "null solver" in hprlp.last_error()


def test_new_symbols_are_exported_and_documented():
    L = hprlp.lib()
    header = open(os.path.join(ROOT, "include", "hprlp_amd.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in header, name
    for word in ("parent[p] == -1", "0 <= parent[p] < p", "READY", "together or not at all", "ERROR"):
        assert word in header, word
    for name in ("solve_stream", "solve_stream_tensors", "stream_parents_info"):
        assert callable(getattr(hprlp.BatchedSolver, name))
    import inspect
    for fn in (hprlp.BatchedSolver.solve_stream, hprlp.BatchedSolver.solve_stream_tensors, hprlp.stream_schedule):
        assert inspect.signature(fn).parameters["parent"].default is None


def test_parents_checker_under_the_host_sanitizers(tmp_path):
    """stream_schedule.cpp in the stand-alone program tools/stream_parents_check.cpp (its own main, no GPU, no HIP) under
    -fsanitize=address,undefined: clean, exit 0."""
    exe = tmp_path / "stream_parents_check"
    csrc = os.path.join(ROOT, "hpr-lp-c_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                            os.path.join(ROOT, "tools", "stream_parents_check.cpp"), os.path.join(csrc, "stream_schedule.cpp"),
                            "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "stream parents check: ok" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
