"""Streamed batches without a GPU (include/hprlp_amd.h hprlp_stream_schedule_host / hprlp_batched_solver_solve_stream, DESIGN.md
"Streamed batches"): the schedule the streamed loop follows -- freed slots in ascending order take the queued problems in
ascending order, a member of length 0 hands its slot on within the same event -- against a heap simulation written here; the
figures DESIGN.md quotes for the CPU oracle's iteration counts; the refusals that need no solver; the exported symbols; and the
stand-alone checker of the schedule under the host sanitizers."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, hprlp

# The CPU oracle's iterations of the 24 members of make_batch(planted_lp(300, 400, 2400, 7, "network"), 24, 2) at stop_tol 1e-6,
# use_CR_scaling off (oracle.solve_batched; every member OPTIMAL, no lambda bump), in evaluations of check_iter = 150.
ORACLE_ITERS_1E6 = (3150, 3750, 6900, 8850, 4500, 5100, 3900, 4050, 9750, 5700, 2550, 4950, 3150, 4800, 2850, 5550, 5550, 2100, 3300,
                    3600, 7800, 8250, 4800, 5700)


def simulate(events, width):
    """The rule restated with a heap of (event at which the slot's member ends, slot): all slots that end at one event are freed
    together and refilled in ascending slot order; a new member of length 0 ends at the same event, in a later pass of it."""
    count = len(events)
    W = min(width, count)
    slot, ein, eout = [-1] * count, [-1] * count, [-1] * count
    heap, nxt = [], 0
    for k in range(W):
        slot[nxt], ein[nxt] = k, 0
        heapq.heappush(heap, (int(events[nxt]), k, nxt))
        nxt += 1
    while heap:
        e = heap[0][0]
        ended = []
        while heap and heap[0][0] == e:
            ended.append(heapq.heappop(heap))
        while ended:   # the passes of event e
            for _, _, p in ended:
                eout[p] = e
            again = []
            for _, k, _ in sorted(ended, key=lambda t: t[1]):
                if nxt == count:
                    break
                slot[nxt], ein[nxt] = k, e
                item = (e + int(events[nxt]), k, nxt)
                (again if events[nxt] == 0 else heap).append(item)
                nxt += 1
            heapq.heapify(heap)
            ended = again
    return np.array(slot), np.array(ein), np.array(eout)


def check(events, width):
    got = hprlp.stream_schedule(events, width)
    want = simulate(events, width)
    for g, w, name in zip(got, want, ("slot", "event_in", "event_out")):
        assert np.array_equal(g, w), (name, width, list(events), list(g), list(w))
    s, ein, eout = got
    assert np.array_equal(eout - ein, np.asarray(events))
    for k in range(min(width, len(events))):   # a slot holds one member at a time, and the next enters when the last one leaves
        mine = np.flatnonzero(s == k)
        assert np.array_equal(mine, np.sort(mine))
        assert all(ein[b] == eout[a] for a, b in zip(mine[:-1], mine[1:]))
    return got


@pytest.mark.parametrize("seed", range(6))
def test_schedule_matches_a_heap_simulation_on_random_lengths(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        count, width = int(rng.integers(1, 60)), int(rng.integers(1, 20))
        events = rng.integers(0 if seed % 2 else 1, 12, size=count)
        if seed >= 4:   # many ties and many members that end at once
            events = rng.integers(0, 3, size=count)
        check(events, width)


def test_schedule_on_the_oracles_lengths():
    events = np.array(ORACLE_ITERS_1E6) // 150
    assert (events * 150 == np.array(ORACLE_ITERS_1E6)).all() and events.min() == 14 and events.max() == 65
    s, ein, eout = check(events, 8)
    assert eout.max() == 121 and eout.max() * 150 == 18150
    batches = sum(int(events[g:g + 8].max()) for g in (0, 8, 16))
    assert batches == 179 and [int(events[g:g + 8].max()) * 150 for g in (0, 8, 16)] == [8850, 9750, 8250]
    occupancy = events.sum() / (8 * eout.max()), events.sum() / (8 * batches)
    assert abs(occupancy[0] - 0.83) < 0.005 and abs(occupancy[1] - 0.56) < 0.005, occupancy
    assert list(s[:8]) == list(range(8)) and (ein[:8] == 0).all()
    assert s[8] == 0 and ein[8] == 21 and s[9] == 1 and ein[9] == 25   # (problems 0 and 1 are the first two to end)


def test_members_of_length_zero_hand_the_slot_on_within_the_event():
    s, ein, eout = check([0, 5, 0, 0, 0, 3, 0], 2)
    # slot 0: problem 0 ends at event 0, then 2, 3, 4 in a row, all at event 0, then 5 stays
    assert list(s) == [0, 1, 0, 0, 0, 0, 0] and list(ein) == [0, 0, 0, 0, 0, 0, 3] and list(eout) == [0, 5, 0, 0, 0, 3, 3]
    s, ein, eout = check([0] * 9, 4)
    assert (ein == 0).all() and (eout == 0).all() and list(s) == [0, 1, 2, 3, 0, 1, 2, 3, 0]
    s, ein, eout = check([2, 2, 0, 0, 1], 2)   # both slots freed at event 2; the zero-length members pass through slot 0 then 1
    assert list(s) == [0, 1, 0, 1, 0] and list(ein) == [0, 0, 2, 2, 2] and list(eout) == [2, 2, 2, 2, 3]


@pytest.mark.parametrize("width", (5, 8, 64))
def test_count_at_most_width_is_one_batch(width):
    events = [4, 0, 7, 1, 3]
    s, ein, eout = check(events, width)
    assert list(s) == list(range(5)) and (ein == 0).all() and list(eout) == events


def test_refusals_without_a_gpu():
    L = hprlp.lib()
    i3 = (C.c_int * 3)(1, 2, 3)
    o = [(C.c_int * 3)() for _ in range(3)]
    assert L.hprlp_stream_schedule_host(3, 2, i3, *o) == 4   # (the makespan: problem 2 follows problem 0 in slot 0, events 1 .. 4)
    for count, width, ev, outs, word in ((0, 2, i3, o, "positive"), (3, 0, i3, o, "positive"), (-1, 2, i3, o, "positive"),
                                         (3, 2, None, o, "null"), (3, 2, i3, [o[0], None, o[2]], "null"),
                                         (3, 2, (C.c_int * 3)(1, -1, 3), o, "negative")):
        assert L.hprlp_stream_schedule_host(count, width, ev, *outs) == -1
        assert word in hprlp.last_error(), hprlp.last_error()
    with pytest.raises(ValueError):
        hprlp.stream_schedule([1, -2], 2)
    # the stream entry: what the arguments alone tell is refused before the solver is looked at
    d = (C.c_double * 4)()
    res = hprlp.CBatchedResults()

    def stream(count, width, vec=d, prm=None, out=res):
        return L.hprlp_batched_solver_solve_stream(None, count, width, vec, d, d, d, d, None, None if prm is None else C.byref(prm), None,
                                                   None, None, None, C.byref(out) if out is not None else None)
    for args, word in (((0, 4), "count and width must be positive"), ((4, 0), "count and width must be positive"),
                       ((-3, 4), "count and width must be positive"), ((1, 1, None), "null C"), ((1, 1, d, None, None), "null results")):
        assert stream(*args) == -1
        assert word in hprlp.last_error(), hprlp.last_error()
    prm = hprlp.Parameters(max_iter=451, use_presolve=False).to_c()
    assert prm.check_iter == 150
    assert stream(1, 1, d, prm) == -1
    assert "multiple of check_iter" in hprlp.last_error() and "periodic event" in hprlp.last_error(), hprlp.last_error()
    assert stream(1, 1, d, hprlp.Parameters(max_iter=450, use_presolve=False).to_c()) == -1
    assert "null solver" in hprlp.last_error()
    for fn, args in ((L.hprlp_batched_solver_stream_record, (None, None, None)), (L.hprlp_batched_solver_stream_info, (None,)),
                     (L.hprlp_batched_solver_lambda, (None,)), (L.hprlp_batched_solver_stream_seconds, (None,))):
        assert fn(None, *args) == -1 and "null solver" in hprlp.last_error()


def test_new_symbols_are_exported():
    L = hprlp.lib()
    for name in ("hprlp_batched_solver_solve_stream", "hprlp_batched_solver_stream_record", "hprlp_batched_solver_stream_info",
                 "hprlp_batched_solver_stream_seconds", "hprlp_batched_solver_lambda", "hprlp_stream_schedule_host"):
        assert hasattr(L, name), name
    for name in ("solve_stream", "stream_info", "lambda_max"):
        assert callable(getattr(hprlp.BatchedSolver, name))
    header = open(os.path.join(ROOT, "include", "hprlp_amd.h")).read()
    for name in ("hprlp_batched_solver_solve_stream", "hprlp_batched_solver_stream_record", "hprlp_batched_solver_stream_info",
                 "hprlp_batched_solver_lambda", "hprlp_stream_schedule_host"):
        assert name + "(" in header, name


def test_schedule_checker_under_the_host_sanitizers(tmp_path):
    """stream_schedule.cpp in the stand-alone program tools/stream_schedule_check.cpp (its own main, no GPU, no HIP) under
    -fsanitize=address,undefined: clean, exit 0."""
    exe = tmp_path / "stream_schedule_check"
    csrc = os.path.join(ROOT, "hpr-lp-c_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                            os.path.join(ROOT, "tools", "stream_schedule_check.cpp"), os.path.join(csrc, "stream_schedule.cpp"),
                            "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "stream schedule check: ok" in run.stdout, (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
