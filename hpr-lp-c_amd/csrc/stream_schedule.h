// stream_schedule.h -- which queued problem enters which slot of a streamed batch, and when (DESIGN.md "Streamed batches").
// Plain host code: no HIP header, no device call.  The streamed loop of batched.hip takes its slot decisions from stream_assign;
// stream_schedule plays the same rule forward from each problem's length, so that the loop's record can be held to it without a
// GPU (hprlp_stream_schedule_host, tests/test_batched_stream.py), and tools/stream_schedule_check.cpp runs both under the host
// sanitizers.
#pragma once

#include <vector>

namespace hprlp {

// The problems of a stream call that have not entered a slot yet: next .. count-1, in order.
struct StreamQueue {
    int count = 0, next = 0;
    int left() const { return count - next; }
};

// One refill pass: the freed slots, in ASCENDING order, take the queued problems in ascending order, as many as both last.
// freed: nfreed slot numbers, ascending.  pair_slot / pair_problem: room for nfreed entries; they come out ordered by slot.
// Returns the number of pairs.
int stream_assign(StreamQueue &q, const int *freed, int nfreed, int *pair_slot, int *pair_problem);

// The whole schedule from the problems' lengths.  events[p] >= 0: the evaluations problem p stays for (its final iteration /
// check_iter; 0: it ends at its iteration-0 evaluation, and its slot is handed on within the same event).  Slots
// 0 .. min(width, count)-1 take problems 0, 1, ... at event 0; at every event the members that end are taken out, the freed slots
// are refilled by stream_assign, and a new member of length 0 ends at once and frees its slot for another pass of the same event.
// slot / event_in / event_out: count entries each.  Returns the makespan in events (the largest event_out); throws
// std::invalid_argument for a non-positive count or width, a null array or a negative length.
int stream_schedule(int count, int width, const int *events, int *slot, int *event_in, int *event_out);

// What a stream call's arguments alone tell, refused in one place with one wording (the C entry asks before it looks at the solver,
// the solver again with the parameters it will really use): results and vectors present, count and width positive, max_iter a
// non-negative multiple of check_iter (below 1: 1).  Throws std::invalid_argument.
void stream_check_call(bool has_results, int count, int width, bool has_vectors, int max_iter, int check_iter);

}  // namespace hprlp
