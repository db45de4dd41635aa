// stream_schedule.h -- which queued problem enters which slot of a streamed batch, and when (DESIGN.md "Streamed batches").
// Plain host code: no HIP header, no device call.  The streamed loop of batched.hip takes its slot decisions from stream_assign;
// stream_schedule plays the same rule forward from each problem's length, so that the loop's record can be held to it without a
// GPU (hprlp_stream_schedule_host, tests/test_batched_stream.py), and tools/stream_schedule_check.cpp runs both under the host
// sanitizers.  A call with parents has the same three beside them: StreamParentQueue / stream_assign_parents,
// stream_schedule_parents (tests/test_batched_stream_parents.py) and tools/stream_parents_check.cpp.
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

// ---- parents (DESIGN.md "Streamed batches", "Parents") ---------------------------------------------------------------------------
// parent[p] == -1: p is a root; else 0 <= parent[p] < p and p starts from what problem parent[p] returned.  Throws
// std::invalid_argument for a null array or any other value; the message names p and the value.
void stream_check_parents(int count, const int *parent);

// The problems of a parents call that have not entered a slot yet.  p is READY when it is a root or its parent has been released
// (harvested); the ready ones wait in a heap, smallest number first.  release(p, usable) is called once for every problem that
// ends, before the pass that follows its harvest is assigned: its children become ready, or -- usable false: p's returned point
// cannot start anybody -- they and all their descendants are dropped for good and listed in `dropped`.
struct StreamParentQueue {
    int count = 0, waiting = 0;            // waiting: neither entered nor dropped
    std::vector<int> child_first, child;  // the children of p: child[child_first[p] .. child_first[p + 1]), ascending
    std::vector<int> ready;               // a min-heap (std::push_heap with std::greater)
    std::vector<char> dropped;
    StreamParentQueue() = default;
    StreamParentQueue(int count, const int *parent);  // (checks the array: stream_check_parents)
    int left() const { return waiting; }
    void release(int p, bool usable);
};

// One refill pass of a parents call: the FREE slots -- every slot without a member, those just harvested and those that stood
// empty -- in ascending order take the READY problems in ascending problem number, as many as both last.  free_slots: nfree slot
// numbers, ascending.  pair_slot / pair_problem: room for nfree entries; they come out ordered by slot.  Returns the number of pairs.
int stream_assign_parents(StreamParentQueue &q, const int *free_slots, int nfree, int *pair_slot, int *pair_problem);

// stream_schedule with parents: the same rule played forward, a problem entering no sooner than its parent's event_out (a parent
// of length 0 frees its children for the next pass of the same event).  The initial fill is a pass of event 0 with every slot free,
// in which only roots are ready.  With parent all -1 the arrays and the makespan are stream_schedule's.  O(count log count).
int stream_schedule_parents(int count, int width, const int *events, const int *parent, int *slot, int *event_in, int *event_out);

// What a stream call's arguments alone tell, refused in one place with one wording (the C entry asks before it looks at the solver,
// the solver again with the parameters it will really use): results and vectors present, count and width positive, max_iter a
// non-negative multiple of check_iter (below 1: 1).  Throws std::invalid_argument.
void stream_check_call(bool has_results, int count, int width, bool has_vectors, int max_iter, int check_iter);
// ... and what a parents call adds to it: a parent array, and X0 / Y0 given together or not at all -- a root starts from both of
// its own columns or is a cold member.  The C entry asks this before it looks at the solver; the array's VALUES
// (stream_check_parents) are the solver's to refuse, before anything changes and without a device call: a NULL handle with any
// array at all is still "null solver".
void stream_check_parents_call(const int *parent, bool has_x0, bool has_y0);

}  // namespace hprlp
