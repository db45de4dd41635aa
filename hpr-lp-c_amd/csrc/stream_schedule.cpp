// stream_schedule.cpp -- see stream_schedule.h.  Host only.
#include "stream_schedule.h"

#include <algorithm>
#include <functional>
#include <limits>
#include <utility>
#include <stdexcept>
#include <string>

namespace hprlp {

int stream_assign(StreamQueue &q, const int *freed, int nfreed, int *pair_slot, int *pair_problem) {
    int np = 0;
    for (int i = 0; i < nfreed && q.next < q.count; ++i) {
        pair_slot[np] = freed[i];
        pair_problem[np] = q.next++;
        ++np;
    }
    return np;
}

void stream_check_call(bool has_results, int count, int width, bool has_vectors, int max_iter, int check_iter) {
    if (!has_results) throw std::invalid_argument("batched stream: null results");
    if (count <= 0 || width <= 0) throw std::invalid_argument("batched stream: count and width must be positive");
    if (!has_vectors) throw std::invalid_argument("batched stream: null C / AL / AU / l / u");
    const int ci = std::max(check_iter, 1);
    if (max_iter < 0 || max_iter % ci != 0)
        throw std::invalid_argument("batched stream: max_iter (" + std::to_string(max_iter) + ") must be a multiple of check_iter (" +
                                    std::to_string(ci) + "): every member's last event is then a periodic event of the loop, where slots are handed on");
}

int stream_schedule(int count, int width, const int *events, int *slot, int *event_in, int *event_out) {
    if (count <= 0 || width <= 0) throw std::invalid_argument("stream schedule: count and width must be positive");
    if (!events || !slot || !event_in || !event_out) throw std::invalid_argument("stream schedule: null array");
    for (int p = 0; p < count; ++p)
        if (events[p] < 0) throw std::invalid_argument("stream schedule: a negative length");
    const int W = std::min(width, count);
    std::vector<int> occ(W, -1), freed(W), ps(W), pp(W);
    std::vector<long> end(W, 0);
    StreamQueue q;
    q.count = count;
    for (int k = 0; k < W; ++k) freed[k] = k;  // the initial fill: a refill pass of event 0 with every slot free
    int nfreed = W;
    long e = 0;
    while (true) {
        while (nfreed > 0) {  // the passes of event e
            const int np = stream_assign(q, freed.data(), nfreed, ps.data(), pp.data());
            for (int i = 0; i < np; ++i) {
                const int k = ps[i], p = pp[i];
                occ[k] = p;
                slot[p] = k;
                event_in[p] = static_cast<int>(e);
                end[k] = e + events[p];
            }
            nfreed = 0;
            for (int i = 0; i < np; ++i)  // only a member that has just entered can end within the same event (ps is ascending)
                if (end[ps[i]] == e) freed[nfreed++] = ps[i];
            for (int i = 0; i < nfreed; ++i) {
                event_out[occ[freed[i]]] = static_cast<int>(e);
                occ[freed[i]] = -1;
            }
        }
        long next = std::numeric_limits<long>::max();
        for (int k = 0; k < W; ++k)
            if (occ[k] >= 0) next = std::min(next, end[k]);
        if (next == std::numeric_limits<long>::max()) break;
        if (next > std::numeric_limits<int>::max()) throw std::invalid_argument("stream schedule: the schedule does not fit an int");
        e = next;
        for (int k = 0; k < W; ++k)
            if (occ[k] >= 0 && end[k] == e) {
                event_out[occ[k]] = static_cast<int>(e);
                occ[k] = -1;
                freed[nfreed++] = k;
            }
    }
    return static_cast<int>(e);
}

// ---- parents ------------------------------------------------------------------------------------------------------------------
void stream_check_parents(int count, const int *parent) {
    if (!parent) throw std::invalid_argument("batched stream: null parent");
    for (int p = 0; p < count; ++p)
        if (parent[p] < -1 || parent[p] >= p)
            throw std::invalid_argument("batched stream: parent[" + std::to_string(p) + "] = " + std::to_string(parent[p]) +
                                        " (-1 for a root, else a problem with a smaller number: 0 <= parent[p] < p)");
}

void stream_check_parents_call(const int *parent, bool has_x0, bool has_y0) {
    if (!parent) throw std::invalid_argument("batched stream: null parent");
    if (has_x0 != has_y0)
        throw std::invalid_argument(std::string("batched stream: with parents X0 and Y0 come together or not at all (") +
                                    (has_x0 ? "Y0" : "X0") + " is null): a root starts from both of its columns or is a cold member");
}

StreamParentQueue::StreamParentQueue(int count_, const int *parent) : count(count_), waiting(count_) {
    stream_check_parents(count, parent);
    child_first.assign(static_cast<size_t>(count) + 1, 0);
    for (int p = 0; p < count; ++p)
        if (parent[p] >= 0) ++child_first[parent[p] + 1];
    for (int p = 0; p < count; ++p) child_first[p + 1] += child_first[p];
    child.resize(child_first[count]);
    std::vector<int> at(child_first.begin(), child_first.end() - 1);
    for (int p = 0; p < count; ++p) {  // (ascending p: every list comes out ascending)
        if (parent[p] >= 0) child[at[parent[p]]++] = p;
        else ready.push_back(p);  // (ascending numbers are a min-heap as they stand)
    }
    dropped.assign(count, 0);
}

void StreamParentQueue::release(int p, bool usable) {
    if (usable) {
        for (int i = child_first[p]; i < child_first[p + 1]; ++i) {
            ready.push_back(child[i]);
            std::push_heap(ready.begin(), ready.end(), std::greater<int>());
        }
        return;
    }
    std::vector<int> todo(child.begin() + child_first[p], child.begin() + child_first[p + 1]);
    while (!todo.empty()) {  // every descendant, each once: a problem has one parent
        const int c = todo.back();
        todo.pop_back();
        dropped[c] = 1;
        --waiting;
        todo.insert(todo.end(), child.begin() + child_first[c], child.begin() + child_first[c + 1]);
    }
}

int stream_assign_parents(StreamParentQueue &q, const int *free_slots, int nfree, int *pair_slot, int *pair_problem) {
    int np = 0;
    for (int i = 0; i < nfree && !q.ready.empty(); ++i) {
        std::pop_heap(q.ready.begin(), q.ready.end(), std::greater<int>());
        pair_slot[np] = free_slots[i];
        pair_problem[np] = q.ready.back();
        q.ready.pop_back();
        --q.waiting;
        ++np;
    }
    return np;
}

int stream_schedule_parents(int count, int width, const int *events, const int *parent, int *slot, int *event_in, int *event_out) {
    if (count <= 0 || width <= 0) throw std::invalid_argument("stream schedule: count and width must be positive");
    if (!events || !slot || !event_in || !event_out) throw std::invalid_argument("stream schedule: null array");
    for (int p = 0; p < count; ++p)
        if (events[p] < 0) throw std::invalid_argument("stream schedule: a negative length");
    StreamParentQueue q(count, parent);
    const int W = std::min(width, count);
    // the running members as a min-heap of (the event at which the member ends, its slot); the free slots as a min-heap of numbers
    using Run = std::pair<long, int>;
    std::vector<Run> running;
    std::vector<int> free_heap(W), occ(W, -1), freed, ps(W), pp(W);
    for (int k = 0; k < W; ++k) free_heap[k] = k;  // the initial fill: a pass of event 0 with every slot free (ascending: a min-heap)
    long e = 0;
    bool pass = true;  // (of event 0: the initial fill)
    while (true) {
        while (pass) {  // the passes of event e
            freed.clear();  // the free slots this pass can use, ascending: as many as there are ready problems
            while (!free_heap.empty() && freed.size() < q.ready.size()) {
                std::pop_heap(free_heap.begin(), free_heap.end(), std::greater<int>());
                freed.push_back(free_heap.back());
                free_heap.pop_back();
            }
            const int np = stream_assign_parents(q, freed.data(), static_cast<int>(freed.size()), ps.data(), pp.data());
            pass = false;
            for (int i = 0; i < np; ++i) {
                const int k = ps[i], p = pp[i];
                slot[p] = k;
                event_in[p] = static_cast<int>(e);
                if (events[p] > 0) {
                    occ[k] = p;
                    running.emplace_back(e + events[p], k);
                    std::push_heap(running.begin(), running.end(), std::greater<Run>());
                    continue;
                }
                event_out[p] = static_cast<int>(e);  // a member of length 0: its slot is free again and its children are ready,
                q.release(p, true);                  // for another pass of this event
                free_heap.push_back(k);
                std::push_heap(free_heap.begin(), free_heap.end(), std::greater<int>());
                pass = true;
            }
        }
        if (running.empty()) break;
        if (running.front().first > std::numeric_limits<int>::max()) throw std::invalid_argument("stream schedule: the schedule does not fit an int");
        e = running.front().first;
        while (!running.empty() && running.front().first == e) {  // every member that ends at event e, before the event's first pass
            std::pop_heap(running.begin(), running.end(), std::greater<Run>());
            const int k = running.back().second, p = occ[k];
            running.pop_back();
            event_out[p] = static_cast<int>(e);
            occ[k] = -1;
            q.release(p, true);
            free_heap.push_back(k);
            std::push_heap(free_heap.begin(), free_heap.end(), std::greater<int>());
        }
        pass = true;
    }
    // parent[p] < p: with nothing running the lowest-numbered waiting problem is ready, so the loop above ends with nobody waiting
    if (q.left() != 0) throw std::logic_error("stream schedule: problems left waiting with nothing running");
    return static_cast<int>(e);
}

}  // namespace hprlp
