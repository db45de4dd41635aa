// stream_schedule.cpp -- see stream_schedule.h.  Host only.
#include "stream_schedule.h"

#include <algorithm>
#include <limits>
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

}  // namespace hprlp
