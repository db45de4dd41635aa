// The schedule of a streamed batch (hpr-lp-c_amd/csrc/stream_schedule.cpp; DESIGN.md "Streamed batches") as a stand-alone host
// program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ihpr-lp-c_amd/csrc tools/stream_schedule_check.cpp
//       hpr-lp-c_amd/csrc/stream_schedule.cpp -o build/stream_schedule_check && build/stream_schedule_check
// (one command line.)
// Every array has exactly the size the interface asks for, so that a write past an end is a sanitizer report.  The schedule is
// held to an event-by-event restatement of the rule on random lengths (zeros and ties included), to the figures DESIGN.md quotes,
// and the refusals are exercised.  Needs no GPU and no HIP.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "stream_schedule.h"

using namespace hprlp;

namespace {

// the rule, one event at a time: harvest what ends, refill ascending, repeat while a new member ends at once
int restated(int count, int width, const std::vector<int> &ev, std::vector<int> &slot, std::vector<int> &ein, std::vector<int> &eout) {
    const int W = width < count ? width : count;
    std::vector<int> occ(W, -1), left(W, 0);
    int next = 0, last = 0;
    for (int k = 0; k < W; ++k) {
        occ[k] = next;
        slot[next] = k;
        ein[next] = 0;
        left[k] = ev[next++];
    }
    for (int e = 0;; ++e) {
        bool again = true, any = false;
        while (again) {
            again = false;
            for (int k = 0; k < W; ++k)
                if (occ[k] >= 0 && left[k] == 0) {
                    eout[occ[k]] = e;
                    last = e;
                    occ[k] = -2;  // freed in this pass
                }
            for (int k = 0; k < W; ++k)
                if (occ[k] == -2) {
                    occ[k] = -1;
                    if (next < count) {
                        occ[k] = next;
                        slot[next] = k;
                        ein[next] = e;
                        left[k] = ev[next++];
                        again = again || left[k] == 0;
                    }
                }
        }
        for (int k = 0; k < W; ++k)
            if (occ[k] >= 0) {
                any = true;
                --left[k];
            }
        if (!any) return last;
    }
}

bool refused(int count, int width, const int *ev, int *a, int *b, int *c) {
    try {
        (void)stream_schedule(count, width, ev, a, b, c);
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

}  // namespace

int main() {
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&state](int mod) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return static_cast<int>((state >> 33) % static_cast<uint64_t>(mod));
    };
    int cases = 0;
    for (int rep = 0; rep < 2000; ++rep) {
        const int count = 1 + rnd(70), width = 1 + rnd(24), top = 1 + rnd(rep % 3 == 0 ? 3 : 15);
        std::vector<int> ev(count), s1(count), i1(count), o1(count), s2(count), i2(count), o2(count);
        for (int &v : ev) v = rnd(top + 1);
        const int m1 = stream_schedule(count, width, ev.data(), s1.data(), i1.data(), o1.data());
        const int m2 = restated(count, width, ev, s2, i2, o2);
        if (m1 != m2 || s1 != s2 || i1 != i2 || o1 != o2) {
            std::printf("stream schedule check: FAILED (count %d, width %d, case %d)\n", count, width, rep);
            return 1;
        }
        ++cases;
    }
    {  // the 24 lengths DESIGN.md quotes: 121 events through 8 slots
        const std::vector<int> ev = {21, 25, 46, 59, 30, 34, 26, 27, 65, 38, 17, 33, 21, 32, 19, 37, 37, 14, 22, 24, 52, 55, 32, 38};
        std::vector<int> s(24), i(24), o(24);
        if (stream_schedule(24, 8, ev.data(), s.data(), i.data(), o.data()) != 121) {
            std::printf("stream schedule check: FAILED (the quoted makespan)\n");
            return 1;
        }
    }
    {  // stream_assign stops at the shorter of the two lists
        StreamQueue q;
        q.count = 5;
        q.next = 3;
        const int freed[4] = {1, 4, 6, 7};
        std::vector<int> ps(4), pp(4);
        if (stream_assign(q, freed, 4, ps.data(), pp.data()) != 2 || ps[0] != 1 || pp[0] != 3 || ps[1] != 4 || pp[1] != 4 || q.left() != 0 ||
            stream_assign(q, freed, 4, ps.data(), pp.data()) != 0) {
            std::printf("stream schedule check: FAILED (stream_assign)\n");
            return 1;
        }
    }
    int ev[2] = {1, 2}, neg[2] = {1, -1}, a[2], b[2], c[2];
    if (!refused(0, 1, ev, a, b, c) || !refused(2, 0, ev, a, b, c) || !refused(2, 1, nullptr, a, b, c) || !refused(2, 1, ev, a, nullptr, c) ||
        !refused(2, 1, neg, a, b, c) || refused(2, 1, ev, a, b, c)) {
        std::printf("stream schedule check: FAILED (refusals)\n");
        return 1;
    }
    std::printf("stream schedule check: ok (%d random cases)\n", cases);
    return 0;
}
