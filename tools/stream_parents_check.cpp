// The queue with readiness and the schedule of a streamed batch with parents (hpr-lp-c_amd/csrc/stream_schedule.cpp; DESIGN.md
// "Streamed batches", "Parents") as a stand-alone host program, for a run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ihpr-lp-c_amd/csrc tools/stream_parents_check.cpp
//       hpr-lp-c_amd/csrc/stream_schedule.cpp -o build/stream_parents_check && build/stream_parents_check
// (one command line.)
// Every array has exactly the size the interface asks for, so that a write past an end is a sanitizer report.  The schedule is held
// to an event-by-event restatement of the rule on random forests (chains, binary trees, stars, all roots, random parents; zeros
// and ties among the lengths), with parent all -1 to stream_schedule itself; the queue's drop of a whole subtree and the refusals
// are exercised.  Needs no GPU and no HIP.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "stream_schedule.h"

using namespace hprlp;

namespace {

// the rule, one event at a time, with no heap: take out what ends, mark its children ready, give the free slots (ascending) to
// the ready problems (ascending), repeat while a new member ends at once
int restated(int count, int width, const std::vector<int> &ev, const std::vector<int> &parent, std::vector<int> &slot,
             std::vector<int> &ein, std::vector<int> &eout) {
    const int W = width < count ? width : count;
    std::vector<int> occ(W, -1), left(W, 0);
    std::vector<char> ready(count, 0), entered(count, 0);
    for (int p = 0; p < count; ++p) ready[p] = parent[p] < 0;
    int last = 0, ended = 0;
    for (int e = 0; ended < count; ++e) {
        bool again = true;
        while (again) {
            again = false;
            for (int k = 0; k < W; ++k)
                if (occ[k] >= 0 && left[k] == 0) {
                    const int p = occ[k];
                    eout[p] = e;
                    last = e;
                    ++ended;
                    occ[k] = -1;
                    for (int c = p + 1; c < count; ++c)
                        if (parent[c] == p) ready[c] = 1;
                }
            std::vector<int> fresh;
            int p = 0;
            for (int k = 0; k < W; ++k) {
                if (occ[k] >= 0) continue;
                while (p < count && !(ready[p] && !entered[p])) ++p;
                if (p == count) break;
                entered[p] = 1;
                slot[p] = k;
                ein[p] = e;
                fresh.push_back(k);
                left[k] = ev[p];
                again = again || ev[p] == 0;
                occ[k] = -2 - p;  // (not seen as occupied until the pass is over: a slot is given once per pass)
            }
            for (int k : fresh) occ[k] = -2 - occ[k];
        }
        bool any = false;
        for (int k = 0; k < W; ++k)
            if (occ[k] >= 0) {
                any = true;
                --left[k];
            }
        if (!any && ended < count) return -1;  // (the rule cannot get here: parent[p] < p)
    }
    return last;
}

bool refused(int count, int width, const int *ev, const int *parent, int *a, int *b, int *c) {
    try {
        (void)stream_schedule_parents(count, width, ev, parent, a, b, c);
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

int fail(const char *what, int a = 0, int b = 0, int c = 0) {
    std::printf("stream parents check: FAILED (%s; %d, %d, %d)\n", what, a, b, c);
    return 1;
}

}  // namespace

int main() {
    uint64_t state = 0x2545f4914f6cdd1dull;
    auto rnd = [&state](int mod) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return static_cast<int>((state >> 33) % static_cast<uint64_t>(mod));
    };
    int cases = 0;
    for (int rep = 0; rep < 3000; ++rep) {
        const int count = 1 + rnd(90), width = 1 + rnd(30), top = 1 + rnd(rep % 3 == 0 ? 2 : 12), shape = rep % 5;
        std::vector<int> ev(count), parent(count), s1(count), i1(count), o1(count), s2(count), i2(count), o2(count);
        for (int &v : ev) v = rnd(top + 1);
        const int chains = 1 + rnd(6);
        for (int p = 0; p < count; ++p) {
            if (shape == 0) parent[p] = p < chains ? -1 : p - chains;       // chains, numbered period by period
            else if (shape == 1) parent[p] = p == 0 ? -1 : (p - 1) / 2;     // one binary tree
            else if (shape == 2) parent[p] = p < chains ? -1 : p % chains;  // stars
            else if (shape == 3) parent[p] = -1;                            // all roots
            else parent[p] = rnd(p + 1) - 1;                                // a random forest
        }
        const int m1 = stream_schedule_parents(count, width, ev.data(), parent.data(), s1.data(), i1.data(), o1.data());
        const int m2 = restated(count, width, ev, parent, s2, i2, o2);
        if (m1 != m2 || s1 != s2 || i1 != i2 || o1 != o2) return fail("schedule against the restatement", count, width, rep);
        for (int p = 0; p < count; ++p) {
            if (o1[p] - i1[p] != ev[p]) return fail("a problem's length", count, width, rep);
            if (parent[p] >= 0 && i1[p] < o1[parent[p]]) return fail("a child before its parent's end", count, width, rep);
        }
        if (shape == 3) {
            const int m3 = stream_schedule(count, width, ev.data(), s2.data(), i2.data(), o2.data());
            if (m1 != m3 || s1 != s2 || i1 != i2 || o1 != o2) return fail("all roots against stream_schedule", count, width, rep);
        }
        ++cases;
    }
    {  // one chain: the makespan is the sum of the lengths whatever the width
        const std::vector<int> ev = {3, 0, 5, 1, 0, 0, 7}, parent = {-1, 0, 1, 2, 3, 4, 5};
        std::vector<int> s(7), i(7), o(7);
        for (int width : {1, 2, 7, 64})
            if (stream_schedule_parents(7, width, ev.data(), parent.data(), s.data(), i.data(), o.data()) != 16) return fail("a chain's makespan", width);
    }
    {  // the queue: ready problems ascending, as many as the free slots; an unusable parent drops its whole subtree
        const int parent[8] = {-1, -1, 0, 0, 2, 1, 4, 5};
        StreamParentQueue q(8, parent);
        const int slots[4] = {0, 3, 5, 6};
        std::vector<int> ps(4), pp(4);
        if (q.left() != 8 || stream_assign_parents(q, slots, 4, ps.data(), pp.data()) != 2 || ps[0] != 0 || pp[0] != 0 || ps[1] != 3 || pp[1] != 1 ||
            q.left() != 6 || stream_assign_parents(q, slots, 4, ps.data(), pp.data()) != 0)
            return fail("the roots");
        q.release(1, true);
        q.release(0, false);  // 2, 3, 4, 6 go for good
        if (q.left() != 2 || !q.dropped[2] || !q.dropped[3] || !q.dropped[4] || !q.dropped[6] || q.dropped[5] || q.dropped[7]) return fail("the drop");
        if (stream_assign_parents(q, slots, 1, ps.data(), pp.data()) != 1 || ps[0] != 0 || pp[0] != 5 || q.left() != 1) return fail("the child");
        q.release(5, true);
        if (stream_assign_parents(q, slots + 2, 2, ps.data(), pp.data()) != 1 || ps[0] != 5 || pp[0] != 7 || q.left() != 0) return fail("the grandchild");
    }
    const int ev[3] = {1, 2, 0}, neg[3] = {1, -1, 0}, ok[3] = {-1, 0, 0}, self[3] = {-1, 1, 0}, later[3] = {-1, 2, 0}, low[3] = {-1, -2, 0},
              first[3] = {0, -1, -1};
    int a[3], b[3], c[3];
    if (!refused(0, 1, ev, ok, a, b, c) || !refused(3, 0, ev, ok, a, b, c) || !refused(3, 1, nullptr, ok, a, b, c) ||
        !refused(3, 1, ev, nullptr, a, b, c) || !refused(3, 1, ev, ok, a, nullptr, c) || !refused(3, 1, neg, ok, a, b, c) ||
        !refused(3, 1, ev, self, a, b, c) || !refused(3, 1, ev, later, a, b, c) || !refused(3, 1, ev, low, a, b, c) ||
        !refused(3, 1, ev, first, a, b, c) || refused(3, 1, ev, ok, a, b, c))
        return fail("refusals");
    std::printf("stream parents check: ok (%d random cases)\n", cases);
    return 0;
}
