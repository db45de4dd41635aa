// group_table.cpp -- stage order, table block and launch list of a group recording, and its self-test (group_table.h).  Host only.
#include "group_table.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace hprlp {

GroupTable::GroupTable(bool own_launches, int reduce_blocks, int threads) : own_(own_launches), reduce_blocks_(reduce_blocks), threads_(threads) {}

void GroupTable::note(int kind) { present_.back() |= uint64_t(1) << kind; }

void GroupTable::next_stage() {
    if (present_.back() == 0) return;
    order_.push_back(open_stage());
    present_.push_back(0);
}

void GroupTable::repeat_last(int nseg, int times) {
    if (nseg <= 0 || static_cast<size_t>(nseg) > order_.size()) throw std::invalid_argument("group launches: repeat of stages that were not recorded");
    const std::vector<int> tail(order_.end() - nseg, order_.end());
    for (int t = 1; t < times; ++t) order_.insert(order_.end(), tail.begin(), tail.end());
}

static int bits(uint64_t v) {
    int n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}

int GroupTable::recorded_launches() const {
    int n = bits(present_.back());
    for (int i : order_) n += bits(present_[i]);
    return n;
}

void GroupTable::begin() {
    next_stage();  // (what is open is part of this run)
    bytes_.clear();
    made_.clear();
    first_.assign(present_.size() + 1, 0);
}

size_t GroupTable::put(const void *p, size_t n) {
    const size_t at = (bytes_.size() + kTableAlign - 1) / kTableAlign * kTableAlign;
    bytes_.resize(at + n);
    if (n > 0) std::memcpy(bytes_.data() + at, p, n);
    return at;
}

size_t GroupTable::put_map(const int *grids, int ntasks, int *nwg) {
    int total = 0;
    for (int t = 0; t < ntasks; ++t) total += std::max(grids[t], 0);
    *nwg = total;
    const size_t at = (bytes_.size() + kTableAlign - 1) / kTableAlign * kTableAlign;
    bytes_.resize(at + static_cast<size_t>(total) * 2 * sizeof(int));
    int *pair = reinterpret_cast<int *>(bytes_.data() + at);  // (written in place: the block's storage is aligned for any scalar)
    for (int t = 0; t < ntasks; ++t)
        for (int lb = 0; lb < grids[t]; ++lb) {
            *pair++ = t;
            *pair++ = lb;
        }
    return at;
}

void GroupTable::add(int stage, int kind, GridRule rule, const void *tasks, size_t task_bytes, int ntasks, const int *grids, bool own) {
    if (ntasks <= 0) return;
    GroupLaunch l{kind, stage, ntasks, 0, 0, 0, own_ && own};
    if (!l.own) {
        l.tasks = put(tasks, task_bytes * static_cast<size_t>(ntasks));
        switch (rule) {
            case kGridMapped: l.map = put_map(grids, ntasks, &l.nwg); break;
            case kGridReduce: l.nwg = ntasks * reduce_blocks_; break;
            case kGridPerTask: l.nwg = ntasks; break;
            case kGridPerThread: l.nwg = (ntasks + threads_ - 1) / threads_; break;
        }
        if (l.nwg <= 0) return;  // (members' grids that are all empty: nothing to launch)
    }
    // (stages come in ascending order: a stage's launches are one range of made_, ending where the next one's begin)
    made_.push_back(l);
    for (size_t i = static_cast<size_t>(stage) + 1; i < first_.size(); ++i) first_[i] = made_.size();
}

const std::vector<GroupLaunch> &GroupTable::finish() {
    list_.clear();  // (the vectors of a run keep their capacity: no allocation per run once they have grown)
    for (int i : order_) list_.insert(list_.end(), made_.begin() + first_[i], made_.begin() + first_[i + 1]);
    present_.assign(1, 0);
    order_.clear();
    return list_;
}

int group_iteration_plan(const int *counts, int n, std::vector<int> &len, std::vector<int> &min_count) {
    std::vector<int> c;
    for (int k = 0; k < n; ++k)
        if (counts[k] > 0) c.push_back(counts[k]);
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    int before = 0;
    for (int v : c) {
        len.push_back(v - before);
        min_count.push_back(v);
        before = v;
    }
    return static_cast<int>(c.size());
}

}  // namespace hprlp

extern "C" int hprlp_group_iteration_plan(const int *counts, int n, int *seg_len, int *seg_min_count, int cap) {
    if (n < 0 || cap < 0 || (n > 0 && !counts) || (cap > 0 && (!seg_len || !seg_min_count))) return -1;
    for (int k = 0; k < n; ++k)
        if (counts[k] < 0) return -1;
    std::vector<int> len, min_count;
    const int segs = hprlp::group_iteration_plan(counts, n, len, min_count);
    if (segs > cap) return -1;
    for (int j = 0; j < segs; ++j) seg_len[j] = len[j], seg_min_count[j] = min_count[j];
    return segs;
}

// Checks, numbered: 1 every table and map offset is a multiple of 16; 2 tables and maps do not overlap and lie inside the block;
// 3 grids {3, 0, 2} give the map (0,0) (0,1) (0,2) (2,0) (2,1) and 5 workgroups; 4 a kind with one task takes no table under the
// own-launch rule and one without it; 5 repeat_last(2, 20) over stages s, t issues s t s t ... (40 launches) from one table each;
// 6 the launch list is as long as recorded_launches() says, for two stages that hold the same kind; 7 an empty trailing stage adds
// nothing; 8 the grid rules' workgroup counts; 9 a repeat of stages that were not recorded is refused; 10 the shape of a periodic
// round with detection (a check step's stage, then the evaluation's stage with the three ray kinds, one of them a lone member's):
// the launches of the second stage do not depend on the number of tasks, a lone task goes its own way only where its kind says so,
// and the kinds of a stage are issued in ascending order (the form ahead of the two products that gather what it writes); 11 the
// check stage of a group's device entries (the check of the members' vectors and, for new matrix values, the check of the values:
// two mapped kinds with one task per member in ONE stage): two launches whatever the number of members, on the sum of the
// members' own grids, and a group of one issues the member's own two launches and sends no table; 12 group_iteration_plan: counts
// {7, 6, 0, 7, 149} give the segments 6, 1, 142 at 6, 7, 149, every member is in the first segments without a gap and their lengths
// add up to its count, and counts that are all zero give no segment; 13 the normal iterations of wide members: per segment the
// x-half's stage and the y-half's stage repeated `len` times from one table each, a segment with one member as its own launches,
// the check step's stage behind them.
extern "C" int hprlp_group_table_selftest(void) {
    using namespace hprlp;
    struct Task {
        double a;
        int n;
    };  // (16 bytes; the odd table lengths below come from the 12-byte one)
    struct Odd {
        int a, b, c;
    };
    const Task t3[3] = {{1.0, 3}, {2.0, 0}, {3.0, 2}};
    const Odd o5[5] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}, {10, 11, 12}, {13, 14, 15}};
    const int grids[3] = {3, 0, 2};
    enum { kA = 0, kB = 1, kC = 2, kD = 3 };
    {   // ---- 1, 2, 3, 6, 7, 8: two stages, kind kA in both
        GroupTable g(true, 512, 256);
        g.note(kA), g.note(kB), g.note(kC);
        g.next_stage();
        g.note(kA), g.note(kD);
        g.next_stage();
        g.next_stage();  // (nothing open: no new stage)
        if (g.open_stage() != 2) return 7;
        const int want = g.recorded_launches();
        if (want != 5) return 6;
        g.begin();
        g.add(0, kA, kGridMapped, t3, sizeof(Task), 3, grids, false);
        g.add(0, kB, kGridReduce, o5, sizeof(Odd), 5, nullptr, false);
        g.add(0, kC, kGridPerThread, o5, sizeof(Odd), 5, nullptr, false);
        g.add(1, kA, kGridMapped, t3, sizeof(Task), 3, grids, false);
        g.add(1, kD, kGridPerTask, o5, sizeof(Odd), 3, nullptr, false);
        const size_t block = g.bytes().size();
        const std::vector<char> bytes = g.bytes();
        const std::vector<GroupLaunch> list = g.finish();
        if (static_cast<int>(list.size()) != want) return 6;
        if (g.recorded_launches() != 0 || g.open_stage() != 0) return 7;
        struct Range {
            size_t at, len;
        };
        std::vector<Range> r;
        for (const GroupLaunch &l : list) {
            if (l.own) return 4;
            if (l.tasks % kTableAlign != 0 || l.map % kTableAlign != 0) return 1;
            r.push_back({l.tasks, static_cast<size_t>(l.ntasks) * (l.kind == kA ? sizeof(Task) : sizeof(Odd))});
            if (l.kind == kA) r.push_back({l.map, static_cast<size_t>(l.nwg) * 2 * sizeof(int)});
        }
        for (const Range &e : r)
            if (e.at + e.len > block) return 2;
        std::sort(r.begin(), r.end(), [](const Range &a, const Range &c) { return a.at < c.at; });
        for (size_t i = 1; i < r.size(); ++i)
            if (r[i - 1].at + r[i - 1].len > r[i].at) return 2;
        const int want_map[10] = {0, 0, 0, 1, 0, 2, 2, 0, 2, 1};
        for (const GroupLaunch &l : list) {
            if (l.kind != kA) continue;
            if (l.nwg != 5 || std::memcmp(bytes.data() + l.map, want_map, sizeof(want_map)) != 0) return 3;
            if (std::memcmp(bytes.data() + l.tasks, t3, sizeof(t3)) != 0) return 3;
        }
        if (list[0].kind != kA || list[0].stage != 0 || list[3].kind != kA || list[3].stage != 1) return 6;
        if (list[1].nwg != 5 * 512 || list[2].nwg != 1 || list[4].nwg != 3) return 8;
    }
    for (int own_rule = 0; own_rule < 2; ++own_rule) {  // ---- 4: one task, with a launch of the member's own
        GroupTable g(own_rule != 0, 512, 256);
        g.note(kA);
        g.begin();
        g.add(0, kA, kGridMapped, t3, sizeof(Task), 1, grids, true);
        g.add(0, kB, kGridReduce, o5, sizeof(Odd), 1, nullptr, false);  // (no launch of its own: a table under either rule)
        const size_t block = g.bytes().size();
        const std::vector<GroupLaunch> list = g.finish();
        if (list.size() != 2 || list[0].own != (own_rule != 0) || list[1].own) return 4;
        if (own_rule ? block != sizeof(Odd) : block != 16 + 3 * 2 * sizeof(int) + 8 + sizeof(Odd)) return 4;
        if (!own_rule && list[0].nwg != 3) return 4;
    }
    {   // ---- 5, 9: the Curtis-Reid sweeps' shape
        GroupTable g(false, 512, 256);
        bool refused = false;
        try {
            g.repeat_last(1, 2);
        } catch (const std::invalid_argument &) {
            refused = true;
        }
        if (!refused) return 9;
        g.note(kA);
        g.next_stage();
        g.note(kA);
        g.next_stage();
        g.repeat_last(2, 20);
        g.note(kB);
        if (g.recorded_launches() != 41) return 5;
        g.begin();
        g.add(0, kA, kGridMapped, t3, sizeof(Task), 3, grids, false);
        g.add(1, kA, kGridMapped, t3, sizeof(Task), 1, grids, false);
        g.add(2, kB, kGridPerTask, o5, sizeof(Odd), 5, nullptr, false);
        const std::vector<GroupLaunch> list = g.finish();
        if (list.size() != 41) return 5;
        for (int i = 0; i < 40; ++i)
            if (list[i].stage != i % 2 || list[i].tasks != list[i % 2].tasks || list[i].map != list[i % 2].map) return 5;
        if (list[0].tasks == list[1].tasks || list[40].stage != 2) return 5;
    }
    for (int members = 1; members <= 5; members += 4) {  // ---- 10
        enum { kX = 0, kRd = 1, kForm = 2, kCol = 3, kRow = 4, kFin = 5 };
        GroupTable g(true, 512, 256);
        g.note(kX), g.note(kFin);
        g.next_stage();
        g.note(kRd), g.note(kForm), g.note(kCol), g.note(kRow), g.note(kFin);
        if (g.recorded_launches() != 7) return 10;
        g.begin();
        const int gr[5] = {1, 3, 2, 1, 5};
        const bool lone = members == 1;  // (what the recorder says of a kind with a launch of the member's own: one task)
        g.add(0, kX, kGridMapped, o5, sizeof(Odd), members, gr, lone);
        g.add(0, kFin, kGridPerTask, o5, sizeof(Odd), members, nullptr, false);
        g.add(1, kRd, kGridMapped, o5, sizeof(Odd), members, gr, lone);
        g.add(1, kForm, kGridReduce, o5, sizeof(Odd), members, nullptr, lone);
        g.add(1, kCol, kGridMapped, o5, sizeof(Odd), 1, gr, true);   // (one member has a previous iterate: a lone task)
        g.add(1, kRow, kGridMapped, o5, sizeof(Odd), 1, gr, false);  // (a kind without a launch of the member's own)
        g.add(1, kFin, kGridPerTask, o5, sizeof(Odd), members, nullptr, false);
        const std::vector<GroupLaunch> list = g.finish();
        if (list.size() != 7) return 10;
        for (size_t i = 1; i < list.size(); ++i)
            if (list[i].stage < list[i - 1].stage || (list[i].stage == list[i - 1].stage && list[i].kind <= list[i - 1].kind)) return 10;
        if (list[3].kind != kForm || list[3].own != (members == 1) || (!list[3].own && list[3].nwg != members * 512)) return 10;
        if (!list[4].own || list[5].own || list[5].nwg != 1) return 10;
    }
    for (int members = 1; members <= 5; members += 4) {  // ---- 11
        enum { kDataCheck = 0, kValuesCheck = 1 };
        GroupTable g(true, 512, 256);
        g.note(kDataCheck), g.note(kValuesCheck);
        if (g.recorded_launches() != 2) return 11;
        g.begin();
        const int gr[5] = {1, 1, 2, 1, 3};
        const bool lone = members == 1;
        g.add(0, kDataCheck, kGridMapped, o5, sizeof(Odd), members, gr, lone);
        g.add(0, kValuesCheck, kGridMapped, o5, sizeof(Odd), members, gr, lone);
        const size_t block = g.bytes().size();
        const std::vector<GroupLaunch> list = g.finish();
        if (list.size() != 2 || list[0].kind != kDataCheck || list[1].kind != kValuesCheck || list[0].stage != 0 || list[1].stage != 0) return 11;
        if (list[0].own != lone || list[1].own != lone || (lone ? block != 0 : block == 0)) return 11;
        if (!lone && (list[0].nwg != 8 || list[1].nwg != 8 || list[0].ntasks != 5 || list[0].tasks == list[1].tasks)) return 11;
    }
    {   // ---- 12, 13
        const int counts[5] = {7, 6, 0, 7, 149};
        std::vector<int> len, at;
        if (group_iteration_plan(counts, 5, len, at) != 3) return 12;
        const int want_len[3] = {6, 1, 142}, want_at[3] = {6, 7, 149};
        for (int j = 0; j < 3; ++j)
            if (len[j] != want_len[j] || at[j] != want_at[j]) return 12;
        for (int k = 0; k < 5; ++k) {  // (a member's segments are the first ones, without a gap, and add up to its count)
            int sum = 0;
            bool out = false;
            for (int j = 0; j < 3; ++j) {
                const bool in = counts[k] >= at[j];
                if (in && out) return 12;
                out = !in;
                if (in) sum += len[j];
            }
            if (sum != counts[k]) return 12;
        }
        len.clear(), at.clear();
        const int none[2] = {0, 0};
        if (group_iteration_plan(none, 2, len, at) != 0 || !len.empty()) return 12;
        // the two stages of a segment's iteration (x-half, y-half: each kind alone in its stage) issued len times from one table
        // each, segment after segment, with the check step's stage behind them
        enum { kXn = 0, kYn = 1, kXc = 2 };
        GroupTable g(true, 512, 256);
        const int seg_len[2] = {6, 1};
        for (int j = 0; j < 2; ++j) {
            g.note(kXn);
            g.next_stage();
            g.note(kYn);
            g.next_stage();
            g.repeat_last(2, seg_len[j]);
        }
        g.note(kXc);
        if (g.recorded_launches() != 2 * 7 + 1) return 13;
        g.begin();
        const int gr[2] = {3, 2};
        const Odd o2[2] = {{1, 2, 3}, {4, 5, 6}};
        g.add(0, kXn, kGridMapped, o2, sizeof(Odd), 2, gr, false);
        g.add(1, kYn, kGridMapped, o2, sizeof(Odd), 2, gr, false);
        g.add(2, kXn, kGridMapped, o2, sizeof(Odd), 1, gr, true);  // (the second segment holds one member: its own launches)
        g.add(3, kYn, kGridMapped, o2, sizeof(Odd), 1, gr, true);
        g.add(4, kXc, kGridMapped, o2, sizeof(Odd), 2, gr, false);
        const std::vector<GroupLaunch> list = g.finish();
        if (list.size() != 15) return 13;
        for (int i = 0; i < 12; ++i)
            if (list[i].stage != i % 2 || list[i].own || list[i].nwg != 5 || list[i].tasks != list[i % 2].tasks) return 13;
        if (list[12].stage != 2 || !list[12].own || list[13].stage != 3 || !list[13].own || list[14].stage != 4 || list[14].own) return 13;
    }
    return 0;
}
