// group_pack.cpp -- the packing layout of a group call's staging and result blocks and its self-test (group_pack.h).  Host only.
#include "group_pack.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace hprlp {

namespace {
size_t take(size_t &at, size_t len) {
    if (len == 0) return kPackAbsent;
    const size_t here = at;
    at += (len + kPackAlign - 1) / kPackAlign * kPackAlign;
    return here;
}
void put(double *block, size_t at, const double *src, size_t len) {
    if (at != kPackAbsent && src && len > 0) std::memcpy(block + at, src, sizeof(double) * len);
}
}  // namespace

GroupPackLayout group_pack_layout(const PackMember *members, int count) {
    GroupPackLayout L;
    L.slot.resize(static_cast<size_t>(std::max(count, 0)));
    for (int k = 0; k < count; ++k) {
        const PackMember &mb = members[k];
        PackSlot &s = L.slot[k];
        const size_t m = static_cast<size_t>(std::max(mb.m, 0)), n = static_cast<size_t>(std::max(mb.n, 0));
        // the order of Solver::set_matrix_values' staging, [val | AL | AU | l | u | c]; without values Solver::set_data's
        if (mb.nnz > 0) s.val = take(L.data_doubles, static_cast<size_t>(mb.nnz));
        if (mb.bounds) {
            s.AL = take(L.data_doubles, m);
            s.AU = take(L.data_doubles, m);
            s.l = take(L.data_doubles, n);
            s.u = take(L.data_doubles, n);
        }
        if (mb.c) s.c = take(L.data_doubles, n);
        if (mb.x0) s.x0 = take(L.start_doubles, n);
        if (mb.y0) s.y0 = take(L.start_doubles, m);
        if (mb.result) {
            s.x = take(L.result_doubles, n);
            s.y = take(L.result_doubles, m);
            s.z = take(L.result_doubles, n);
        }
        if (mb.cert == 1) {
            s.cert_rn = take(L.cert_doubles, m);
            s.cert_cn = take(L.cert_doubles, n);
            s.cert_ray = take(L.cert_doubles, m);
            s.cert_aty = take(L.cert_doubles, n);
        } else if (mb.cert == 2) {
            s.cert_cn = take(L.cert_doubles, n);
            s.cert_ray = take(L.cert_doubles, n);
        }
    }
    return L;
}

void group_pack_data(const GroupPackLayout &L, int k, const PackMember &mb, const double *AL, const double *AU, const double *l, const double *u,
                     const double *c, double *block) {
    const PackSlot &s = L.slot[static_cast<size_t>(k)];
    const size_t m = static_cast<size_t>(std::max(mb.m, 0)), n = static_cast<size_t>(std::max(mb.n, 0));
    put(block, s.AL, AL, m);
    put(block, s.AU, AU, m);
    put(block, s.l, l, n);
    put(block, s.u, u, n);
    put(block, s.c, c, n);
}

void group_pack_values(const GroupPackLayout &L, int k, const PackMember &mb, const double *val, double *block) {
    put(block, L.slot[static_cast<size_t>(k)].val, val, static_cast<size_t>(std::max<long>(mb.nnz, 0)));
}

void group_pack_start(const GroupPackLayout &L, int k, const PackMember &mb, const double *x0, const double *y0, double *block) {
    const PackSlot &s = L.slot[static_cast<size_t>(k)];
    put(block, s.x0, x0, static_cast<size_t>(std::max(mb.n, 0)));
    put(block, s.y0, y0, static_cast<size_t>(std::max(mb.m, 0)));
}

void group_unpack_result(const GroupPackLayout &L, int k, const PackMember &mb, const double *block, double *x, double *y, double *z) {
    const PackSlot &s = L.slot[static_cast<size_t>(k)];
    const size_t m = static_cast<size_t>(std::max(mb.m, 0)), n = static_cast<size_t>(std::max(mb.n, 0));
    if (s.x != kPackAbsent && x) std::memcpy(x, block + s.x, sizeof(double) * n);
    if (s.y != kPackAbsent && y) std::memcpy(y, block + s.y, sizeof(double) * m);
    if (s.z != kPackAbsent && z) std::memcpy(z, block + s.z, sizeof(double) * n);
}

}  // namespace hprlp

// Checks, numbered: 1 absent vectors take no room and have no offset; 2 every range lies inside its block; 3 the ranges of a block
// are disjoint; 4 offsets are aligned; 5 a pack / unpack round trip of the data and start blocks returns what went in and leaves
// the padding alone; 6 the result round trip; 7 an empty group and members of size zero; 8 matrix values (set_matrix_values_many):
// a member's values lie in front of its vectors in the order [val | AL | AU | l | u | c], aligned, disjoint from everything else
// and inside the block, odd, even and single counts, a member with values and no vectors; the round trip leaves the padding alone;
// 9 certificates (loop_many): kind 1 takes [row_norm (m) | col_norm (n) | ray (m) | A^T y (n)], kind 2 [col_norm (n) | ray (n)],
// kind 0 nothing, in member order without gaps but the padding, aligned, disjoint, inside the block, and in no other block.
extern "C" int hprlp_group_pack_selftest(void) {
    using namespace hprlp;
    // odd sizes, sizes below and at the alignment, every combination of given / absent
    std::vector<PackMember> mem;
    const int sizes[][2] = {{1, 1}, {3, 5}, {31, 33}, {32, 64}, {120, 200}, {300, 500}, {0, 7}, {7, 0}};
    int combo = 0;
    for (const auto &sz : sizes)
        for (int rep = 0; rep < 4; ++rep, ++combo) {
            PackMember p;
            p.m = sz[0], p.n = sz[1];
            p.c = combo & 1, p.bounds = (combo >> 1) & 1, p.x0 = (combo >> 2) & 1, p.y0 = (combo >> 3) & 1, p.result = (combo % 3) != 0;
            mem.push_back(p);
        }
    const int K = static_cast<int>(mem.size());
    const GroupPackLayout L = group_pack_layout(mem.data(), K);
    if (static_cast<int>(L.slot.size()) != K) return 1;
    struct Range {
        size_t at, len;
    };
    std::vector<Range> data, start, result;
    size_t want_data = 0, want_start = 0, want_result = 0;
    auto padded = [](size_t len) { return (len + kPackAlign - 1) / kPackAlign * kPackAlign; };
    for (int k = 0; k < K; ++k) {
        const PackMember &p = mem[k];
        const PackSlot &s = L.slot[k];
        const size_t m = static_cast<size_t>(p.m), n = static_cast<size_t>(p.n);
        const struct { size_t at, len; bool given; std::vector<Range> *block; size_t *want; } v[10] = {
            {s.AL, m, p.bounds, &data, &want_data}, {s.AU, m, p.bounds, &data, &want_data}, {s.l, n, p.bounds, &data, &want_data},
            {s.u, n, p.bounds, &data, &want_data}, {s.c, n, p.c, &data, &want_data}, {s.x0, n, p.x0, &start, &want_start},
            {s.y0, m, p.y0, &start, &want_start}, {s.x, n, p.result, &result, &want_result}, {s.y, m, p.result, &result, &want_result},
            {s.z, n, p.result, &result, &want_result}};
        for (const auto &e : v) {
            const bool there = e.given && e.len > 0;
            if (there != (e.at != kPackAbsent)) return 1;
            if (!there) continue;
            if (e.at % kPackAlign != 0) return 4;
            e.block->push_back({e.at, e.len});
            *e.want += padded(e.len);
        }
    }
    if (want_data != L.data_doubles || want_start != L.start_doubles || want_result != L.result_doubles) return 1;  // (no room for the absent)
    const std::pair<std::vector<Range> *, size_t> blocks[3] = {{&data, L.data_doubles}, {&start, L.start_doubles}, {&result, L.result_doubles}};
    for (const auto &b : blocks) {
        std::vector<Range> r = *b.first;
        for (const Range &e : r)
            if (e.at + e.len > b.second) return 2;
        std::sort(r.begin(), r.end(), [](const Range &a, const Range &c) { return a.at < c.at; });
        for (size_t i = 1; i < r.size(); ++i)
            if (r[i - 1].at + r[i - 1].len > r[i].at) return 3;
    }
    // round trips on host memory: a value that names its member, vector and index
    auto value = [](int k, int vec, size_t i) { return 1000.0 * k + 100.0 * vec + static_cast<double>(i) + 0.25; };
    const double pad = -7.5;
    std::vector<double> dblock(L.data_doubles + 1, pad), sblock(L.start_doubles + 1, pad), rblock(L.result_doubles + 1, pad);
    std::vector<std::vector<double>> src(static_cast<size_t>(K) * 7);
    for (int k = 0; k < K; ++k) {
        const PackMember &p = mem[k];
        const size_t len[7] = {size_t(p.m), size_t(p.m), size_t(p.n), size_t(p.n), size_t(p.n), size_t(p.n), size_t(p.m)};
        for (int v = 0; v < 7; ++v) {
            std::vector<double> &a = src[static_cast<size_t>(k) * 7 + v];
            a.resize(len[v]);
            for (size_t i = 0; i < len[v]; ++i) a[i] = value(k, v, i);
        }
        const std::vector<double> *a = &src[static_cast<size_t>(k) * 7];
        group_pack_data(L, k, p, p.bounds ? a[0].data() : nullptr, p.bounds ? a[1].data() : nullptr, p.bounds ? a[2].data() : nullptr,
                        p.bounds ? a[3].data() : nullptr, p.c ? a[4].data() : nullptr, dblock.data());
        group_pack_start(L, k, p, p.x0 ? a[5].data() : nullptr, p.y0 ? a[6].data() : nullptr, sblock.data());
    }
    size_t written_d = 0, written_s = 0;
    for (int k = 0; k < K; ++k) {
        const PackSlot &s = L.slot[k];
        const size_t at[7] = {s.AL, s.AU, s.l, s.u, s.c, s.x0, s.y0};
        for (int v = 0; v < 7; ++v) {
            if (at[v] == kPackAbsent) continue;
            const std::vector<double> &a = src[static_cast<size_t>(k) * 7 + v];
            const double *blk = v < 5 ? dblock.data() : sblock.data();
            if (std::memcmp(blk + at[v], a.data(), sizeof(double) * a.size()) != 0) return 5;
            (v < 5 ? written_d : written_s) += a.size();
        }
    }
    // (everything that is not a vector's range still holds the padding value, the guard element behind the block included)
    if (static_cast<size_t>(std::count(dblock.begin(), dblock.end(), pad)) != dblock.size() - written_d) return 5;
    if (static_cast<size_t>(std::count(sblock.begin(), sblock.end(), pad)) != sblock.size() - written_s) return 5;
    // results: the device's side of the block is played by the host here
    for (int k = 0; k < K; ++k) {
        const PackMember &p = mem[k];
        const PackSlot &s = L.slot[k];
        if (!p.result) continue;
        for (int i = 0; i < p.n; ++i) {
            rblock[s.x + i] = value(k, 7, i);
            rblock[s.z + i] = value(k, 9, i);
        }
        for (int i = 0; i < p.m; ++i) rblock[s.y + i] = value(k, 8, i);
    }
    for (int k = 0; k < K; ++k) {
        const PackMember &p = mem[k];
        std::vector<double> x(static_cast<size_t>(p.n) + 1, pad), y(static_cast<size_t>(p.m) + 1, pad), z(static_cast<size_t>(p.n) + 1, pad);
        group_unpack_result(L, k, p, rblock.data(), x.data(), y.data(), z.data());
        for (int i = 0; i < p.n; ++i)
            if (x[i] != (p.result ? value(k, 7, i) : pad) || z[i] != (p.result ? value(k, 9, i) : pad)) return 6;
        for (int i = 0; i < p.m; ++i)
            if (y[i] != (p.result ? value(k, 8, i) : pad)) return 6;
        if (x[p.n] != pad || y[p.m] != pad || z[p.n] != pad) return 6;
    }
    if (rblock[L.result_doubles] != pad) return 6;
    // an empty group; a member that gave nothing
    const GroupPackLayout E = group_pack_layout(nullptr, 0);
    if (!E.slot.empty() || E.data_doubles || E.start_doubles || E.result_doubles) return 7;
    PackMember none;
    none.m = 5, none.n = 9;
    const GroupPackLayout N = group_pack_layout(&none, 1);
    if (N.data_doubles || N.start_doubles || N.result_doubles || N.slot[0].c != kPackAbsent || N.slot[0].x != kPackAbsent) return 7;
    if (N.slot[0].val != kPackAbsent) return 7;
    for (const PackSlot &s : L.slot)
        if (s.val != kPackAbsent) return 8;  // (nobody above gave values)
    // matrix values: nnz 1, odd, even, at and around the alignment; with all vectors, with none (a member on its own way)
    {
        const long counts[] = {1, 7, 31, 32, 33, 64, 2501, 2500, 0};
        std::vector<PackMember> vm;
        for (size_t i = 0; i < sizeof(counts) / sizeof(counts[0]); ++i) {
            PackMember p;
            p.m = 3 + static_cast<int>(i) * 5, p.n = 4 + static_cast<int>(i) * 7, p.nnz = counts[i];
            p.c = p.bounds = (i % 3) != 2;
            vm.push_back(p);
        }
        const int VK = static_cast<int>(vm.size());
        const GroupPackLayout V = group_pack_layout(vm.data(), VK);
        if (V.start_doubles || V.result_doubles) return 8;
        std::vector<double> vblock(V.data_doubles + 1, pad);
        std::vector<Range> vr;
        size_t want = 0, written = 0;
        for (int k = 0; k < VK; ++k) {
            const PackMember &p = vm[k];
            const PackSlot &s = V.slot[k];
            const size_t m = static_cast<size_t>(p.m), n = static_cast<size_t>(p.n), nz = static_cast<size_t>(p.nnz);
            if ((nz > 0) != (s.val != kPackAbsent)) return 8;
            if (p.bounds != (s.AL != kPackAbsent) || p.c != (s.c != kPackAbsent)) return 8;
            const size_t at[6] = {s.val, s.AL, s.AU, s.l, s.u, s.c};
            const size_t len[6] = {nz, m, m, n, n, n};
            size_t prev = kPackAbsent;
            std::vector<std::vector<double>> srcv(6);
            for (int v = 0; v < 6; ++v) {
                if (at[v] == kPackAbsent) continue;
                if (at[v] % kPackAlign != 0) return 8;
                if (at[v] != want) return 8;  // (the order of the staging, nothing in between but the padding)
                if (prev != kPackAbsent && at[v] <= prev) return 8;
                prev = at[v];
                want += padded(len[v]);
                vr.push_back({at[v], len[v]});
                srcv[v].resize(len[v]);
                for (size_t i = 0; i < len[v]; ++i) srcv[v][i] = value(k, v, i);
                written += len[v];
            }
            group_pack_values(V, k, p, nz > 0 ? srcv[0].data() : nullptr, vblock.data());
            group_pack_data(V, k, p, p.bounds ? srcv[1].data() : nullptr, p.bounds ? srcv[2].data() : nullptr, p.bounds ? srcv[3].data() : nullptr,
                            p.bounds ? srcv[4].data() : nullptr, p.c ? srcv[5].data() : nullptr, vblock.data());
            for (int v = 0; v < 6; ++v)
                if (at[v] != kPackAbsent && std::memcmp(vblock.data() + at[v], srcv[v].data(), sizeof(double) * len[v]) != 0) return 8;
        }
        if (want != V.data_doubles) return 8;
        for (const Range &e : vr)
            if (e.at + e.len > V.data_doubles) return 8;
        for (size_t i = 1; i < vr.size(); ++i)
            if (vr[i - 1].at + vr[i - 1].len > vr[i].at) return 8;
        if (static_cast<size_t>(std::count(vblock.begin(), vblock.end(), pad)) != vblock.size() - written) return 8;
    }
    {
        const int shapes[][3] = {{1, 2, 1}, {2, 1, 2}, {30, 50, 0}, {33, 31, 1}, {400, 600, 2}, {64, 32, 1}, {5, 9, 0}, {1, 1, 2}};
        std::vector<PackMember> cmv;
        for (const auto &sh : shapes) {
            PackMember p;
            p.m = sh[0], p.n = sh[1], p.cert = sh[2];
            cmv.push_back(p);
        }
        const GroupPackLayout Cl = group_pack_layout(cmv.data(), static_cast<int>(cmv.size()));
        if (Cl.data_doubles || Cl.start_doubles || Cl.result_doubles) return 9;
        size_t want = 0;
        for (size_t k = 0; k < cmv.size(); ++k) {
            const PackMember &p = cmv[k];
            const PackSlot &s = Cl.slot[k];
            const size_t m = static_cast<size_t>(p.m), n = static_cast<size_t>(p.n);
            const size_t at[4] = {s.cert_rn, s.cert_cn, s.cert_ray, s.cert_aty};
            const size_t len[4] = {m, n, p.cert == 1 ? m : n, n};
            const bool there[4] = {p.cert == 1, p.cert != 0, p.cert != 0, p.cert == 1};
            for (int v = 0; v < 4; ++v) {
                if (there[v] != (at[v] != kPackAbsent)) return 9;
                if (!there[v]) continue;
                if (at[v] != want || at[v] % kPackAlign != 0) return 9;  // (in order, nothing in between but the padding: disjoint)
                want += padded(len[v]);
                if (at[v] + len[v] > Cl.cert_doubles) return 9;
            }
            if (s.x != kPackAbsent || s.AL != kPackAbsent || s.val != kPackAbsent || s.x0 != kPackAbsent) return 9;
        }
        if (want != Cl.cert_doubles) return 9;
        for (const PackSlot &s : L.slot)
            if (s.cert_rn != kPackAbsent || s.cert_cn != kPackAbsent || s.cert_ray != kPackAbsent || s.cert_aty != kPackAbsent) return 9;
        if (L.cert_doubles) return 9;
    }
    return 0;
}
