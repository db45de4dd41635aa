// group_pack.h -- where the vectors of a group call lie in its staging and result blocks (many.cpp: set_data_many, resolve_many,
// set_matrix_values_many; DESIGN.md "Many small LPs", group re-solve and group matrix values).  Host only: no HIP header, no device call (hprlp_group_pack_selftest runs without a
// GPU, and tools/group_pack_check.cpp runs the same code under the host sanitizers).
#pragma once

#include <cstddef>
#include <vector>

namespace hprlp {

constexpr size_t kPackAbsent = static_cast<size_t>(-1);  // offset of a vector that was not given: it takes no room
constexpr size_t kPackAlign = 32;                         // doubles: every vector starts on a 256-byte boundary of its block

// One member of a group call: its sizes and which vectors it gave (set_data_many: c, bounds; resolve_many: x0, y0, result;
// set_matrix_values_many: nnz values, c, bounds).
struct PackMember {
    int m = 0, n = 0;
    long nnz = 0;                    // matrix values given (0: none): they lie in front of the member's vectors in the data block
    bool c = false, bounds = false;  // bounds: AL, AU (m) and l, u (n) together
    bool x0 = false, y0 = false;
    bool result = false;             // the member's solution [x (n) | y (m) | z (n)] comes back through the group's block
    // a verdict's raw arrays come back through the group's certificate block (loop_many): 1 primal infeasible [row_norm (m) |
    // col_norm (n) | ray_y (m) | A^T y_s (n)], 2 dual infeasible [col_norm (n) | ray_d (n)], 0 none
    int cert = 0;
};

// Offsets in doubles (kPackAbsent: not there).  Four blocks: the data of set_data_many, the starts of resolve_many (both travel
// host -> device in one copy each), the results and the certificates of a round's verdicts (device -> host in one copy each).
struct PackSlot {
    size_t val = kPackAbsent;
    size_t AL = kPackAbsent, AU = kPackAbsent, l = kPackAbsent, u = kPackAbsent, c = kPackAbsent;
    size_t x0 = kPackAbsent, y0 = kPackAbsent;
    size_t x = kPackAbsent, y = kPackAbsent, z = kPackAbsent;
    size_t cert_rn = kPackAbsent, cert_cn = kPackAbsent, cert_ray = kPackAbsent, cert_aty = kPackAbsent;
};
struct GroupPackLayout {
    std::vector<PackSlot> slot;
    size_t data_doubles = 0, start_doubles = 0, result_doubles = 0, cert_doubles = 0;
};

GroupPackLayout group_pack_layout(const PackMember *members, int count);

// The caller's vectors of member k into the data / start block (null sources are absent vectors: the layout must say so too)
void group_pack_data(const GroupPackLayout &L, int k, const PackMember &mb, const double *AL, const double *AU, const double *l, const double *u,
                     const double *c, double *block);
void group_pack_values(const GroupPackLayout &L, int k, const PackMember &mb, const double *val, double *block);
void group_pack_start(const GroupPackLayout &L, int k, const PackMember &mb, const double *x0, const double *y0, double *block);
// member k's solution out of the result block
void group_unpack_result(const GroupPackLayout &L, int k, const PackMember &mb, const double *block, double *x, double *y, double *z);

}  // namespace hprlp

extern "C" int hprlp_group_pack_selftest(void);  // 0, or the number of the check that failed
