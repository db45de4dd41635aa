// batch_prep.h -- the host side of solve_batched that needs no device: the panel geometry (shared with the kernels of
// batched.hip), the per-member scaling of a batch's vectors, the maps between the caller's units and scaled units (per element:
// batch_units.h, which the kernels call too), and the allocation of the results.  Plain host code: no HIP header, no HIP call; hprlp_batched_prepare_host (abi.cpp) runs it on
// plain arrays, so that its arithmetic can be held to a restatement bit for bit without a GPU (tests/test_batch_prep.py).
#pragma once

#include <array>
#include <cstddef>
#include <vector>

#include "batch_units.h"
#include "structs.h"

namespace hprlp {

// a batched result whose every member has status `status` and no arrays
HPRLP_batched_results make_batched_error(const char *status, int m, int n, int B);  // reference batched_solver.cu:356-368
// ... and one with all eight arrays for B members (status zeroed); throws when the host allocation fails
HPRLP_batched_results alloc_batched_results(int m, int n, int B);


// ---- panel geometry ------------------------------------------------------------------------------------------------------
// thread -> (row slot, problem): lane l of a wave handles sub-row l / Bw and problem chunk*Bw + l % Bw, Bw = Bc = the
// chunk width; a 256-thread block covers 4 * (64/Bw) rows of one chunk.
struct Geo {
    int Bp, Bw, nchunk, rows_per_wave, rows_per_block;
};
inline Geo make_geo(int Bp, int Bc) {
    Geo g;
    g.Bp = Bp;
    g.Bw = Bc;
    g.nchunk = Bp / Bc;
    g.rows_per_wave = 64 / g.Bw;
    g.rows_per_block = 4 * g.rows_per_wave;
    return g;
}
int padded_batch(int B);  // a power of two up to 64, a multiple of 64 above
// Chunk width.  Below 64 problems: one chunk.  From 64 up: 64 (a wave = one row, scalar CSR loads); HPRLP_BATCH_CHUNK = 8 / 16 /
// 32 / 64 overrides (read per call).
int choose_chunk(int m, int n, int Bp);
// element (row i, problem k) of a device panel with `rows` rows (the host's copy of pidx)
inline size_t panel_index(const Geo &g, int rows, int i, int k) {
    return (static_cast<size_t>(k / g.Bw) * rows + i) * g.Bw + k % g.Bw;
}
// column-major (ABI) rows x B -> padded device panel
void to_panel(const std::vector<double> &cm, int rows, int B, const Geo &g, double pad, std::vector<double> &out);
// ... and back: the first B members of a panel -> column-major rows x B
void from_panel(const std::vector<double> &panel, int rows, int B, const Geo &g, double *cm);

// ---- a batch's vectors in scaled units (reference batched_solver.cu:792-885) -----------------------------------------------
struct BatchData {
    int m = 0, n = 0, B = 0;
    std::vector<double> C, AL, AU, L, U;  // column-major, n x B / m x B; infinite row sides and bounds are +-kInfReplacement
    std::vector<double> b_scale, c_scale, norm_b, norm_c, norm_b_org, norm_c_org, objc;  // per member
    std::vector<double> sigma;            // the first sigma (batch_units.h: first_sigma)
};
// The per-member scalar vectors of a BatchData, enumerated once: the seven that a device-entry call computes where the batch lies,
// in the order in which it stores them (batched.hip: DataScalar), then objc.
constexpr int kMemberScalars = 8;
template <class Data>  // BatchData or const BatchData
inline auto member_scalars(Data &d) -> std::array<decltype(&d.sigma), kMemberScalars> {
    return {{&d.b_scale, &d.c_scale, &d.norm_b, &d.norm_c, &d.norm_b_org, &d.norm_c_org, &d.sigma, &d.objc}};
}
// ... and the scalars of the first W members of q alone: no vectors (a streamed batch's slots at its start)
inline BatchData first_members(const BatchData &q, int W) {
    BatchData d;
    d.m = q.m; d.n = q.n; d.B = W;
    const auto to = member_scalars(d);
    const auto from = member_scalars(q);
    for (int s = 0; s < kMemberScalars; ++s) to[s]->assign(from[s]->begin(), from[s]->begin() + W);
    return d;
}

// The order in which a norm's sum of squares is added up is part of its bits.  Rule 0 is the reference's: long double,
// sequentially.  Rule 1, the "tree" rule, is one a GPU can follow, fixed by the vector's length alone (DESIGN.md "Device-resident
// batches"; kb_data_in / kb_data_bc of batched.hip are its device side, tree_sum_of_squares below its host twin).  The terms
// t_i = v_i * v_i are rounded to double and never fused with the add.  Rows are cut into segments of kNormSeg consecutive rows;
// within a segment, lane j of kNormLanes adds the terms with (i - s * kNormSeg) % kNormLanes == j in increasing i, from 0.0; the
// lane sums are folded by halving strides (a[j] += a[j + stride], stride kNormLanes / 2 ... 1); the segment sums are added in
// increasing s, from 0.0.
constexpr int kNormRuleReference = 0, kNormRuleTree = 1;
constexpr int kNormSeg = 16384, kNormLanes = 256;
static_assert(kNormSeg % kNormLanes == 0 && (kNormLanes & (kNormLanes - 1)) == 0, "whole rounds of a power of two of lanes");
constexpr int norm_segments(int rows) { return (rows + kNormSeg - 1) / kNormSeg; }
// rn (m) / cn (n): the shared matrix' row / column scaling.  obj_constants null: model_obj_constant for every member.
// norm_rule: kNormRuleReference (the default: the bits of every call before the rule existed) or kNormRuleTree.
BatchData prepare_batch(int m, int n, int B, const double *C, const double *AL, const double *AU, const double *l, const double *u,
                        const double *obj_constants, double model_obj_constant, const double *rn, const double *cn,
                        bool use_bc_scaling, int norm_rule = kNormRuleReference);

// ---- caller's units <-> scaled units, column-major rows x B in place: batch_units.h's maps of the same names, element by element --
// a start: X0 with cn and b_scale, Y0 with rn and c_scale
void start_to_scaled(double *v, int rows, int B, const double *norm, const std::vector<double> &scale);
// a solution: x with cn and b_scale, y with rn and c_scale ...
void point_to_caller(double *v, int rows, int B, const double *norm, const std::vector<double> &scale);
// ... and z
void reduced_cost_to_caller(double *z, int n, int B, const double *cn, const std::vector<double> &c_scale);

}  // namespace hprlp
