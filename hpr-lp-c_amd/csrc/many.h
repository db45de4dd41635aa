// many.h -- a group of independent single-GPU solvers advanced in lock-step (many.cpp; DESIGN.md "Many small LPs").  Private.
#pragma once

#include "solver.h"

namespace hprlp {

// what a run_many call did: evaluation rounds; host waits (one per round + two per round with a restart); launches of the normal
// iterations; group launches of every kind (those, the group forms of the regular kernels, the packing of the scalars); copies of
// the scalars to the host; operations issued for ONE member (an own evaluation -- iteration 0, a member outside the group launches
// --, check step, restart piece, the ray test or the certificate of a member outside the group launches); member-evaluations
// served by group launches; member ray tests served by group launches; certificates collected through the group's block (each
// round with such a verdict adds one wait and one copy to the counts above)
struct GroupCounts {
    long rounds = 0, waits = 0, launches = 0, group_launches = 0, copies = 0, own = 0, served = 0, ray_served = 0, certs_served = 0;
};

// what a group set-up, scaling or teardown did (hprlp_last_setup_many_counts; each call fills its own slots): calls to the driver
// for device memory, pinned memory and host-to-device copies of the set-up; kernel launches and host waits of the scaling (the
// launches of members that scaled on their own included); members served by the group's scaling launches / that ran their own
// Solver::scale(); device frees of the teardown
struct SetupCounts {
    long device_allocs = 0, pinned_allocs = 0, h2d_copies = 0, scale_launches = 0, scale_waits = 0, served = 0, own = 0, device_frees = 0;
};

// Wide members (DESIGN.md "Many small LPs", wide members): solvers off the small path with Solver::group_wide set.  What the
// calling thread's last group call with such a member did (hprlp_last_many_wide_counts): wide members that join the group launches
// / that cannot (a tiled copy, split rows); launches of the normal iterations issued through the group's recorder, two per
// iteration of a segment whatever the number of its members; segments (group_table.h: group_iteration_plan); member-iterations
// served by them; launches of the group power iteration (the packing of the scalars included) and its host waits.
// check_group zeroes the block and fills the first two slots whenever it sees a wide member.
struct WideCounts {
    long joined = 0, refused = 0, normal_launches = 0, segments = 0, member_iterations = 0, power_launches = 0, power_waits = 0;
};
WideCounts &last_wide_counts();  // (hprlp_solve_many_wide adds its power iteration to its loop)

// Throws (before anything is launched) unless s[0..count) are distinct, non-null, scaled, unsharded solvers on one device.
// need_scaled = false: a solver never scaled is welcome (scale_many).
void check_group(Solver *const *s, int count, const char *who, bool need_scaled = true);
// Solver::scale() for every member, in lock-step: the pieces of scale() recorded into one GroupLaunches for the members that join
// (Solver::joins_group, fused Ruiz norms) -- one launch per kernel kind and stage, three host waits for the whole group; every other
// member runs its own scale()
// inside the same call, and so does a group with fewer than two joining members.  Every member ends bit for bit where its own
// scale() leaves it.
void scale_many(Solver **s, int count, SetupCounts *counts = nullptr);
// lambda (not x 1.01) and iteration count per member; small-path members in one launch per class.  Wide members that join (two at
// least): the regular path of Solver::power_iteration in group launches -- ten iterations and the error terms recorded once and
// issued as one run, one copy of the scalars and one wait per block for all of them, each member's own stopping test on the host
// (a member that stopped is in no later block), the tail of a max_iter that is no multiple of ten as single iterations without
// error terms, the two scratch vectors zeroed: lambda, iteration count and power_iters are the member's own.  Everybody else on
// their own.
void power_iteration_many(Solver **s, int count, int max_iter, double tol, double *lambda_out, int *iters_out);
// normal[k] normal iterations of member k (small-path members together; wide members that join in segments of group launches, two
// launches per iteration of a segment), then one check step each if then_check (the group's check launches for the members that
// join them); waits at the end
void iterate_many(Solver **s, int count, const int *normal, bool then_check);
// Solver::compute_residuals for every member: out[8 * k ..] as hprlp_solver_residuals.  Group launches for the members that join
// them and have iter[k] > 0; one copy of the scalars, one wait.
void residuals_many(Solver **s, int count, const int *iter, const int *compute_gap, double *out);
// Solver::update_sigma_and_restart for every member from in[6 * k ..] as hprlp_solver_restart; sigma_out (optional): the new sigmas
void restart_many(Solver **s, int count, const double *in, double *sigma_out);
// hprlp_solver_ray_step for every member: the evaluation with the gap, then the ray test, one copy of the scalars and one wait,
// through the group launches for the members that join.  tested[k]: 1 or 0 as that entry's return value; out + 9 k is untouched
// where it is 0.  The members have passed check_group and the arrays are not null (abi.cpp owns those refusals); throws before
// anything is launched for a first step without restart[k].
void ray_step_many(Solver **s, int count, const int *restart, double *out, int *tested);
// Solver::solve_loop + collect_solution for every member, from its current state.  With detection on, the ray tests and the
// certificates of the members that join are the group's (DESIGN.md "Many small LPs", group detection).
void run_many(Solver **s, int count, HPRLP_results *out, GroupCounts *counts = nullptr);

// ---- group re-solve, group matrix values and their device twins (DESIGN.md "Many small LPs": group re-solve, group matrix values,
// group device re-solve) -----------------------------------------------------------------------------------------------------------
// Three pairs of entries.  A host entry takes the members' vectors in host memory; its device twin takes them in DEVICE memory of
// the caller's (obj_constant and sigma stay host values) and a stream `caller` on which they were produced: one event on it, the
// group's stream waits for it before its first read, and the call returns after the group's stream has drained.  The two of a
// pair are one body in many.cpp; a pair is described once below, with what its twin does differently.  For all six: the members
// have passed check_group and data / out are not null (abi.cpp owns those refusals); every refusal comes before anything a solver
// reads is written, so it leaves every member as it was; the members that join (two at least) are served by the group launches,
// every other member runs its own single entry -- Solver::set_data / resolve / set_matrix_values, or their *_device forms --
// inside the same call.
struct MemberData {   // Solver::set_data's arguments for one member (hprlp_member_data); all null: nothing changes
    const double *c = nullptr, *obj_constant = nullptr, *AL = nullptr, *AU = nullptr, *l = nullptr, *u = nullptr;
};
struct MemberStart {  // Solver::resolve's arguments for one member (hprlp_member_start)
    const double *x0 = nullptr, *y0 = nullptr;
    double sigma = -1.0;
};
struct MemberValues {  // Solver::set_matrix_values' arguments for one member (hprlp_member_values); all null: the member is skipped
    const double *val = nullptr;
    long nnz = 0;
    const double *c = nullptr, *obj_constant = nullptr, *AL = nullptr, *AU = nullptr, *l = nullptr, *u = nullptr;
};
struct MemberOut {  // where one member's solution goes (hprlp_member_out): device buffers of the caller's, null: not wanted
    double *x = nullptr, *y = nullptr, *z = nullptr;
};
// What a group call did outside the loop, the operations of the members that went their own way included: copies host -> device
// (staging blocks and task tables) and device -> host, host waits, kernel launches and memsets; members served by the group
// launches / that went their own way (a member that gave nothing, or obj_constant only, is neither).  What the group issues is
// counted where it is issued; what a member on its own issues is NOMINAL: the operations its single entry issues in the common
// case (staging below the allocator cache's block size: one upload; no locality ordering; code arrays in place) -- set_matrix_values
// apart, where scaling launches and scalar fetches are counted where the solver counts them.
struct CallCounts {
    long h2d = 0, d2h = 0, waits = 0, launches = 0, memsets = 0, served = 0, own = 0;
};
// hprlp_last_resolve_many_counts (set_data_many, resolve_many and twins); resolve: the loop's operations issued for one member
// (GroupCounts::own)
struct ResolveCounts : CallCounts {
    long loop_own = 0;
};
// hprlp_last_values_many_counts (set_matrix_values_many and twin); members whose value maps were built in this call
struct ValuesCounts : CallCounts {
    long maps = 0;
};
// what a device group call did beyond ResolveCounts / ValuesCounts (hprlp_last_many_device_counts): non-null device pointers
// checked; lookups issued to the runtime for them (a pointer inside a range already reported in the call needs none); launches of
// the device check; flag words copied back; members served by the group launches / that ran their own device entry; host waits
// before the first write of anything a solver reads (the check's: 0 where nothing had to be checked).  Filled as the call
// proceeds, so it also tells what a refused call did.
struct DeviceCounts {
    long pointers = 0, lookups = 0, check_launches = 0, flags = 0, served = 0, own = 0, waits_before_write = 0;
};

// Solver::set_data for every member.  Refused first: an incomplete bounds group, a NaN in obj_constant or, host entry, in a vector.
// The members that join (something given, Solver::joins_group_resolve): all given vectors in one pinned block and one copy,
// k_reduce_many<DataInTask>, finalize, k_reduce_many<DataBcTask>, finalize, the scalars packed, one copy back, ONE wait, then each
// member's host formulas.  The device twin: every non-null pointer of every member passes check_device_pointer (one lookup per
// distinct range), then ONE launch checks the vectors of all members where they lie for NaN, one copy of the flag words, one wait;
// the joiners' passes read the caller's buffers -- same kernels, same bits.
void set_data_many(Solver **s, int count, const MemberData *data, ResolveCounts *counts = nullptr);
void set_data_many_device(Solver **s, int count, const MemberData *data, hipStream_t caller, ResolveCounts *counts = nullptr,
                          DeviceCounts *dcounts = nullptr);
// check_starts: throws, naming `who: member k`, for a NaN sigma and, host_vectors, for a non-finite start entry; touches nothing.
void check_starts(Solver *const *s, int count, const MemberStart *start, const char *who, bool host_vectors);
// Solver::resolve for every member: zeroing, bound codes, ctrl (a sigma override included) and the starts of the joining members
// (Solver::joins_group_resolve) recorded into the group's launches, the lock-step loop of run_many with their iteration-0
// evaluations recorded as well, the solutions through one device block, one copy and one wait.  start null: all cold.  The starts
// have passed check_starts.  The device twin: the pointers of starts and outputs looked up, the starts of all members checked
// where they lie by one launch (non-finite entries); a member on its own runs from start to solution before the loop, which then
// holds the joiners alone; the solutions are stored into dst[k] (null: none wanted) and out[k].x / y / z stay null.
void resolve_many(Solver **s, int count, const MemberStart *start, HPRLP_results *out, ResolveCounts *counts = nullptr);
void resolve_many_device(Solver **s, int count, const MemberStart *start, const MemberOut *dst, hipStream_t caller, HPRLP_results *out,
                         ResolveCounts *counts = nullptr, DeviceCounts *dcounts = nullptr);
// Solver::set_matrix_values for every member that gave values.  All host rules of all members first (all six vectors, nnz, NaN
// in obj_constant or, host entry, in a vector); the values of ALL of them in one pinned block and one copy, checked by ONE launch
// into one flag word per member, one copy of the flags, one wait.  Then the members that join (values given,
// Solver::joins_group_resolve, scale_many's conditions): scatter, gather and the zeroing of reset_iterates recorded in one stage,
// and Solver::scale()'s pieces walked behind them (scale_many's walk).  The device twin: the pointers looked up; vectors and
// values checked where they lie in the same stage (a second flag word per member; a vector's NaN wins); a joiner's `val` must be
// aligned to 16 bytes (the scatter loads pairs; the staging block is aligned by construction).
void set_matrix_values_many(Solver **s, int count, const MemberValues *data, ValuesCounts *counts = nullptr);
void set_matrix_values_many_device(Solver **s, int count, const MemberValues *data, hipStream_t caller, ValuesCounts *counts = nullptr,
                                   DeviceCounts *dcounts = nullptr);

}  // namespace hprlp

