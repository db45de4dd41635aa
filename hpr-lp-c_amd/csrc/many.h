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

// Throws (before anything is launched) unless s[0..count) are distinct, non-null, scaled, unsharded solvers on one device.
// need_scaled = false: a solver never scaled is welcome (scale_many).
void check_group(Solver *const *s, int count, const char *who, bool need_scaled = true);
// Solver::scale() for every member, in lock-step: the pieces of scale() recorded into one GroupLaunches for the members that join
// (Solver::joins_group, fused Ruiz norms) -- one launch per kernel kind and stage, three host waits for the whole group; every other
// member runs its own scale()
// inside the same call, and so does a group with fewer than two joining members.  Every member ends bit for bit where its own
// scale() leaves it.
void scale_many(Solver **s, int count, SetupCounts *counts = nullptr);
// lambda (not x 1.01) and iteration count per member; small-path members in one launch per class, the others on their own
void power_iteration_many(Solver **s, int count, int max_iter, double tol, double *lambda_out, int *iters_out);
// normal[k] normal iterations of member k (small-path members together), then one check step each if then_check (the group's check
// launches for the members that join them); waits at the end
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

// ---- group re-solve (DESIGN.md "Many small LPs", group re-solve) ------------------------------------------------------------
struct MemberData {   // Solver::set_data's arguments for one member (hprlp_member_data); all null: nothing changes
    const double *c = nullptr, *obj_constant = nullptr, *AL = nullptr, *AU = nullptr, *l = nullptr, *u = nullptr;
};
struct MemberStart {  // Solver::resolve's arguments for one member (hprlp_member_start)
    const double *x0 = nullptr, *y0 = nullptr;
    double sigma = -1.0;
};
// what a set_data_many / resolve_many call did (hprlp_last_resolve_many_counts): copies host -> device (staging blocks and task
// tables) and device -> host, host waits, kernel launches and memsets, all OUTSIDE the loop and with the operations of the members
// that went their own way included; members served by the group launches / that went their own way (a member that gave nothing,
// or obj_constant only, is neither); resolve_many: the loop's operations issued for one member (GroupCounts::own).  What the
// group issues is counted where it is issued; what a member on its own issues is NOMINAL: the operations its single entries issue
// in the common case (staging below the allocator cache's block size: one upload; no locality ordering; code arrays in place)
struct ResolveCounts {
    long h2d = 0, d2h = 0, waits = 0, launches = 0, memsets = 0, served = 0, own = 0, loop_own = 0;
};
// Solver::set_data for every member.  The members that join (Solver::joins_group_resolve, two at least): all given vectors in one
// pinned block and one copy, k_reduce_many<DataInTask>, finalize, k_reduce_many<DataBcTask>, finalize, the scalars packed, one copy back, ONE wait, then
// each member's host formulas.  Every other member runs its own set_data inside the same call.  The members have passed
// check_group and data is not null (abi.cpp owns those refusals); throws before anything is written or launched: an incomplete
// bounds group, a NaN.
void set_data_many(Solver **s, int count, const MemberData *data, ResolveCounts *counts = nullptr);
// Solver::resolve for every member: zeroing, bound codes, ctrl (a sigma override included) and the starts of the joining members
// recorded into the group's launches, the lock-step loop of run_many with their iteration-0 evaluations recorded as well, the
// solutions through one device block, one copy and one wait.  start null: all cold.  The members have passed check_group, out
// is not null (abi.cpp owns those refusals) and the starts have passed check_starts.
// check_starts: throws, naming `member k`, for a NaN sigma or a non-finite start entry; touches nothing.
void check_starts(Solver *const *s, int count, const MemberStart *start);
void resolve_many(Solver **s, int count, const MemberStart *start, HPRLP_results *out, ResolveCounts *counts = nullptr);

// ---- group matrix values (DESIGN.md "Many small LPs", group matrix values) ------------------------------------------------------
struct MemberValues {  // Solver::set_matrix_values' arguments for one member (hprlp_member_values); all null: the member is skipped
    const double *val = nullptr;
    long nnz = 0;
    const double *c = nullptr, *obj_constant = nullptr, *AL = nullptr, *AU = nullptr, *l = nullptr, *u = nullptr;
};
// what a set_matrix_values_many call did (hprlp_last_values_many_counts): copies host -> device (the staging block and the task
// tables) and device -> host, host waits, kernel launches, memsets; members served by the group launches / that went their own way
// (for those the operations their own Solver::set_matrix_values issues are added: counted where the solver counts them -- scaling
// launches, scalar fetches --, nominal otherwise, as ResolveCounts); members whose value maps were built in this call
struct ValuesCounts {
    long h2d = 0, d2h = 0, waits = 0, launches = 0, memsets = 0, served = 0, own = 0, maps = 0;
};
// Solver::set_matrix_values for every member that gave values.  All host checks of all members first; the values of ALL of them
// in one pinned block and one copy, checked by ONE launch into one flag word per member, one copy of the flags, one wait -- up to
// there nothing a solver reads has been written, so a refusal leaves every member as it was.  Then the members that join
// (values given, Solver::joins_group_resolve, scale_many's conditions, two at least): scatter, gather and the zeroing of
// reset_iterates recorded in one stage, and Solver::scale()'s pieces walked behind them (scale_many's walk); every other member
// runs its own set_matrix_values inside the same call.  The members have passed check_group and data is not null (abi.cpp owns
// those refusals).
void set_matrix_values_many(Solver **s, int count, const MemberValues *data, ValuesCounts *counts = nullptr);

// ---- group device re-solve (DESIGN.md "Many small LPs", group device re-solve) ---------------------------------------------------
struct MemberOut {  // where one member's solution goes (hprlp_member_out): device buffers of the caller's, null: not wanted
    double *x = nullptr, *y = nullptr, *z = nullptr;
};
// what a device group call did beyond ResolveCounts / ValuesCounts (hprlp_last_many_device_counts): non-null device pointers
// checked; lookups issued to the runtime for them (a pointer inside a range already reported in the call needs none); launches of
// the device check; flag words copied back; members served by the group launches / that ran their own device entry; host waits
// before the first write of anything a solver reads (the check's: 0 where nothing had to be checked)
struct DeviceCounts {
    long pointers = 0, lookups = 0, check_launches = 0, flags = 0, served = 0, own = 0, waits_before_write = 0;
};
// set_data_many, resolve_many and set_matrix_values_many with the members' vectors in DEVICE memory of the caller's (obj_constant
// and sigma stay host values) and the solutions stored into dst[k] (null: none wanted); out[k].x / y / z stay null.  `caller` is
// the stream the inputs were produced on: one event on it, the group's stream waits for it before its first read, and the call
// returns after the group's stream has drained.  Every non-null pointer of every member passes check_device_pointer first (one
// lookup per distinct range); then ONE launch checks the vectors of all members where they lie (NaN in a data vector, a
// non-finite start entry; the values in the same stage), one copy of the flag words, one wait -- a refusal of any kind leaves
// every member as it was.  The members that join read the caller's buffers where the host entries read the staging block, same
// kernels, same bits; every other member runs its own Solver::set_data_device / resolve_device / set_matrix_values_device inside
// the same call.  The members have passed check_group and data / out are not null (abi.cpp owns those refusals).  dcounts is
// filled as the call proceeds, so it also tells what a refused call did.
void set_data_many_device(Solver **s, int count, const MemberData *data, hipStream_t caller, ResolveCounts *counts = nullptr,
                          DeviceCounts *dcounts = nullptr);
void resolve_many_device(Solver **s, int count, const MemberStart *start, const MemberOut *dst, hipStream_t caller, HPRLP_results *out,
                         ResolveCounts *counts = nullptr, DeviceCounts *dcounts = nullptr);
void set_matrix_values_many_device(Solver **s, int count, const MemberValues *data, hipStream_t caller, ValuesCounts *counts = nullptr,
                                   DeviceCounts *dcounts = nullptr);

}  // namespace hprlp
