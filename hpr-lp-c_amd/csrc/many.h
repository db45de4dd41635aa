// many.h -- a group of independent single-GPU solvers advanced in lock-step (many.cpp; DESIGN.md "Many small LPs").  Private.
#pragma once

#include "solver.h"

namespace hprlp {

// what a run_many call did: evaluation rounds; host waits (one per round + two per round with a restart); launches of the normal
// iterations; group launches of every kind (those, the group forms of the regular kernels, the packing of the scalars); copies of
// the scalars to the host; operations issued for ONE member (an own evaluation -- iteration 0, a member outside the group launches
// --, ray test, check step or restart piece); member-evaluations served by group launches
struct GroupCounts {
    long rounds = 0, waits = 0, launches = 0, group_launches = 0, copies = 0, own = 0, served = 0;
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
// Solver::scale() for every member, in lock-step: one launch per kernel kind and step for the members that join (Solver::joins_group,
// fused Ruiz norms) -- kernels.h: ScaleLaunches --, three host waits for the whole group; every other member runs its own scale()
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
// Solver::solve_loop + collect_solution for every member, from its current state
void run_many(Solver **s, int count, HPRLP_results *out, GroupCounts *counts = nullptr);

}  // namespace hprlp
