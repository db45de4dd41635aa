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

// Throws (before anything is launched) unless s[0..count) are distinct, non-null, scaled, unsharded solvers on one device.
void check_group(Solver *const *s, int count, const char *who);
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
