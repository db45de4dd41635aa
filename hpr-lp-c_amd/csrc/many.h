// many.h -- a group of independent single-GPU solvers advanced in lock-step (many.cpp; DESIGN.md "Many small LPs").  Private.
#pragma once

#include "solver.h"

namespace hprlp {

// what a run_many call did: evaluation rounds, host waits (one per round + two per restart of a member), group launches
struct GroupCounts {
    long rounds = 0, waits = 0, launches = 0;
};

// Throws (before anything is launched) unless s[0..count) are distinct, non-null, scaled, unsharded solvers on one device.
void check_group(Solver *const *s, int count, const char *who);
// lambda (not x 1.01) and iteration count per member; small-path members in one launch per class, the others on their own
void power_iteration_many(Solver **s, int count, int max_iter, double tol, double *lambda_out, int *iters_out);
// normal[k] normal iterations of member k (small-path members together), then one check step each if then_check; waits at the end
void iterate_many(Solver **s, int count, const int *normal, bool then_check);
// Solver::solve_loop + collect_solution for every member, from its current state
void run_many(Solver **s, int count, HPRLP_results *out, GroupCounts *counts = nullptr);

}  // namespace hprlp
