// many.cpp -- a group of independent solvers advanced in lock-step (DESIGN.md "Many small LPs").
//
// A Netlib-scale LP runs as one workgroup (small.hip) and keeps one CU of 256 busy.  K such LPs, each with its own matrix, are
// advanced together here: one k_small_iterations_many launch per <KMAX, R> class carries the normal iterations of every member
// (workgroup b = member b, the single-LP kernel's arithmetic on the member's own arguments), and one host wait serves the
// evaluations of all members.  Everything else -- check step, evaluation, stopping test, restart rule, sigma update, detection --
// is the member's own code (the pieces of Solver::solve_loop), so a member's iterates and results are the bits it gets alone.
//
// Ordering is by stream: for the duration of a call every member works on ONE stream (the first member's), after its own stream
// has been waited for once; the members' streams come back at exit, after one wait for the group's.
#include <algorithm>
#include <cmath>

#include "many.h"

namespace hprlp {

namespace {

// The members on one stream, quiet, for the lifetime of this object.
struct GroupScope {
    Solver **s;
    int count;
    hipStream_t group = nullptr;
    std::vector<hipStream_t> own;
    std::vector<char> verbose;
    GroupScope(Solver **s_, int count_) : s(s_), count(count_), own(static_cast<size_t>(count_)), verbose(static_cast<size_t>(count_)) {
        HIP_CHECK(hipSetDevice(s[0]->prm.device_number));
        for (int k = 0; k < count; ++k) HIP_CHECK(hipStreamSynchronize(s[k]->stream));
        group = s[0]->stream;
        for (int k = 0; k < count; ++k) {
            own[k] = s[k]->stream;
            verbose[k] = s[k]->verbose ? 1 : 0;
            s[k]->stream = group;
            s[k]->verbose = false;  // (interleaved banners and iteration tables are of no use)
        }
    }
    ~GroupScope() {
        (void)hipStreamSynchronize(group);  // nothing of a member is in flight on another stream than its own afterwards
        for (int k = 0; k < count; ++k) {
            s[k]->stream = own[k];
            s[k]->verbose = verbose[k] != 0;
        }
    }
};

bool on_small_path(const Solver *s) { return s->use_small && !s->comm; }

}  // namespace

void check_group(Solver *const *s, int count, const char *who) {
    const std::string w(who);
    if (!s) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    for (int k = 0; k < count; ++k) {
        if (!s[k]) throw std::runtime_error(w + ": member " + std::to_string(k) + " is null");
        if (s[k]->comm) throw std::runtime_error(w + ": member " + std::to_string(k) + " is a sharded solver; a group runs on one GPU");
        if (!s[k]->scaled) throw std::runtime_error(w + ": member " + std::to_string(k) + " was never scaled (hprlp_solver_scale)");
        if (s[k]->prm.device_number != s[0]->prm.device_number)
            throw std::runtime_error(w + ": member " + std::to_string(k) + " lives on another device than member 0");
        for (int j = 0; j < k; ++j)
            if (s[j] == s[k]) throw std::runtime_error(w + ": members " + std::to_string(j) + " and " + std::to_string(k) + " are the same solver");
    }
}

void power_iteration_many(Solver **s, int count, int max_iter, double tol, double *lambda_out, int *iters_out) {
    check_group(s, count, "power_iteration_many");
    const auto t0 = time_now();
    GroupScope scope(s, count);
    std::vector<SmallPowerTask> tasks;
    std::vector<int> who;
    for (int k = 0; k < count; ++k) {
        if (!s[k]->small_power_wanted()) continue;
        Solver &m = *s[k];
        m.finish_tiling();
        m.invalidate_far();
        m.power_start(m.sm1.p);
        HIP_CHECK(hipMemsetAsync(m.scal.p + S_SMALL_PW_LAMBDA, 0, 2 * sizeof(double), scope.group));
        tasks.push_back(SmallPowerTask{m.small_args(), m.sm1.p, m.scal.p + S_SMALL_PW_LAMBDA, tol, 0, max_iter});
        who.push_back(k);
    }
    SmallTaskBuf buf;
    std::vector<char> done(static_cast<size_t>(count), 0);
    if (!tasks.empty()) {
        launch_small_power_many(tasks.data(), static_cast<int>(tasks.size()), buf, scope.group);
        for (int k : who) s[k]->fetch_enqueue();
        HIP_CHECK(hipStreamSynchronize(scope.group));
        for (int k : who) {
            Solver &m = *s[k];
            ++m.fetches;
            const double lambda_dev = m.scal_h[S_SMALL_PW_LAMBDA];
            const int done_dev = static_cast<int>(m.scal_h[S_SMALL_PW_ITERS]);
            // (as Solver::power_iteration: anything but a positive finite lambda of a kernel that ran goes to the regular path below)
            if (!(done_dev > 0 && std::isfinite(lambda_dev) && lambda_dev > 0.0)) continue;
            m.power_iters = done_dev;
            m.power_time = time_since(t0);  // the group's wall time: what a member's reported time starts from
            if (lambda_out) lambda_out[k] = lambda_dev;
            if (iters_out) iters_out[k] = done_dev;
            done[k] = 1;
        }
    }
    for (int k = 0; k < count; ++k) {
        if (done[k]) continue;
        int it = 0;
        const double lam = s[k]->power_iteration(max_iter, tol, &it);
        if (lambda_out) lambda_out[k] = lam;
        if (iters_out) iters_out[k] = it;
    }
}

void iterate_many(Solver **s, int count, const int *normal, bool then_check) {
    check_group(s, count, "iterate_many");
    if (!normal) throw std::runtime_error("iterate_many: null iteration counts");
    for (int k = 0; k < count; ++k)
        if (normal[k] < 0) throw std::runtime_error("iterate_many: normal[" + std::to_string(k) + "] is negative");
    GroupScope scope(s, count);
    std::vector<SmallIterTask> tasks;
    for (int k = 0; k < count; ++k) {
        if (!on_small_path(s[k]) || normal[k] <= 0) continue;
        s[k]->finish_tiling();
        tasks.push_back(SmallIterTask{s[k]->small_args(), 0, normal[k]});
    }
    SmallTaskBuf buf;
    launch_small_iterations_many(tasks.data(), static_cast<int>(tasks.size()), buf, scope.group);
    for (int k = 0; k < count; ++k)
        if (!on_small_path(s[k])) s[k]->run_normal(normal[k]);
    if (then_check)
        for (int k = 0; k < count; ++k) s[k]->step(true);
    HIP_CHECK(hipStreamSynchronize(scope.group));
}

void run_many(Solver **s, int count, HPRLP_results *out, GroupCounts *counts) {
    check_group(s, count, "run_many");
    if (!out) throw std::runtime_error("run_many: null results");
    GroupCounts gc;
    {
        GroupScope scope(s, count);
        std::vector<LoopState> ls(static_cast<size_t>(count));
        std::vector<char> active(static_cast<size_t>(count), 1);
        for (int k = 0; k < count; ++k) s[k]->loop_begin(&ls[k], &out[k]);
        SmallTaskBuf buf;
        std::vector<SmallIterTask> tasks;
        int left = count;
        while (left > 0) {
            // 1-3: every active member's evaluation enqueued, one wait, then member by member what follows the wait
            for (int k = 0; k < count; ++k)
                if (active[k]) s[k]->loop_enqueue_evaluation(&ls[k]);
            HIP_CHECK(hipStreamSynchronize(scope.group));
            ++gc.rounds;
            ++gc.waits;
            tasks.clear();
            for (int k = 0; k < count; ++k) {
                if (!active[k]) continue;
                ++s[k]->fetches;
                // 4-5: the member's own decision; a restart runs its movement, copy, check step and weighted norm here (two
                // waits of its own: the exception to "one wait per round")
                if (!s[k]->loop_decide(&ls[k])) {
                    s[k]->loop_finish(&ls[k]);
                    active[k] = 0;
                    --left;
                    continue;
                }
                if (ls[k].restarted) gc.waits += 2;
                if (on_small_path(s[k]) && ls[k].pending > 0) tasks.push_back(SmallIterTask{s[k]->small_args(), 0, ls[k].pending});
            }
            // 6: the normal iterations of all small-path members, one launch per class
            gc.launches += launch_small_iterations_many(tasks.data(), static_cast<int>(tasks.size()), buf, scope.group);
            // 7: every member's own check step (members off the small path run their normal iterations first)
            for (int k = 0; k < count; ++k)
                if (active[k]) s[k]->loop_advance(&ls[k], on_small_path(s[k]));
        }
        for (int k = 0; k < count; ++k) s[k]->collect_solution(&out[k]);
    }
    if (counts) *counts = gc;
}

}  // namespace hprlp
