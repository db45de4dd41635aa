// many.cpp -- a group of independent solvers advanced in lock-step (DESIGN.md "Many small LPs").
//
// A Netlib-scale LP runs as one workgroup (small.hip) and keeps one CU of 256 busy.  K such LPs, each with its own matrix, are
// advanced together here: one k_small_iterations_many launch per <KMAX, R> class carries the normal iterations of every member
// (workgroup b = member b, the single-LP kernel's arithmetic on the member's own arguments).  Check step, evaluation and restart
// run in the group forms of the regular kernels (kernels.h: GroupLaunches -- one launch per kernel for all members, a workgroup
// running the single kernel's body as workgroup lb of lg of its member), and one copy and one host wait serve the scalars of all
// members.  The host side -- stopping test, restart rule, sigma update, detection -- is the member's own code (the pieces of
// Solver::solve_loop), so a member's iterates and results are the bits it gets alone.  A member that cannot join the group launches
// (Solver::joins_group) issues its own launches inside the same lock-step; so does every member for its iteration-0 evaluation
// (resolve_many apart: the group re-solve further down).  The ray tests of the infeasibility detection and the certificates of the
// members that join are the group's as well (DESIGN.md "Many small LPs", group detection).  New matrix values for the whole group
// (set_matrix_values_many) share scale_many's walk of Solver::scale() (scale_walk).  Each of the three group entries for new data,
// re-solve and new values has a twin with the vectors in the caller's device memory (DESIGN.md "Many small LPs", group device
// re-solve): the two share their steps, one body per pair where the arrangement allows (the second half of this file).
// A member off the small path that asked for it (Solver::group_wide; DESIGN.md "Many small LPs", wide members) joins the group
// launches all the same: its normal iterations run as recorded segments of the group kinds of the normal half-steps
// (record_normal), its power iteration's regular path in group launches (power_wide).
//
// Ordering is by stream: for the duration of a call every member works on ONE stream (the first member's), after its own stream
// has been waited for once; the members' streams come back at exit, after one wait for the group's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>

#include "many.h"
#include "group_pack.h"
#include "group_table.h"
#include "values.h"

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

thread_local WideCounts g_wide;

// The normal iterations counts[i] of the wide members who[i], recorded: segment by segment (group_table.h: group_iteration_plan)
// the x-halves of the segment's members as one stage, their y-halves as the next, the two issued `len` times from one table each.
// A member's iterations follow each other in the order of its own launches; a segment with one member goes through that member's
// own k_spmv_fused launches (the recorder's own-launch rule).  The caller records the check steps behind them.
void record_normal(Solver **s, const std::vector<int> &who, const std::vector<int> &counts, GroupLaunches &gl) {
    if (who.size() == 1) {
        // One wide member in the whole round (a group of one, or the last one still running): what it issues alone, its graph
        // replays, at once -- everything recorded for it so far has run, and its check step, recorded next, runs behind them.
        // (Enqueued one by one the same iterations cost 0.025 s against 0.018 s per 2000: profiles/many_wide_ab.txt, K = 1.)
        s[who[0]]->run_normal(counts[0]);
        return;
    }
    std::vector<int> len, at;
    const int segs = group_iteration_plan(counts.data(), static_cast<int>(counts.size()), len, at);
    for (int j = 0; j < segs; ++j) {
        long members = 0;
        for (int half = 0; half < 2; ++half) {
            for (size_t i = 0; i < who.size(); ++i)
                if (counts[i] >= at[j]) {
                    s[who[i]]->normal_half(half == 1, gl);
                    members += half;
                }
            gl.next_stage();  // (the y-half gathers what the x-half stores, the next x-half what the y-half stores)
        }
        gl.repeat_last(2, len[j]);
        g_wide.normal_launches += 2L * len[j];
        ++g_wide.segments;
        g_wide.member_iterations += members * len[j];
    }
}

std::vector<char> who_joins(Solver **s, int count) {
    std::vector<char> j(static_cast<size_t>(count));
    for (int k = 0; k < count; ++k) j[k] = s[k]->joins_group() ? 1 : 0;
    return j;
}

// Solver::power_iteration's regular path for the wide members `who` (two at least, all joining) in group launches.  The pieces are
// the member's own (Solver::power_norm / power_piece / power_err), a stage each: every one reads what the one before it wrote.
// A block is ten iterations -- three stages recorded once, issued ten times -- and the error terms, then one copy of the scalars and
// one wait for all members; each member's stopping test is its own, and a member that stopped is in no later block.  What is
// left of a max_iter that is no multiple of ten runs as the member's own path runs it: single iterations, no error terms, no
// fetch.  lambda is the last fetched one (1.0 if there was no block), as alone.
void power_wide(Solver **s, const std::vector<int> &who, int max_iter, double tol, double *lambda_out, int *iters_out, hipStream_t st,
                clock_type::time_point t0) {
    GroupLaunches gl;
    for (int k : who) {
        Solver &m = *s[k];
        m.finish_tiling();
        m.invalidate_far();
        m.power_start(m.sm1.p);
        m.power_norm(&gl);
        if (lambda_out) lambda_out[k] = 1.0;
    }
    gl.next_stage();
    std::vector<int> active = who, next;
    auto record_iterations = [&](int times) {
        for (int piece = 0; piece < 3; ++piece) {
            for (int k : active) s[k]->power_piece(piece, &gl);
            gl.next_stage();
        }
        gl.repeat_last(3, times);
    };
    int i = 0;
    for (; !active.empty() && i + 10 <= max_iter; i += 10) {
        record_iterations(10);
        for (int k : active) {
            s[k]->power_err(&gl);
            gl.pack(s[k]->scal.p, s[k]->scal_h.p);
        }
        g_wide.power_launches += gl.run(st);
        g_wide.power_launches += gl.fetch(st);  // (the packing kernel)
        HIP_CHECK(hipStreamSynchronize(st));
        ++g_wide.power_waits;
        gl.deliver();
        next.clear();
        for (int k : active) {
            Solver &m = *s[k];
            ++m.fetches;
            if (lambda_out) lambda_out[k] = m.scal_h[S_PW_QZ];
            if (std::sqrt(m.scal_h[S_PW_ERR2]) < tol) m.power_iters = i + 10;
            else next.push_back(k);
        }
        active.swap(next);
    }
    if (!active.empty() && i < max_iter) record_iterations(max_iter - i);
    for (int k : active) s[k]->power_iters = max_iter;
    if (gl.recorded_launches() > 0) g_wide.power_launches += gl.run(st);
    // leave the scratch vectors clean
    for (int k : who) {
        HIP_CHECK(hipMemsetAsync(s[k]->gsm.p, 0, sizeof(double) * s[k]->m_pad, st));
        HIP_CHECK(hipMemsetAsync(s[k]->gsn.p, 0, sizeof(double) * s[k]->n_pad, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    ++g_wide.power_waits;
    for (int k : who) {
        s[k]->power_time = time_since(t0);  // the group's wall time
        if (iters_out) iters_out[k] = s[k]->power_iters;
    }
}

// what has been recorded and enqueued, then the one copy of the scalars, the wait and each member's scalars into its host block
void run_fetch_wait(GroupLaunches &gl, hipStream_t group, GroupCounts &gc) {
    const int copies = gl.fetch(group);
    gc.group_launches += copies;  // (the packing kernel)
    gc.copies += copies;
    HIP_CHECK(hipStreamSynchronize(group));
    ++gc.waits;
    gl.deliver();
}

// Solver::scale() walked for the members who[0 ..) at once (scale_many, set_matrix_values_many).  gl records with a table for every
// kind (own_launches = false) and may hold closed stages already: they run in front of the scaling, in the first copy of the
// tables.  Launches, waits and served members are added to sc; st is the group's stream.
void scale_walk(Solver **s, const std::vector<int> &who, GroupLaunches &gl, hipStream_t st, SetupCounts &sc) {
    const int nj = static_cast<int>(who.size());
    // The pieces are scale()'s own (solver.cpp), in its order, recorded into one GroupLaunches with a table for every kind
    // (inside a stage a kind may hold one member's task).  The group's own:
    // the stages, one block for the second pairs of gathered vectors, and the sums block -- two slots per member, where the
    // pieces finalise |b|^2 and |c|^2 and from where one copy brings them to the host, three times.
    const auto t0 = time_now();
    std::vector<Solver::ScaleWalk> w(static_cast<size_t>(nj));
    auto member = [&](int j) -> Solver & { return *s[who[j]]; };
    // the second pair of gathered vectors of every member with Ruiz passes, pieces of one block
    auto aligned = [](size_t doubles) { return (doubles + 31) / 32 * 32; };
    size_t pair_doubles = 0;
    for (int j = 0; j < nj; ++j)
        if (member(j).prm.use_Ruiz_scaling) pair_doubles += aligned(static_cast<size_t>(member(j).m_pad)) + aligned(static_cast<size_t>(member(j).n_pad));
    DBuf<double> pairs(std::max<size_t>(pair_doubles, 1)), sums(static_cast<size_t>(2) * nj);
    HBuf<double> sums_h;
    sums_h.alloc(static_cast<size_t>(2) * nj);
    auto run_fetch_wait = [&]() {
        sc.scale_launches += gl.run(st);
        HIP_CHECK(hipMemcpyAsync(sums_h.p, sums.p, sizeof(double) * 2 * nj, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ++sc.scale_waits;
    };
    // ---- the start of scale(): norms of the unscaled b and c
    size_t at = 0;
    for (int j = 0; j < nj; ++j) {
        Solver &m = member(j);
        w[j].sums = sums.p + 2 * j;
        if (m.prm.use_Ruiz_scaling) {
            w[j].gm_next = pairs.p + at;
            at += aligned(static_cast<size_t>(m.m_pad));
            w[j].gn_next = pairs.p + at;
            at += aligned(static_cast<size_t>(m.n_pad));
        }
        m.scale_begin(&w[j], &gl);
    }
    run_fetch_wait();
    for (int j = 0; j < nj; ++j) member(j).scale_norms_org(sums_h.p + 2 * j);
    // ---- Curtis-Reid: twenty sweeps over A and A^T (two tables, issued twenty times), exp / clamp, the scaling pass
    auto each_cr = [&](auto piece) {
        for (int j = 0; j < nj; ++j)
            if (member(j).prm.use_CR_scaling) piece(member(j), &w[j]);
        gl.next_stage();
    };
    bool any_cr = false;
    for (int j = 0; j < nj; ++j) any_cr = any_cr || member(j).prm.use_CR_scaling;
    if (any_cr) {
        each_cr([&](Solver &m, Solver::ScaleWalk *v) { m.scale_cr_sweep(v, false, &gl); });
        each_cr([&](Solver &m, Solver::ScaleWalk *v) { m.scale_cr_sweep(v, true, &gl); });
        gl.repeat_last(2, 20);
        each_cr([&](Solver &m, Solver::ScaleWalk *v) { m.scale_cr_exp(v, &gl); });
        each_cr([&](Solver &m, Solver::ScaleWalk *v) { m.scale_cr_apply(v, &gl); });
    }
    // ---- Ruiz (ten passes) and Pock-Chambolle (one); a member's pass `it` is its own whatever the others' switches are
    int most = 0;
    for (const Solver::ScaleWalk &v : w) most = std::max(most, v.passes);
    for (int it = 0; it < most; ++it) {
        for (int j = 0; j < nj; ++j) member(j).scale_pass(&w[j], it, &gl);
        gl.next_stage();
    }
    // ---- b / c scaling: the second round trip, for the members that have it
    bool any_bc = false;
    for (int j = 0; j < nj; ++j) {
        if (!member(j).prm.use_bc_scaling) continue;
        any_bc = true;
        member(j).scale_sums(&w[j], &gl, nullptr);
    }
    if (any_bc) run_fetch_wait();
    for (int j = 0; j < nj; ++j) member(j).scale_bc_apply(sums_h.p + 2 * j, &gl);
    gl.next_stage();
    // ---- the norms of the scaled b and c, the bound codes, then the two gathered vectors back to zero
    for (int j = 0; j < nj; ++j) member(j).scale_finish(&w[j], &gl, nullptr);
    gl.next_stage();
    for (int j = 0; j < nj; ++j) member(j).scale_end(&gl);
    run_fetch_wait();
    for (int j = 0; j < nj; ++j) {
        Solver &m = member(j);
        m.scale_norms(sums_h.p + 2 * j);
        m.scal_h[S_TMP0] = sums_h[2 * j + 1];         // (what the member's own last fetch leaves in its host block)
        m.fetches += m.prm.use_bc_scaling ? 6 : 4;    // (the scalar fetches of its own scale())
        m.scaling_time = time_since(t0);              // the group's wall time
        m.scaled = true;
        ++sc.served;
    }
}

}  // namespace

void check_group(Solver *const *s, int count, const char *who, bool need_scaled) {
    const std::string w(who);
    if (!s) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    for (int k = 0; k < count; ++k) {
        if (!s[k]) throw std::runtime_error(w + ": member " + std::to_string(k) + " is null");
        if (s[k]->comm) throw std::runtime_error(w + ": member " + std::to_string(k) + " is a sharded solver; a group runs on one GPU");
        if (need_scaled && !s[k]->scaled) throw std::runtime_error(w + ": member " + std::to_string(k) + " was never scaled (hprlp_solver_scale)");
        if (s[k]->prm.device_number != s[0]->prm.device_number)
            throw std::runtime_error(w + ": member " + std::to_string(k) + " lives on another device than member 0");
        for (int j = 0; j < k; ++j)
            if (s[j] == s[k]) throw std::runtime_error(w + ": members " + std::to_string(j) + " and " + std::to_string(k) + " are the same solver");
    }
    // (the call goes on: its wide members, for hprlp_last_many_wide_counts)
    WideCounts wc;
    for (int k = 0; k < count; ++k)
        if (s[k]->group_wide && !on_small_path(s[k])) ++(s[k]->joins_group() ? wc.joined : wc.refused);
    if (wc.joined + wc.refused > 0) g_wide = wc;
}

WideCounts &last_wide_counts() { return g_wide; }

void scale_many(Solver **s, int count, SetupCounts *counts) {
    check_group(s, count, "scale_many", false);
    SetupCounts sc;
    GroupScope scope(s, count);
    const bool fused_norms = env_get("HPRLP_NO_FUSED_NORMS") == nullptr;  // (separate norm passes: the member scales on its own)
    std::vector<int> who;
    for (int k = 0; k < count; ++k)
        if (fused_norms && s[k]->joins_group() && s[k]->m_loc > 0 && s[k]->n_loc > 0) who.push_back(k);
    if (who.size() < 2) who.clear();  // (a group of one issues the member's own launches)
    std::vector<char> joins(static_cast<size_t>(count), 0);
    for (int k : who) joins[k] = 1;
    const long launches_before = scaling_launch_count();
    for (int k = 0; k < count; ++k) {
        if (joins[k]) continue;
        const long f0 = s[k]->fetches;
        s[k]->scale();
        sc.scale_waits += s[k]->fetches - f0 + 1;  // (its scalar fetches and its final wait)
        ++sc.own;
    }
    sc.scale_launches += scaling_launch_count() - launches_before;
    if (!who.empty()) {
        GroupLaunches gl(/*own_launches=*/false);
        scale_walk(s, who, gl, scope.group, sc);
    }
    if (counts) *counts = sc;
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
    // ---- wide members that join: the regular path in group launches (a group of one issues the member's own launches below)
    std::vector<int> wide;
    for (int k = 0; k < count; ++k)
        if (!on_small_path(s[k]) && s[k]->joins_group()) wide.push_back(k);
    if (wide.size() >= 2) {
        power_wide(s, wide, max_iter, tol, lambda_out, iters_out, scope.group, t0);
        for (int k : wide) done[k] = 1;
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
    const std::vector<char> joins = who_joins(s, count);
    // (wide members that join: their iterations recorded in segments, the check steps behind them; everybody else off the small path
    // on their own)
    std::vector<int> wide, wide_counts;
    for (int k = 0; k < count; ++k) {
        if (on_small_path(s[k])) continue;
        if (joins[k] && normal[k] > 0) wide.push_back(k), wide_counts.push_back(normal[k]);
        else if (!joins[k]) s[k]->run_normal(normal[k]);
    }
    GroupLaunches gl;
    record_normal(s, wide, wide_counts, gl);
    if (then_check)
        for (int k = 0; k < count; ++k) s[k]->step(true, joins[k] ? &gl : nullptr);
    gl.run(scope.group);
    HIP_CHECK(hipStreamSynchronize(scope.group));
}

void residuals_many(Solver **s, int count, const int *iter, const int *compute_gap, double *out) {
    check_group(s, count, "residuals_many");
    if (!iter || !compute_gap || !out) throw std::runtime_error("residuals_many: null iter, compute_gap or out");
    for (int k = 0; k < count; ++k)
        if (iter[k] < 0) throw std::runtime_error("residuals_many: iter[" + std::to_string(k) + "] is negative");
    GroupScope scope(s, count);
    const std::vector<char> joins = who_joins(s, count);
    GroupLaunches gl;
    GroupCounts gc;
    for (int k = 0; k < count; ++k) {
        s[k]->residuals_launch(iter[k], compute_gap[k] != 0, joins[k] && iter[k] > 0 ? &gl : nullptr);
        gl.pack(s[k]->scal.p, s[k]->scal_h.p);
    }
    gl.run(scope.group);
    run_fetch_wait(gl, scope.group, gc);
    for (int k = 0; k < count; ++k) {
        Residuals r;
        RestartState rs;
        ++s[k]->fetches;
        s[k]->residuals_consume(iter[k], compute_gap[k] != 0, &r, &rs);
        double *o = out + 8 * static_cast<size_t>(k);
        o[0] = r.err_Rp; o[1] = r.err_Rd; o[2] = r.primal_obj; o[3] = r.dual_obj;
        o[4] = r.rel_gap; o[5] = r.kkt; o[6] = rs.current_gap; o[7] = s[k]->lambda_max;
    }
}

void restart_many(Solver **s, int count, const double *in, double *sigma_out) {
    check_group(s, count, "restart_many");
    if (!in) throw std::runtime_error("restart_many: null input");
    GroupScope scope(s, count);
    const std::vector<char> joins = who_joins(s, count);
    GroupLaunches gl;
    GroupCounts gc;
    for (int k = 0; k < count; ++k) {
        s[k]->movement_launch(joins[k] ? &gl : nullptr);
        gl.pack(s[k]->scal.p, s[k]->scal_h.p);
    }
    gl.run(scope.group);
    run_fetch_wait(gl, scope.group, gc);
    for (int k = 0; k < count; ++k) {
        const double *v = in + 6 * static_cast<size_t>(k);
        RestartState rs;  // (as hprlp_solver_restart)
        rs.flag = 1;
        rs.first = false;
        rs.current_gap = v[0]; rs.best_gap = v[1]; rs.best_sigma = v[2];
        Residuals r;
        r.err_Rd = v[3]; r.err_Rp = v[4]; r.rel_gap = v[5];
        ++s[k]->fetches;
        s[k]->restart_launch(&rs, r, joins[k] ? &gl : nullptr);
    }
    gl.run(scope.group);
    HIP_CHECK(hipStreamSynchronize(scope.group));
    if (sigma_out)
        for (int k = 0; k < count; ++k) sigma_out[k] = s[k]->sigma;
}

void ray_step_many(Solver **s, int count, const int *restart, double *out, int *tested) {
    const char *who = "hprlp_solver_ray_step_many";
    // (the list, the count, the arrays and the members have been checked by the caller: abi.cpp owns those refusals)
    for (int k = 0; k < count; ++k)
        if (!restart[k] && !s[k]->ray_prev_x.p)
            throw std::runtime_error(std::string(who) + ": member " + std::to_string(k) + ": the first step of a solver needs restart != 0");
    GroupScope scope(s, count);
    const std::vector<char> joins = who_joins(s, count);
    GroupLaunches gl;
    GroupCounts gc;
    for (int k = 0; k < count; ++k) {
        GroupLaunches *g = joins[k] ? &gl : nullptr;
        if (restart[k]) s[k]->ray_begin(g);
        s[k]->residuals_launch(1, true, g);
        tested[k] = s[k]->ray_test(g) ? 1 : 0;  // (a member outside the group: its own launches, behind its own evaluation)
        gl.pack(s[k]->scal.p, s[k]->scal_h.p);
    }
    gl.run(scope.group);
    run_fetch_wait(gl, scope.group, gc);
    const int slots[9] = {S_RAY_DY, S_RAY_CD, S_RAY_VY, S_RAY_WD, S_RAY_YN, S_RAY_DN, S_RAY_DZ, S_RAY_VZ, S_RAY_WQ};
    for (int k = 0; k < count; ++k) {
        Residuals r;
        RestartState rs;
        ++s[k]->fetches;
        s[k]->residuals_consume(1, true, &r, &rs);  // (as hprlp_solver_ray_step: the evaluation a periodic check runs)
        if (!tested[k]) continue;
        for (int i = 0; i < 9; ++i) out[9 * static_cast<size_t>(k) + i] = s[k]->scal_h[slots[i]];
    }
}

namespace {

// The lock-step loop of run_many from every member's current state, up to loop_finish (the solutions are the caller's).  gl may
// hold records already (resolve_many: zeroing, ctrl, starts): they run in front of the first evaluation, in the same copy of the
// tables.  iter0 (null: nobody): the members whose iteration-0 evaluation is recorded into the group as well -- only resolve_many
// sets it; for everybody else iteration 0 is a member's own, as it always was.
void loop_many(Solver **s, int count, HPRLP_results *out, GroupCounts &gc, GroupScope &scope, const std::vector<char> &joins, GroupLaunches &gl,
               const char *iter0) {
    std::vector<LoopState> ls(static_cast<size_t>(count));
    std::vector<char> active(static_cast<size_t>(count), 1);
    // (a joining member's first detection run: its ray vectors zeroed by recorded fills, ahead of the first evaluation)
    for (int k = 0; k < count; ++k) s[k]->loop_begin(&ls[k], &out[k], joins[k] ? &gl : nullptr);
    SmallTaskBuf buf;
    std::vector<SmallIterTask> tasks;
    std::vector<int> flagged, verdicts, wide, wide_counts;
    std::vector<PackMember> cm;  // the certificate block of a round with verdicts: device, and pinned
    DBuf<double> cert_d;
    HBuf<double> cert_h;
    // (between two rounds gl holds the check steps recorded in step 11: they run with the next evaluation, a stage ahead)
    auto in_group = [&](int k) { return joins[k] && (ls[k].iter > 0 || (iter0 && iter0[k])); };
    int left = count;
    while (left > 0) {
        // 1-3: the evaluation of every active member and, where detection asks for one, its ray test in the same stage
        // (kernels.hip: GroupKinds); one copy of the scalars, one wait.  Iteration 0 (launch_lu, a start's evaluation) is a
        // member's own, and so is everything of a member outside the group launches, its ray test included.
        for (int k = 0; k < count; ++k) {
            if (!active[k]) continue;
            if (in_group(k)) {
                s[k]->loop_enqueue_evaluation(&ls[k], &gl);
                ++gc.served;
                if (s[k]->loop_enqueue_ray(&ls[k], &gl)) ++gc.ray_served;
            }
            gl.pack(s[k]->scal.p, s[k]->scal_h.p);
        }
        gc.group_launches += gl.run(scope.group);
        for (int k = 0; k < count; ++k) {
            if (!active[k] || in_group(k)) continue;
            s[k]->loop_enqueue_evaluation(&ls[k], nullptr, false);  // (between the group's kernels and the group's copy)
            ++gc.own;
        }
        run_fetch_wait(gl, scope.group, gc);
        ++gc.rounds;
        // 4: every member's status and restart flag; finished members drop out
        flagged.clear();
        verdicts.clear();
        for (int k = 0; k < count; ++k) {
            if (!active[k]) continue;
            ++s[k]->fetches;
            if (!s[k]->loop_status(&ls[k])) {
                active[k] = 0;
                --left;
                if (ls[k].verdict && joins[k]) {
                    verdicts.push_back(k);  // (finished below, once the group's block is back)
                    continue;
                }
                if (ls[k].verdict) ++gc.own;
                s[k]->loop_certificate(&ls[k]);
                s[k]->loop_finish(&ls[k]);
                continue;
            }
            if (ls[k].restarted) flagged.push_back(k);
        }
        if (!verdicts.empty()) {
            // 4b: the certificates of this round's verdicts among the joining members: the raw arrays of all of them into one
            // device block (copies, and A^T y_s by the plain product straight into it), one copy, one wait, then each member's own
            // finish_certificate and un-permutation
            cm.assign(static_cast<size_t>(count), PackMember());
            for (int k : verdicts) cm[k].m = s[k]->m_loc, cm[k].n = s[k]->n_loc, cm[k].cert = ls[k].verdict;
            const GroupPackLayout L = group_pack_layout(cm.data(), count);
            if (cert_d.n < L.cert_doubles) {
                cert_d.alloc(2 * L.cert_doubles);
                cert_h.alloc(2 * L.cert_doubles, false);
            }
            auto dev = [&](size_t off) { return off == kPackAbsent ? nullptr : cert_d.p + off; };
            auto host = [&](size_t off) { return off == kPackAbsent ? nullptr : cert_h.p + off; };
            for (int k : verdicts) {
                const PackSlot &p = L.slot[k];
                s[k]->certificate_launch(ls[k].verdict, dev(p.cert_rn), dev(p.cert_cn), dev(p.cert_ray), dev(p.cert_aty), &gl);
            }
            gc.group_launches += gl.run(scope.group);
            HIP_CHECK(hipMemcpyAsync(cert_h.p, cert_d.p, sizeof(double) * L.cert_doubles, hipMemcpyDeviceToHost, scope.group));
            ++gc.copies;
            HIP_CHECK(hipStreamSynchronize(scope.group));
            ++gc.waits;
            for (int k : verdicts) {
                const PackSlot &p = L.slot[k];
                s[k]->certificate_consume(ls[k].verdict, ls[k].verdict_iter, host(p.cert_rn), host(p.cert_cn), host(p.cert_ray), host(p.cert_aty));
                ++gc.certs_served;
                s[k]->loop_finish(&ls[k]);
            }
        }
        if (!flagged.empty()) {
            // 5-6: movement of the flagged members
            for (int k : flagged) {
                s[k]->loop_movement(&ls[k], joins[k] ? &gl : nullptr);
                if (!joins[k]) ++gc.own;
                gl.pack(s[k]->scal.p, s[k]->scal_h.p);
            }
            gc.group_launches += gl.run(scope.group);
            run_fetch_wait(gl, scope.group, gc);
            // 7-9: each one's sigma rule on the host; restart copy, ctrl, check step and gap
            for (int k : flagged) {
                ++s[k]->fetches;
                s[k]->loop_restart(&ls[k], joins[k] ? &gl : nullptr);
                if (!joins[k]) ++gc.own;
                gl.pack(s[k]->scal.p, s[k]->scal_h.p);
            }
            gc.group_launches += gl.run(scope.group);
            run_fetch_wait(gl, scope.group, gc);
            for (int k : flagged) ++s[k]->fetches;
        }
        // 10: the normal iterations of all small-path members, one launch per class; those of the wide members that join, recorded
        // in segments (they run with the check steps, in front of the next round's evaluation)
        tasks.clear();
        wide.clear();
        wide_counts.clear();
        for (int k = 0; k < count; ++k) {
            if (!active[k]) continue;
            s[k]->loop_plan(&ls[k]);  // (a restart's weighted norm consumed: the rare lambda bump inside is the member's own launch)
            if (ls[k].pending <= 0) continue;
            if (on_small_path(s[k])) tasks.push_back(SmallIterTask{s[k]->small_args(), 0, ls[k].pending});
            else if (joins[k]) wide.push_back(k), wide_counts.push_back(ls[k].pending);
        }
        const int it_launches = launch_small_iterations_many(tasks.data(), static_cast<int>(tasks.size()), buf, scope.group);
        gc.launches += it_launches;
        gc.group_launches += it_launches;
        record_normal(s, wide, wide_counts, gl);
        // 11: the check step: recorded for the members of the group launches (it runs in front of the next round's evaluation,
        // same stream); members outside them run their normal iterations first
        for (int k = 0; k < count; ++k) {
            if (!active[k]) continue;
            s[k]->loop_advance(&ls[k], on_small_path(s[k]) || joins[k], joins[k] ? &gl : nullptr);
            if (!joins[k] && ls[k].pending >= 0) ++gc.own;
        }
        gl.next_stage();  // (the evaluation's Rd overwrites the partials the check step's finalize reads)
    }
}

}  // namespace

void run_many(Solver **s, int count, HPRLP_results *out, GroupCounts *counts) {
    check_group(s, count, "run_many");
    if (!out) throw std::runtime_error("run_many: null results");
    GroupCounts gc;
    {
        GroupScope scope(s, count);
        const std::vector<char> joins = who_joins(s, count);
        GroupLaunches gl;
        loop_many(s, count, out, gc, scope, joins, gl, nullptr);
        for (int k = 0; k < count; ++k) s[k]->collect_solution(&out[k]);
    }
    if (counts) *counts = gc;
}

// ------------------------------------------------------------------------------------------------
// group re-solve, group matrix values and group device re-solve (DESIGN.md "Many small LPs"): set_data, resolve and
// set_matrix_values of every member of a group, with the members' vectors in host memory or in device memory of the caller's.
// The rule is the group launches': a workgroup runs the single kernel's body as workgroup lb of its member's own grid (the bodies
// of values.hip's kernels included), the zeroing is reset_iterates' fills, the scaling is scale_many's walk, so every stored number
// is the member's own; what changes is who issues the launches, how the caller's vectors travel and how often the host waits
// (once per call outside the loop, never once per member).  A host entry and its device twin are ONE body over a Source (below):
// the shared steps are written once, and where the body branches on the source a comment names the difference.
// ------------------------------------------------------------------------------------------------
// The blocks of a group call, kept with member 0 (the owner of the group's stream) and grown on demand: staging of the data / the
// starts (pinned, and its device copy), the data passes' partials, the solutions (device, and pinned), the launch tables.
struct GroupBlocks {
    SmallTaskBuf in;
    DBuf<double> parts, out_d;
    HBuf<double> out_h;
    GroupLaunches gl;
    // set_matrix_values: the recorder with a table for every kind (what scale_walk asks for); the flag words of a check stage
    GroupLaunches tables{/*own_launches=*/false};
    DBuf<unsigned long long> flags;
    HBuf<unsigned long long> flags_h;
    // the device entries: the event recorded on the caller's stream
    hipEvent_t inputs_ready = nullptr;
    GroupBlocks() = default;
    GroupBlocks(const GroupBlocks &) = delete;
    GroupBlocks &operator=(const GroupBlocks &) = delete;
    ~GroupBlocks() {
        if (inputs_ready) (void)hipEventDestroy(inputs_ready);
    }
};

namespace {

// What tells a host group entry from its device twin.  A host entry reads pieces of the pinned staging block after one copy,
// checks the vectors with host loops, copies the solutions back in one block, and a member that goes its own way runs
// Solver::set_data / resolve / set_matrix_values.  A device entry reads the caller's buffers after one event wait on `caller`,
// looks every pointer up (PointerChecks) and checks the vectors where they lie in one stage (check_stage), stores the solutions
// into the caller's buffers, and a member on its own runs Solver::set_data_device / resolve_device / set_matrix_values_device.
// The nominal counts of those single entries differ and stay next to the calls.
struct Source {
    const char *who;               // the entry's name, in front of every message
    hipStream_t caller = nullptr;  // a device entry: the stream the inputs were produced on
    DeviceCounts *dc = nullptr;    // a device entry: filled as the call proceeds, so it also tells what a refused call did
    bool device() const { return dc != nullptr; }
};

GroupBlocks &blocks_of(Solver *owner) {
    if (!owner->group_blocks) owner->group_blocks = std::make_shared<GroupBlocks>();
    return *owner->group_blocks;
}

// The cleanup shell of a group call: on a throw the owner's blocks go, and whatever was recorded into them goes with them.
struct DropBlocksOnThrow {
    Solver *owner;  // null: the call holds no blocks
    int live = std::uncaught_exceptions();
    ~DropBlocksOnThrow() {
        if (owner && std::uncaught_exceptions() > live) owner->group_blocks.reset();
    }
};

std::string member(const char *who, int k) { return std::string(who) + ": member " + std::to_string(k); }

// The members of the group launches: the wanted ones, two at least (a group of one issues the member's own launches).
std::vector<int> joiners(const std::vector<char> &wanted, std::vector<char> &mask) {
    std::vector<int> in;
    for (size_t k = 0; k < wanted.size(); ++k)
        if (wanted[k]) in.push_back(static_cast<int>(k));
    if (in.size() < 2) in.clear();
    mask.assign(wanted.size(), 0);
    for (int k : in) mask[k] = 1;
    return in;
}

// ---- the checks of host vectors: a host entry's only (a device entry's vectors are checked where they lie, check_stage)
void host_scan(const char *who, int k, const double *v, long len, const char *what, bool finite, const char *verdict) {
    for (long i = 0; v && i < len; ++i)
        if (finite ? !std::isfinite(v[i]) : std::isnan(v[i]))
            throw std::runtime_error(member(who, k) + ": " + what + "[" + std::to_string(i) + "] " + verdict);
}
void host_no_nan(const char *who, int k, const Solver &m, const double *c, const double *AL, const double *AU, const double *l, const double *u) {
    const struct { const double *v; long len; const char *what; } vecs[5] = {{c, m.n, "c"}, {AL, m.m, "AL"}, {AU, m.m, "AU"}, {l, m.n, "l"}, {u, m.n, "u"}};
    for (const auto &e : vecs) host_scan(who, k, e.v, e.len, e.what, false, "is NaN");
}

// ---- the checks of a device entry
// The pointer checks of one call.  A pointer that lies, with its length, inside a range the runtime has already reported in this
// call is device memory of the group's device with room for it: no second lookup (a group cut from a few packed tensors costs a
// few lookups whatever its size).  Everything else goes through check_device_pointer, whose words the refusal carries.
class PointerChecks {
  public:
    PointerChecks(int device, const char *who, DeviceCounts &dc) : device_(device), who_(who), dc_(dc) {}
    void operator()(int k, const void *p, size_t count, const char *name) {
        if (!p) return;  // (not given / not wanted)
        ++dc_.pointers;
        const char *b = static_cast<const char *>(p), *e = b + count * sizeof(double);
        if (reinterpret_cast<uintptr_t>(p) % sizeof(double) == 0)
            for (const DeviceRange &r : seen_)
                if (b >= r.base && e <= r.base + r.bytes) return;
        ++dc_.lookups;
        DeviceRange r;
        check_device_pointer(p, count, device_, name, member(who_, k).c_str(), &r);
        if (r.bytes > 0) seen_.push_back(r);
    }
    void data_vectors(int k, size_t m, size_t n, const double *c, const double *AL, const double *AU, const double *l, const double *u) {
        (*this)(k, c, n, "c"); (*this)(k, AL, m, "AL"); (*this)(k, AU, m, "AU"); (*this)(k, l, n, "l"); (*this)(k, u, n, "u");
    }

  private:
    int device_;
    const char *who_;
    DeviceCounts &dc_;
    std::vector<DeviceRange> seen_;
};

// The group's stream waits for what the caller's stream has been given so far (one event per call).
void wait_for_caller(GroupBlocks &gb, hipStream_t caller, hipStream_t st) {
    if (!gb.inputs_ready) HIP_CHECK(hipEventCreateWithFlags(&gb.inputs_ready, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(gb.inputs_ready, caller));
    HIP_CHECK(hipStreamWaitEvent(st, gb.inputs_ready, 0));
}

// ---- the flag block.  `words` flag words of all ones (kDataCheckClean, kValuesAllFinite) by ONE memset; fetch_flags: one copy,
// one wait
unsigned long long *cleared_flags(GroupBlocks &gb, size_t words, hipStream_t st) {
    if (gb.flags.n < words) {
        gb.flags.alloc(words);
        gb.flags_h.alloc(words);
    }
    HIP_CHECK(hipMemsetAsync(gb.flags.p, 0xff, sizeof(unsigned long long) * words, st));
    return gb.flags.p;
}
const unsigned long long *fetch_flags(GroupBlocks &gb, size_t words, hipStream_t st) {
    HIP_CHECK(hipMemcpyAsync(gb.flags_h.p, gb.flags.p, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return gb.flags_h.p;
}
// One check stage, before the first write of anything a solver reads: the cleared words, what `record` records against them as ONE
// stage of the group's launches, the words back.  Counted into the call's counts and, for a device entry, into dc.
template <class Record>
const unsigned long long *check_stage(GroupBlocks &gb, size_t words, hipStream_t st, CallCounts &c, DeviceCounts *dc, Record record) {
    unsigned long long *flags = cleared_flags(gb, words, st);
    ++c.memsets;
    GroupLaunches &chk = gb.gl;
    const long tables0 = chk.tables_sent();
    record(chk, flags);
    const int launches = chk.run(st);
    c.launches += launches;
    if (dc) dc->check_launches += launches;
    c.h2d += chk.tables_sent() - tables0;
    const unsigned long long *back = fetch_flags(gb, words, st);
    ++c.d2h, ++c.waits;
    if (dc) dc->flags += static_cast<long>(words), ++dc->waits_before_write;
    return back;
}
DataCheckArgs nan_check(int m, int n, const double *c, const double *AL, const double *AU, const double *l, const double *u) {
    return DataCheckArgs{{c, AL, AU, l, u}, {n, m, m, n, n}, 0};
}
// k_data_check's word of member k as the host group entries' message
void throw_if_flagged(unsigned long long word, const char *const names[kDataCheckVecs], const std::string &who, const char *what) {
    if (word == kDataCheckClean) return;
    const int v = static_cast<int>(word >> kDataCheckShift);
    const unsigned long long i = word & ((1ULL << kDataCheckShift) - 1);
    throw std::runtime_error(who + ": " + (v < kDataCheckVecs ? names[v] : "?") + "[" + std::to_string(i) + "] " + what);
}
const char *const kDataNames[kDataCheckVecs] = {"c", "AL", "AU", "l", "u"};  // (the host entries' order of vectors)
const char *const kStartNames[kDataCheckVecs] = {"x0", "y0", "", "", ""};

// ------------------------------------------------------------------------------------------------
// set_data_many / set_data_many_device
// ------------------------------------------------------------------------------------------------
// The two data passes of the members `in`: recorded, run, the scalars packed and fetched, ONE wait, then each member's host
// formulas.  at[k]: where member k's given vectors are read on the device -- pieces of the staging block, or the caller's own
// buffers; data[k].obj_constant is host memory either way.
void data_passes(Solver **s, const std::vector<int> &in, const std::vector<PackMember> &pm, const MemberData *data, const MemberData *at,
                 GroupBlocks &gb, hipStream_t st, ResolveCounts &rc, clock_type::time_point t0, const Source &src) {
    const int nj = static_cast<int>(in.size());
    const size_t per = static_cast<size_t>(4) * kReduceBlocks;
    if (gb.parts.n < per * nj) gb.parts.alloc(per * nj);
    GroupLaunches &gl = gb.gl;
    const long tables0 = gl.tables_sent();
    for (int j = 0; j < nj; ++j) {
        const int k = in[j];
        Solver &m = *s[k];
        m.data_time[0] = m.data_time[1] = m.data_time[2] = 0.0;
        if (data[k].obj_constant) m.obj_constant = *data[k].obj_constant;
        m.data_first_pass(at[k].AL, at[k].AU, at[k].l, at[k].u, at[k].c, pm[k].bounds, gb.parts.p + per * j, &gl);
    }
    gl.next_stage();  // (the second pass reads the sums the first pass' finalize leaves in the member's scalars)
    for (int j = 0; j < nj; ++j) {
        const int k = in[j];
        s[k]->data_second_pass(pm[k].bounds, pm[k].c, gb.parts.p + per * j, &gl);
        gl.pack(s[k]->scal.p, s[k]->scal_h.p);
    }
    rc.launches += gl.run(st);
    const int copies = gl.fetch(st);
    rc.launches += copies;  // (the packing kernel)
    rc.d2h += copies;
    rc.h2d += gl.tables_sent() - tables0;
    HIP_CHECK(hipStreamSynchronize(st));
    ++rc.waits;
    gl.deliver();
    const double wall = time_since(t0);  // the group call's wall time is every member's
    for (int k : in) {
        Solver &m = *s[k];
        ++m.fetches;
        m.data_consume(pm[k].bounds, pm[k].c);
        m.invalidate_far();
        m.data_time[1] = m.data_time[2] = wall;
        m.data_since_run += wall;
        // (the words that travelled: none for a device entry, the given vectors for a host entry)
        if (src.device()) m.set_transfer(0, 0, true);
        else
            m.set_transfer((pm[k].bounds ? 2 * static_cast<size_t>(m.m_loc) + 2 * static_cast<size_t>(m.n_loc) : 0) + (pm[k].c ? m.n_loc : 0), 0,
                           false);
        ++rc.served;
    }
}

void set_data_group(Solver **s, int count, const MemberData *data, const Source &src, ResolveCounts *counts) {
    const char *who = src.who;
    // (the list, the count, data and the members have been checked by the caller: abi.cpp owns those refusals, group_members)
    // ---- the host rules of all members (Solver::set_data's), before anything is launched or written
    bool any = false;
    for (int k = 0; k < count; ++k) {
        const MemberData &d = data[k];
        const bool bounds = d.AL || d.AU || d.l || d.u;
        if (bounds && !(d.AL && d.AU && d.l && d.u))
            throw std::runtime_error(member(who, k) + ": AL, AU, l and u are given together or not at all (b_scale couples them)");
        if (!src.device()) host_no_nan(who, k, *s[k], d.c, d.AL, d.AU, d.l, d.u);  // (host memory only)
        if (d.obj_constant && std::isnan(*d.obj_constant)) throw std::runtime_error(member(who, k) + ": obj_constant is NaN");
        any = any || d.c || bounds;
    }
    if (src.device()) {  // every pointer of every member: still nothing launched or written
        PointerChecks pass(s[0]->prm.device_number, who, *src.dc);
        for (int k = 0; k < count; ++k)
            pass.data_vectors(k, static_cast<size_t>(s[k]->m_loc), static_cast<size_t>(s[k]->n_loc), data[k].c, data[k].AL, data[k].AU, data[k].l, data[k].u);
    }
    ResolveCounts rc;
    const auto t0 = time_now();
    GroupScope scope(s, count);
    const hipStream_t st = scope.group;
    std::vector<PackMember> pm(static_cast<size_t>(count));
    std::vector<char> wanted(static_cast<size_t>(count)), joins;
    for (int k = 0; k < count; ++k) {
        pm[k].m = s[k]->m_loc, pm[k].n = s[k]->n_loc;
        pm[k].c = data[k].c != nullptr, pm[k].bounds = data[k].AL != nullptr;
        wanted[k] = (pm[k].c || pm[k].bounds) && s[k]->joins_group_resolve();
    }
    const std::vector<int> in = joiners(wanted, joins);
    for (int k = 0; k < count; ++k)
        if (!joins[k]) pm[k].c = pm[k].bounds = false;  // (no room in the group's block)
    // A device entry always takes the group's blocks (its check needs the flag words), a host entry once somebody joins.
    GroupBlocks *gb = src.device() || !in.empty() ? &blocks_of(s[0]) : nullptr;
    DropBlocksOnThrow drop{gb ? s[0] : nullptr};
    if (src.device() && any) {
        // ---- a device entry's check: the vectors of ALL members where they lie, one launch, one copy of the flag words, one wait
        wait_for_caller(*gb, src.caller, st);
        const unsigned long long *flags = check_stage(*gb, static_cast<size_t>(count), st, rc, src.dc, [&](GroupLaunches &chk, unsigned long long *w) {
            for (int k = 0; k < count; ++k) chk.data_check(nan_check(s[k]->m_loc, s[k]->n_loc, data[k].c, data[k].AL, data[k].AU, data[k].l, data[k].u), w + k);
        });
        for (int k = 0; k < count; ++k) throw_if_flagged(flags[k], kDataNames, member(who, k), "is NaN");  // (the lowest member first)
    }
    // -- from here on the call goes through
    // ---- the members that go their own way: the single entry of the source's kind
    for (int k = 0; k < count; ++k) {
        const MemberData &d = data[k];
        if (joins[k] || !(d.c || d.obj_constant || d.AL)) continue;  // (nothing given: the member keeps its bits)
        if (src.device()) s[k]->set_data_device(d.c, d.obj_constant, d.AL, d.AU, d.l, d.u, src.caller);
        else s[k]->set_data(d.c, d.obj_constant, d.AL, d.AU, d.l, d.u);
        if (!(d.c || d.AL)) continue;  // (obj_constant alone is a host assignment)
        ++rc.own;
        if (src.device()) {
            ++src.dc->own;
            // Solver::set_data_device, nominal (many.h: ResolveCounts): the flag's memset, its check, two passes and two finalizes;
            // the flag's copy and the scalars', a wait each
            rc.memsets += 1, rc.launches += 5, rc.d2h += 2, rc.waits += 2;
        } else {
            // Solver::set_data, nominal (many.h: ResolveCounts): the staging in one copy, or one per vector from the allocator cache's
            // block size on; two passes and two finalizes; the scalars' copy and its wait
            const size_t words = (d.AL ? 2 * static_cast<size_t>(s[k]->m_loc) + 2 * static_cast<size_t>(s[k]->n_loc) : 0) + (d.c ? s[k]->n_loc : 0);
            rc.h2d += words * sizeof(double) < kDeviceCacheMinBytes ? 1 : (d.AL ? 4 : 0) + (d.c ? 1 : 0);
            rc.launches += 4, rc.d2h += 1, rc.waits += 1;
        }
    }
    if (!in.empty()) {
        // ---- where the joiners' vectors are read: a device entry's in the caller's buffers, a host entry's in pieces of the
        // staging block after one copy
        std::vector<MemberData> staged;
        if (!src.device()) {
            const GroupPackLayout L = group_pack_layout(pm.data(), count);
            double *host = static_cast<double *>(gb->in.stage(sizeof(double) * L.data_doubles));
            for (int k : in) group_pack_data(L, k, pm[k], data[k].AL, data[k].AU, data[k].l, data[k].u, data[k].c, host);
            gb->in.send(sizeof(double) * L.data_doubles, st);
            ++rc.h2d;
            const double *dev = static_cast<const double *>(gb->in.dev);
            auto at = [&](size_t off) { return off == kPackAbsent ? nullptr : dev + off; };
            staged.resize(static_cast<size_t>(count));
            for (int k : in) {
                const PackSlot &p = L.slot[k];
                staged[k].c = at(p.c), staged[k].AL = at(p.AL), staged[k].AU = at(p.AU), staged[k].l = at(p.l), staged[k].u = at(p.u);
            }
        }
        data_passes(s, in, pm, data, src.device() ? data : staged.data(), *gb, st, rc, t0, src);
        if (src.device()) src.dc->served += static_cast<long>(in.size());
    }
    if (counts) *counts = rc;
}

}  // namespace

void set_data_many(Solver **s, int count, const MemberData *data, ResolveCounts *counts) {
    set_data_group(s, count, data, Source{"hprlp_solver_set_data_many"}, counts);
}
void set_data_many_device(Solver **s, int count, const MemberData *data, hipStream_t caller, ResolveCounts *counts, DeviceCounts *dcounts) {
    DeviceCounts unused;
    set_data_group(s, count, data, Source{"hprlp_solver_set_data_many_device", caller, dcounts ? dcounts : &unused}, counts);
}

// ------------------------------------------------------------------------------------------------
// resolve_many / resolve_many_device.  Two bodies over shared steps: the loop arrangements differ from the first member that goes
// its own way to the last solution (see each), and folded into one function nearly every line would sit under a branch.
// ------------------------------------------------------------------------------------------------
void check_starts(Solver *const *s, int count, const MemberStart *start, const char *who, bool host_vectors) {
    for (int k = 0; start && k < count; ++k) {
        if (std::isnan(start[k].sigma)) throw std::runtime_error(member(who, k) + ": sigma is NaN");
        if (!host_vectors) continue;  // (a device entry's starts are checked where they lie: resolve_many_device's check stage)
        host_scan(who, k, start[k].x0, s[k]->n, "warm start: x0", true, "is not finite");
        host_scan(who, k, start[k].y0, s[k]->m, "warm start: y0", true, "is not finite");
    }
}

namespace {

std::vector<int> resolve_joiners(Solver **s, int count, std::vector<char> &grouped) {
    std::vector<char> wanted(static_cast<size_t>(count));
    for (int k = 0; k < count; ++k) wanted[k] = s[k]->joins_group_resolve();
    return joiners(wanted, grouped);
}

// Zeroing, bound codes, ctrl (a sigma override included) and the starts of the joiners, recorded: they run in front of the first
// evaluation.  at[k]: where member k's start is read on the device -- pieces of the staging block, or the caller's own buffers.
void record_starts(Solver **s, const std::vector<int> &in, const MemberStart *start, const MemberStart *at, GroupLaunches &gl, ResolveCounts &rc) {
    for (int k : in) {
        Solver &m = *s[k];
        m.reset_iterates(&gl);
        m.init_iteration_state(&gl, start[k].sigma);
        if (start[k].x0 || start[k].y0) {
            m.invalidate_far();
            m.start_launch(at[k].x0, at[k].y0, nullptr, nullptr, &gl);
        }
    }
    rc.launches += gl.recorded_launches();
    gl.next_stage();  // (the evaluation's Rd / Rp overwrite the partials the start's finalize reads)
}

// The lock-step loop as Solver::resolve runs its own: the reported time starts from the set_data seconds since the previous loop.
void resolve_loop(Solver **s, int count, HPRLP_results *out, GroupCounts &gc, GroupScope &scope, const std::vector<char> &joins, GroupLaunches &gl,
                  const char *iter0) {
    struct TimeBase {
        Solver **s;
        int count;
        ~TimeBase() {
            for (int k = 0; k < count; ++k) s[k]->time_base = -1.0;
        }
    } tb{s, count};
    for (int k = 0; k < count; ++k) s[k]->time_base = s[k]->data_since_run;
    loop_many(s, count, out, gc, scope, joins, gl, iter0);
}

}  // namespace

// ALL members stay in one loop_many call -- `grouped` marks whose iteration-0 evaluation is the group's, the others ride along
// with their own launches (rc.loop_own) -- and the solutions are collected afterwards: the joiners' through one device block.
void resolve_many(Solver **s, int count, const MemberStart *start, HPRLP_results *out, ResolveCounts *counts) {
    std::vector<MemberStart> cold;
    if (!start) {
        cold.resize(static_cast<size_t>(count));
        start = cold.data();
    }
    ResolveCounts rc;
    GroupCounts gc;
    {
        GroupScope scope(s, count);
        const hipStream_t st = scope.group;
        const std::vector<char> joins = who_joins(s, count);
        std::vector<char> grouped;
        const std::vector<int> in = resolve_joiners(s, count, grouped);
        const int nj = static_cast<int>(in.size());
        // ---- the members that go their own way: Solver::resolve up to its loop
        for (int k = 0; k < count; ++k) {
            if (grouped[k]) continue;
            Solver &m = *s[k];
            const MemberStart &b = start[k];
            m.reset_iterates();
            m.init_iteration_state();
            if (b.sigma > 0.0) m.set_sigma_lambda(b.sigma, m.lambda_max, true);
            if (b.x0 || b.y0) m.set_start(b.x0, b.y0);
            ++rc.own;
            // (nominal, many.h: ResolveCounts -- what Solver::resolve issues for a member without a locality ordering)
            rc.memsets += 17, rc.waits += 1;                                        // reset_iterates
            rc.launches += (m.hook_no_bound_codes ? 0 : 2) + 1 + (b.sigma > 0.0 ? 1 : 0);  // bound codes, ctrl, the override
            if (b.x0 || b.y0) rc.h2d += (b.x0 ? 1 : 0) + (b.y0 ? 1 : 0), rc.launches += 4, rc.waits += 1;  // set_start
            rc.launches += 1, rc.d2h += 3, rc.waits += 1;                            // collect_solution (below)
        }
        GroupLaunches own_gl;  // (nobody in the group: the loop of run_many with tables of its own)
        GroupBlocks *gb = nj > 0 ? &blocks_of(s[0]) : nullptr;
        GroupLaunches &gl = gb ? gb->gl : own_gl;
        DropBlocksOnThrow drop{gb ? s[0] : nullptr};
        std::vector<PackMember> pm(static_cast<size_t>(count));
        for (int k : in) {
            pm[k].m = s[k]->m_loc, pm[k].n = s[k]->n_loc;
            pm[k].x0 = start[k].x0 != nullptr, pm[k].y0 = start[k].y0 != nullptr, pm[k].result = true;
        }
        const GroupPackLayout L = group_pack_layout(pm.data(), count);
        if (nj > 0) {
            // ---- the joiners' starts: pieces of the staging block after one copy
            std::vector<MemberStart> staged(static_cast<size_t>(count));
            if (L.start_doubles > 0) {
                double *host = static_cast<double *>(gb->in.stage(sizeof(double) * L.start_doubles));
                for (int k : in) group_pack_start(L, k, pm[k], start[k].x0, start[k].y0, host);
                gb->in.send(sizeof(double) * L.start_doubles, st);
                ++rc.h2d;
                const double *dev = static_cast<const double *>(gb->in.dev);  // (it outlives the start kernels: no wait between them and the loop)
                for (int k : in) {
                    const PackSlot &p = L.slot[k];
                    staged[k].x0 = p.x0 != kPackAbsent ? dev + p.x0 : nullptr, staged[k].y0 = p.y0 != kPackAbsent ? dev + p.y0 : nullptr;
                }
            }
            record_starts(s, in, start, staged.data(), gl, rc);
        }
        resolve_loop(s, count, out, gc, scope, joins, gl, grouped.data());
        rc.loop_own = gc.own;
        // ---- the solutions: a member's own collect_solution, the group's through one block, one copy and one wait
        for (int k = 0; k < count; ++k)
            if (!grouped[k]) s[k]->collect_solution(&out[k]);
        if (nj > 0) {
            if (gb->out_d.n < L.result_doubles) {
                gb->out_d.alloc(L.result_doubles);
                gb->out_h.alloc(L.result_doubles, false);
            }
            for (int k : in) {
                const PackSlot &p = L.slot[k];
                auto at = [&](size_t off) { return off == kPackAbsent ? nullptr : gb->out_d.p + off; };
                s[k]->solution_launch(at(p.x), at(p.y), at(p.z), &gl);
            }
            const long tables0 = gl.tables_sent();
            rc.launches += gl.run(st);
            rc.h2d += gl.tables_sent() - tables0;  // (the tables of what runs in front of the loop ride on the loop's first copy)
            HIP_CHECK(hipMemcpyAsync(gb->out_h.p, gb->out_d.p, sizeof(double) * L.result_doubles, hipMemcpyDeviceToHost, st));
            ++rc.d2h;
            HIP_CHECK(hipStreamSynchronize(st));
            ++rc.waits;
            for (int k : in) {
                Solver &m = *s[k];
                HPRLP_results *o = &out[k];
                o->x = static_cast<double *>(std::malloc(sizeof(double) * std::max(m.n_loc, 1)));
                o->y = static_cast<double *>(std::malloc(sizeof(double) * std::max(m.m_loc, 1)));
                o->z = static_cast<double *>(std::malloc(sizeof(double) * std::max(m.n_loc, 1)));
                if (!o->x || !o->y || !o->z) throw std::runtime_error("host allocation of the solution failed");
                group_unpack_result(L, k, pm[k], gb->out_h.p, o->x, o->y, o->z);
                ++rc.served;
            }
        }
        for (int k = 0; k < count; ++k)
            s[k]->set_transfer((start[k].x0 ? s[k]->n_loc : 0) + static_cast<size_t>(start[k].y0 ? s[k]->m_loc : 0),
                               2 * static_cast<size_t>(s[k]->n_loc) + s[k]->m_loc, false);
    }
    if (counts) *counts = rc;
}

// The members that go their own way run Solver::resolve_device from start to solution BEFORE the loop; only the joiners are
// looped, as a sub-list whose results are copied back, and their solutions are stored straight into the caller's buffers.
void resolve_many_device(Solver **s, int count, const MemberStart *start, const MemberOut *dst, hipStream_t caller, HPRLP_results *out,
                         ResolveCounts *counts, DeviceCounts *dcounts) {
    const char *who = "hprlp_solver_resolve_many_device";
    DeviceCounts unused;
    DeviceCounts &dc = dcounts ? *dcounts : unused;
    std::vector<MemberStart> cold;
    if (!start) {
        cold.resize(static_cast<size_t>(count));
        start = cold.data();
    }
    std::vector<MemberOut> none;
    if (!dst) {
        none.resize(static_cast<size_t>(count));
        dst = none.data();
    }
    bool warm = false;
    for (int k = 0; k < count; ++k) warm = warm || start[k].x0 || start[k].y0;
    PointerChecks pass(s[0]->prm.device_number, who, dc);
    for (int k = 0; k < count; ++k) {
        const size_t m = static_cast<size_t>(s[k]->m_loc), n = static_cast<size_t>(s[k]->n_loc);
        pass(k, start[k].x0, n, "x0"); pass(k, start[k].y0, m, "y0");
        pass(k, dst[k].x, n, "x"); pass(k, dst[k].y, m, "y"); pass(k, dst[k].z, n, "z");
    }
    ResolveCounts rc;
    GroupCounts gc;
    {
        GroupScope scope(s, count);
        const hipStream_t st = scope.group;
        std::vector<char> grouped;
        const std::vector<int> in = resolve_joiners(s, count, grouped);
        const int nj = static_cast<int>(in.size());
        GroupBlocks &gb = blocks_of(s[0]);
        GroupLaunches &gl = gb.gl;
        DropBlocksOnThrow drop{s[0]};
        wait_for_caller(gb, caller, st);  // (the outputs too: what the caller's stream still does with them comes first)
        if (warm) {
            // ---- the check: the starts of ALL members where they lie, one launch, one copy of the flag words, one wait
            const unsigned long long *flags = check_stage(gb, static_cast<size_t>(count), st, rc, &dc, [&](GroupLaunches &chk, unsigned long long *w) {
                for (int k = 0; k < count; ++k)
                    chk.data_check(DataCheckArgs{{start[k].x0, start[k].y0, nullptr, nullptr, nullptr}, {s[k]->n_loc, s[k]->m_loc, 0, 0, 0}, 1}, w + k);
            });
            for (int k = 0; k < count; ++k) throw_if_flagged(flags[k], kStartNames, member(who, k) + ": warm start", "is not finite");
        }
        // -- from here on the call goes through
        // ---- the members that go their own way: Solver::resolve_device, start to solution
        for (int k = 0; k < count; ++k) {
            if (grouped[k]) continue;
            const MemberStart &b = start[k];
            s[k]->resolve_device(b.sigma, b.x0, b.y0, caller, dst[k].x, dst[k].y, dst[k].z, &out[k]);
            ++rc.own, ++dc.own;
            // (nominal, many.h: ResolveCounts -- what Solver::resolve_device issues for a member without a locality ordering)
            rc.memsets += 17, rc.waits += 1;                                                         // reset_iterates
            rc.launches += (s[k]->hook_no_bound_codes ? 0 : 2) + 1 + (b.sigma > 0.0 ? 1 : 0);         // bound codes, ctrl, the override
            if (b.x0 || b.y0) rc.memsets += 1, rc.launches += 1 + 4, rc.d2h += 1, rc.waits += 2;    // the check, the start
            rc.launches += dst[k].x || dst[k].y || dst[k].z ? 1 : 0, rc.waits += 1;                  // the solution, the final wait
        }
        if (nj > 0) {
            record_starts(s, in, start, start, gl, rc);  // (the starts are read in the caller's buffers)
            // ---- the lock-step loop over the group's members
            std::vector<Solver *> js(static_cast<size_t>(nj));
            std::vector<HPRLP_results> jout(static_cast<size_t>(nj));
            for (int j = 0; j < nj; ++j) js[j] = s[in[j]], jout[j] = out[in[j]];
            const std::vector<char> all(static_cast<size_t>(nj), 1);
            resolve_loop(js.data(), nj, jout.data(), gc, scope, all, gl, all.data());
            rc.loop_own = gc.own;
            // ---- the solutions: straight into the callers' buffers (an output that is not wanted: the member's own scratch,
            // where its collect_solution puts it), one launch, one wait, no copy
            for (int j = 0; j < nj; ++j) {
                const int k = in[j];
                Solver &m = *s[k];
                out[k] = jout[j];
                out[k].x = out[k].y = out[k].z = nullptr;
                const MemberOut &o = dst[k];
                if (o.x || o.y || o.z) m.solution_launch(o.x ? o.x : m.sn1.p, o.y ? o.y : m.sm1.p, o.z ? o.z : m.gsn.p + m.col_off, &gl);
            }
            const long tables0 = gl.tables_sent();
            rc.launches += gl.run(st);
            rc.h2d += gl.tables_sent() - tables0;  // (the tables of what runs in front of the loop ride on the loop's first copy)
            HIP_CHECK(hipStreamSynchronize(st));
            ++rc.waits;
            for (int k : in) {
                s[k]->set_transfer(0, 0, true);
                ++rc.served, ++dc.served;
            }
        }
    }
    if (counts) *counts = rc;
}

// ------------------------------------------------------------------------------------------------
// set_matrix_values_many / set_matrix_values_many_device
// ------------------------------------------------------------------------------------------------
namespace {

// The apply for the members `in`: scatter, gather and zeroing in one stage, Solver::scale()'s pieces behind them, one recorder;
// then what Solver::values_apply and set_matrix_values leave, with the group call's wall times.  at[k]: where member k's values
// and vectors are read on the device -- pieces of the staging block, or the caller's own buffers; data[k]: nnz and the host
// pointer obj_constant.
void values_apply_group(Solver **s, const std::vector<int> &in, const MemberValues *data, const MemberValues *at, const std::vector<char> &built,
                        double maps_seconds, double upload_seconds, GroupBlocks &gb, hipStream_t st, ValuesCounts &vc, clock_type::time_point t0,
                        const Source &src) {
    const auto t_k = time_now();
    GroupLaunches &gl = gb.tables;
    const long tables0 = gl.tables_sent();
    for (int k : in) {
        Solver &m = *s[k];
        gl.values_in(data[k].nnz, at[k].val, m.map_A.p, m.map_AT.p, m.A.val.p, m.AT.val.p);
        gl.vectors_in(VectorsInArgs{m.m_loc, m.n_loc, at[k].AL, at[k].AU, at[k].l, at[k].u, at[k].c, m.perm_r_dev.p, m.perm_c_dev.p, m.AL.p,
                                    m.AU.p, m.l.p, m.u.p, m.c.p});
        if (data[k].obj_constant) m.obj_constant = *data[k].obj_constant;
        m.reset_iterates(&gl);
    }
    gl.next_stage();  // (the scaling reads what the three kinds of this stage write)
    const double kernels_seconds = time_since(t_k);
    SetupCounts sc;
    scale_walk(s, in, gl, st, sc);
    vc.launches += sc.scale_launches;
    vc.waits += sc.scale_waits;
    vc.d2h += sc.scale_waits;  // (the sums block comes back once per wait)
    vc.h2d += gl.tables_sent() - tables0;
    vc.served += sc.served;
    const double wall = time_since(t0);
    for (int k : in) {
        Solver &m = *s[k];
        m.matrix_time[0] = built[k] ? maps_seconds : 0.0;
        m.matrix_time[1] = upload_seconds;
        m.matrix_time[2] = kernels_seconds;
        m.matrix_time[3] = m.scaling_time;
        m.matrix_time[4] = wall;
        ++m.matrix_calls;
        m.data_since_run += wall;
        // (the words that travelled: none for a device entry, values and vectors for a host entry)
        if (src.device()) m.set_transfer(0, 0, true);
        else m.set_transfer(static_cast<size_t>(data[k].nnz) + 2 * static_cast<size_t>(m.m) + 3 * static_cast<size_t>(m.n), 0, false);
    }
}

void set_matrix_values_group(Solver **s, int count, const MemberValues *data, const Source &src, ValuesCounts *counts) {
    const char *who = src.who;
    // ---- the host rules of all members, before the first upload (Solver::set_matrix_values' rules and messages)
    std::vector<char> gave(static_cast<size_t>(count), 0);
    int ngave = 0;
    for (int k = 0; k < count; ++k) {
        const MemberValues &d = data[k];
        if (!(d.val || d.c || d.obj_constant || d.AL || d.AU || d.l || d.u)) continue;  // skipped: the member keeps every bit
        if (!d.val || !d.c || !d.AL || !d.AU || !d.l || !d.u)
            throw std::runtime_error(member(who, k) + ": val, c, AL, AU, l and u are all required (every scaled vector depends on the values)");
        if (d.nnz != static_cast<long>(s[k]->A.view.nnz))
            throw std::runtime_error(member(who, k) + ": nnz is " + std::to_string(d.nnz) + ", the model has " + std::to_string(s[k]->A.view.nnz) +
                                     " entries (the pattern cannot change)");
        if (!src.device()) host_no_nan(who, k, *s[k], d.c, d.AL, d.AU, d.l, d.u);  // (host memory only)
        if (d.obj_constant && std::isnan(*d.obj_constant)) throw std::runtime_error(member(who, k) + ": obj_constant is NaN");
        gave[k] = 1;
        ++ngave;
    }
    double ptr_seconds = 0.0;
    if (src.device()) {  // every pointer of every member that gave: still nothing launched or written
        const auto t_ptr = time_now();
        PointerChecks pass(s[0]->prm.device_number, who, *src.dc);
        for (int k = 0; k < count; ++k) {
            if (!gave[k]) continue;
            const MemberValues &d = data[k];
            pass(k, d.val, static_cast<size_t>(d.nnz), "val");
            pass.data_vectors(k, static_cast<size_t>(s[k]->m), static_cast<size_t>(s[k]->n), d.c, d.AL, d.AU, d.l, d.u);
        }
        ptr_seconds = time_since(t_ptr);
    }
    ValuesCounts vc;
    const auto t0 = time_now();
    GroupScope scope(s, count);
    const hipStream_t st = scope.group;
    const bool fused_norms = env_get("HPRLP_NO_FUSED_NORMS") == nullptr;  // (scale_many's condition)
    std::vector<char> wanted(static_cast<size_t>(count)), joins;
    for (int k = 0; k < count; ++k) wanted[k] = gave[k] && fused_norms && s[k]->joins_group_resolve() && s[k]->m_loc > 0 && s[k]->n_loc > 0;
    const std::vector<int> in = joiners(wanted, joins);
    // The scatter of a joining member (no value map for A) loads the values as 16-byte pairs.  A host entry's come from the staging
    // block, where every vector starts on a multiple of kPackAlign = 32 doubles of a pinned block's copy; a device entry's come from
    // the caller's buffer: an 8-byte aligned `val` is the single entries' rule, the pairs need 16.  (The stores go to A_val + 2 t and
    // AT_val + 2 t: hipMalloc's, or pieces of the group's arena, 256-byte aligned both.)
    if (src.device())
        for (int k : in)
            if (reinterpret_cast<uintptr_t>(data[k].val) % 16)
                throw std::runtime_error(member(who, k) + ": val is not aligned to 16 bytes (the group's scatter loads the values in pairs)");
    // One member alone is checked by its own call before it writes anything, and nobody else is written: no block.
    GroupBlocks *gb = ngave >= 2 ? &blocks_of(s[0]) : nullptr;
    DropBlocksOnThrow drop{gb ? s[0] : nullptr};
    // ---- value maps: a member's own construction, once (joining members have no ordering: map_A stays null, map_AT comes from
    // the host transpose); the members on their own way build theirs inside their own call
    const auto t_maps = time_now();
    std::vector<char> built(static_cast<size_t>(count), 0);
    for (int k : in) {
        if (s[k]->have_maps) continue;
        s[k]->build_value_maps();
        built[k] = 1;
        ++vc.maps;
    }
    const double maps_seconds = time_since(t_maps);
    const auto t_up = time_now();
    std::vector<MemberValues> staged;  // a host entry: where the joiners' values and vectors lie in the staging block
    if (gb) {
        const size_t K = static_cast<size_t>(count);
        const double *dev = nullptr;
        GroupPackLayout L;
        if (src.device()) {
            wait_for_caller(*gb, src.caller, st);
        } else {
            // ---- a host entry's staging: [val | AL | AU | l | u | c] of the joining members and the values of the others in ONE
            // pinned block, one copy
            std::vector<PackMember> pm(K);
            for (int k = 0; k < count; ++k) {
                if (!gave[k]) continue;
                pm[k].m = s[k]->m_loc, pm[k].n = s[k]->n_loc, pm[k].nnz = data[k].nnz;
                pm[k].c = pm[k].bounds = joins[k] != 0;
            }
            L = group_pack_layout(pm.data(), count);
            double *host = static_cast<double *>(gb->in.stage(sizeof(double) * std::max<size_t>(L.data_doubles, 1)));
            for (int k = 0; k < count; ++k) {
                if (!gave[k]) continue;
                group_pack_values(L, k, pm[k], data[k].val, host);
                group_pack_data(L, k, pm[k], data[k].AL, data[k].AU, data[k].l, data[k].u, data[k].c, host);
            }
            if (L.data_doubles > 0) {
                gb->in.send(sizeof(double) * L.data_doubles, st);
                ++vc.h2d;
            }
            dev = static_cast<const double *>(gb->in.dev);
            auto at = [&](size_t off) { return off == kPackAbsent ? nullptr : dev + off; };
            staged.resize(K);
            for (int k : in) {
                const PackSlot &p = L.slot[k];
                staged[k].val = at(p.val), staged[k].c = at(p.c), staged[k].AL = at(p.AL), staged[k].AU = at(p.AU), staged[k].l = at(p.l),
                staged[k].u = at(p.u);
            }
        }
        // ---- the check, in ONE stage: everybody's values (a host entry: in the staging block) into one flag word per member, all
        // bits set: clean; a device entry's vectors too, where they lie, into a second word per member (the vectors' at k, the
        // values' at count + k).  One memset, one copy, one wait.
        const size_t val_at = src.device() ? K : 0;
        const unsigned long long *flags = check_stage(*gb, val_at + K, st, vc, src.dc, [&](GroupLaunches &chk, unsigned long long *w) {
            for (int k = 0; k < count; ++k) {
                if (!gave[k]) continue;
                const MemberValues &d = data[k];
                if (src.device()) {
                    chk.data_check(nan_check(s[k]->m, s[k]->n, d.c, d.AL, d.AU, d.l, d.u), w + k);
                    chk.values_check(d.val, d.nnz, w + val_at + k);
                } else if (L.slot[k].val != kPackAbsent) {
                    chk.values_check(dev + L.slot[k].val, d.nnz, w + k);
                }
            }
        });
        // (a vector's NaN of any member wins: a host entry's host checks of the vectors have come first)
        if (src.device())
            for (int k = 0; k < count; ++k)
                if (gave[k]) throw_if_flagged(flags[k], kDataNames, member(who, k), "is NaN");
        for (int k = 0; k < count; ++k)  // (the lowest member, its smallest position)
            if (gave[k] && flags[val_at + k] != kValuesAllFinite)
                throw std::runtime_error(member(who, k) + ": val[" + std::to_string(flags[val_at + k]) + "] is not finite");
    }
    const double upload_seconds = ptr_seconds + time_since(t_up);  // (a device entry's lookups count as its upload)
    // -- from here on the call goes through
    // ---- the members that go their own way: the single entry of the source's kind (its own upload and checks included)
    for (int k = 0; k < count; ++k) {
        if (!gave[k] || joins[k]) continue;
        Solver &m = *s[k];
        const MemberValues &d = data[k];
        const bool had_maps = m.have_maps;
        const long f0 = m.fetches, l0 = scaling_launch_count();
        try {
            if (src.device()) m.set_matrix_values_device(d.val, d.nnz, d.c, d.obj_constant, d.AL, d.AU, d.l, d.u, src.caller);
            else m.set_matrix_values(d.val, d.nnz, d.c, d.obj_constant, d.AL, d.AU, d.l, d.u);
        } catch (const std::exception &e) {  // (a member alone in the call: its own check's refusal, named as the group's)
            std::string msg = e.what();
            for (const char *own : {"set_matrix_values: ", "set_matrix_values_device: "})
                if (msg.compare(0, std::strlen(own), own) == 0) msg = msg.substr(std::strlen(own));
            throw std::runtime_error(member(who, k) + ": " + msg);
        }
        ++vc.own;
        if (!had_maps) ++vc.maps;
        vc.memsets += 1 + 17;
        vc.d2h += 1 + (m.fetches - f0);
        if (src.device()) {
            ++src.dc->own;
            // the flags' memset, the two checks, scatter, gather, the flags' copy and wait; reset_iterates' seventeen memsets and
            // wait; scale(): its launches, its scalar fetches, its final wait; the wait that ends the call
            vc.launches += 4 + (scaling_launch_count() - l0);
            vc.waits += 1 + 1 + (m.fetches - f0) + 1 + 1;
        } else {
            // its staging in one copy (six from the allocator cache's block size on), the flag's memset, check, scatter, gather, the
            // flag's copy and wait; reset_iterates' seventeen memsets and wait; scale(): its launches, its scalar fetches, its final wait
            const size_t words = static_cast<size_t>(d.nnz) + 2 * static_cast<size_t>(m.m) + 3 * static_cast<size_t>(m.n);
            vc.h2d += words * sizeof(double) < kDeviceCacheMinBytes ? 1 : 6;
            vc.launches += 3 + (scaling_launch_count() - l0);
            vc.waits += 1 + 1 + (m.fetches - f0) + 1;
        }
    }
    if (!in.empty()) {
        values_apply_group(s, in, data, src.device() ? data : staged.data(), built, maps_seconds, upload_seconds, *gb, st, vc, t0, src);
        if (src.device()) src.dc->served += static_cast<long>(in.size());
    }
    if (counts) *counts = vc;
}

}  // namespace

void set_matrix_values_many(Solver **s, int count, const MemberValues *data, ValuesCounts *counts) {
    set_matrix_values_group(s, count, data, Source{"hprlp_solver_set_matrix_values_many"}, counts);
}
void set_matrix_values_many_device(Solver **s, int count, const MemberValues *data, hipStream_t caller, ValuesCounts *counts,
                                   DeviceCounts *dcounts) {
    DeviceCounts unused;
    set_matrix_values_group(s, count, data, Source{"hprlp_solver_set_matrix_values_many_device", caller, dcounts ? dcounts : &unused}, counts);
}

}  // namespace hprlp

