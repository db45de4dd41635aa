// abi_many.cpp -- extern "C" boundary, many small LPs at once (many.cpp; DESIGN.md "Many small LPs"): the checks of a group
// call's list and members, every *_many entry, hprlp_solve_many / _detect / _wide, the wide members and the accessors of the
// count blocks.  Each entry zeroes its count blocks where it always did: the accessors show it, and tests read them.
#include <cstdlib>
#include <iostream>

#include "abi_common.h"
#include "env.h"
#include "many.h"

using namespace hprlp;

// the members of a group call, checked before anything is launched (`who`, for the error messages)
static std::vector<Solver *> group_members(hprlp_solver **h, int count, const char *who, bool need_scaled = true) {
    const std::string w(who);
    if (!h) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    std::vector<Solver *> s(static_cast<size_t>(count));
    for (int k = 0; k < count; ++k) {
        if (!h[k]) throw std::runtime_error(w + ": member " + std::to_string(k) + " is null");
        if (h[k]->sharded)
            throw std::runtime_error(w + ": member " + std::to_string(k) + " is a sharded solver (hprlp_solver_create_dist* / _local*); a group runs on one GPU");
        s[k] = &h[k]->s;
    }
    check_group(s.data(), count, who, need_scaled);
    return s;
}
// the refusals of a group entry's plain arguments, in their order: the list, the count, then `arg` (data or results, `what` in the
// message); group_members comes next
static void check_group_args(hprlp_solver **h, int count, const void *arg, const char *what, const char *who) {
    const std::string w(who);
    if (!h) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    if (!arg) throw std::runtime_error(w + ": null " + what);
}

// the public member structs as many.h's
static MemberData to_private(const hprlp_member_data &d) {
    MemberData r;
    r.c = d.c, r.obj_constant = d.obj_constant, r.AL = d.AL, r.AU = d.AU, r.l = d.l, r.u = d.u;
    return r;
}
static MemberValues to_private(const hprlp_member_values &d) {
    MemberValues r;
    r.val = d.val, r.nnz = d.nnz, r.c = d.c, r.obj_constant = d.obj_constant, r.AL = d.AL, r.AU = d.AU, r.l = d.l, r.u = d.u;
    return r;
}
static MemberStart to_private(const hprlp_member_start &b) {
    MemberStart r;
    r.x0 = b.x0, r.y0 = b.y0, r.sigma = b.sigma;
    return r;
}
static MemberOut to_private(const hprlp_member_out &o) {
    MemberOut r;
    r.x = o.x, r.y = o.y, r.z = o.z;
    return r;
}
// one private struct per member; a null list: every member's default (a cold start, no output wanted)
template <class Private, class Public>
static std::vector<Private> private_members(const Public *list, int count) {
    std::vector<Private> v(static_cast<size_t>(count));
    for (int k = 0; list && k < count; ++k) v[k] = to_private(list[k]);
    return v;
}

// The count blocks of the group calls: eight slots each, the calling thread's own, filled by keep_counts and read by the
// hprlp_last_*_counts accessors.  Which call zeroes which block, and when, is the call's own business (tests read it).

// ---- group set-up, scaling and teardown (DESIGN.md "Many small LPs", group set-up) -------------------------------------------
// counts of the calling thread's last hprlp_solver_create_many / _scale_many / _destroy_many; each call zeroes and fills its own
static thread_local long g_setup_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_setup_many_counts(long out[8]) { return read_counts(g_setup_counts, out); }

// hprlp_solver_create for every model.  together: the members whose set-up only allocates, zeroes and uploads
// (Solver::group_setup_fits) are created inside one arena -- a few device blocks, one pinned block, one stream, one copy per
// block and one wait for all of them; every other member, and everybody when !together, is set up as hprlp_solver_create does.
// A model that fails leaves out[k] = NULL and its message in hprlp_last_error(); the others are created.  Returns the number
// created.
static int create_group(const LP_info_cpu *const *models, int count, const HPRLP_parameters *p, hprlp_solver **out, const char *who, bool together) {
    for (int k = 0; k < count; ++k) out[k] = nullptr;
    const AllocCounts before = alloc_counts();
    Arena *arena = nullptr;
    if (together) {
        try {
            arena = arena_create(p->device_number);
        } catch (const std::exception &) {
            // (no device, a wrong device number: every member says so itself below, as in a set-up member by member)
        }
    }
    struct CreatorsReference {  // (the members hold their own: the arena goes with the last of them, or here if nobody joined it)
        Arena *a;
        ~CreatorsReference() { arena_release(a); }
    } creators{arena};
    int made = 0;
    try {
        for (int k = 0; k < count; ++k) {
            hprlp_solver *h = nullptr;
            try {
                if (!models[k]) throw std::runtime_error("null model");
                h = new hprlp_solver();
                h->s.verbose = false;
                if (arena && Solver::group_setup_fits(models[k])) {
                    ArenaScope scope(arena);
                    h->s.setup(models[k], p);
                } else {
                    h->s.setup(models[k], p);
                }
                out[k] = h;
                ++made;
            } catch (const std::exception &e) {  // (one member's failure is not the call's: the others go on)
                set_last_error(std::string(who) + ": model " + std::to_string(k) + ": " + e.what());
                std::cerr << "[error] " << who << ": model " << k << " failed its set-up: " << e.what() << std::endl;
                delete h;
            }
        }
        if (arena) arena_flush(arena);
        if (made > 0) HIP_CHECK(hipDeviceSynchronize());
    } catch (...) {
        for (int k = 0; k < count; ++k) {
            delete out[k];
            out[k] = nullptr;
        }
        throw;
    }
    const AllocCounts after = alloc_counts();
    g_setup_counts[0] = after.device_allocs - before.device_allocs;
    g_setup_counts[1] = after.pinned_allocs - before.pinned_allocs;
    g_setup_counts[2] = after.h2d_copies - before.h2d_copies;
    return made;
}

static void destroy_group(hprlp_solver **h, int count) {
    const long before = alloc_counts().device_frees;
    for (int k = 0; k < count; ++k) {
        try {
            destroy_handle(h[k]);
        } catch (...) {
        }
        h[k] = nullptr;
    }
    g_setup_counts[7] = alloc_counts().device_frees - before;
}

static void keep_scale_counts(const SetupCounts &sc) {
    g_setup_counts[3] = sc.scale_launches;
    g_setup_counts[4] = sc.scale_waits;
    g_setup_counts[5] = sc.served;
    g_setup_counts[6] = sc.own;
}

extern "C" int hprlp_solver_create_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, hprlp_solver **out) {
    return guarded(-1, [&] {
        for (int i = 0; i < 3; ++i) g_setup_counts[i] = 0;
        if (!models) throw std::runtime_error("hprlp_solver_create_many: null model list");
        if (count <= 0) throw std::runtime_error("hprlp_solver_create_many: count must be positive");
        if (!out) throw std::runtime_error("hprlp_solver_create_many: null handle list");
        HPRLP_parameters dflt;
        return create_group(models, count, param ? param : &dflt, out, "hprlp_solver_create_many", true);
    });
}

extern "C" int hprlp_solver_scale_many(hprlp_solver **h, int count) {
    return guarded(-1, [&] {
        keep_scale_counts(SetupCounts());
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_scale_many", false);
        SetupCounts sc;
        scale_many(s.data(), count, &sc);
        keep_scale_counts(sc);
        return 0;
    });
}

extern "C" void hprlp_solver_destroy_many(hprlp_solver **h, int count) {
    g_setup_counts[7] = 0;
    if (!h || count <= 0) return;
    destroy_group(h, count);
}

extern "C" int hprlp_solver_power_iteration_many(hprlp_solver **h, int count, int max_iter, double tol, double *lambda_out, int *iters_out) {
    return guarded(-1, [&] {
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_power_iteration_many");
        if (!lambda_out) throw std::runtime_error("hprlp_solver_power_iteration_many: null lambda_out");
        power_iteration_many(s.data(), count, max_iter, tol, lambda_out, iters_out);
        return 0;
    });
}

extern "C" int hprlp_solver_iterate_many(hprlp_solver **h, int count, const int *normal, int then_check) {
    return guarded(-1, [&] {
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_iterate_many");
        iterate_many(s.data(), count, normal, then_check != 0);
        return 0;
    });
}

extern "C" int hprlp_solver_residuals_many(hprlp_solver **h, int count, const int *iter, const int *compute_gap, double *out) {
    return guarded(-1, [&] {
        // (the plain arguments first, so that a wrong call is refused whatever the handles are)
        if (!iter) throw std::runtime_error("hprlp_solver_residuals_many: null iter");
        if (!compute_gap) throw std::runtime_error("hprlp_solver_residuals_many: null compute_gap");
        if (!out) throw std::runtime_error("hprlp_solver_residuals_many: null out");
        for (int k = 0; k < count; ++k)
            if (iter[k] < 0) throw std::runtime_error("hprlp_solver_residuals_many: iter[" + std::to_string(k) + "] is negative");
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_residuals_many");
        residuals_many(s.data(), count, iter, compute_gap, out);
        return 0;
    });
}

extern "C" int hprlp_solver_restart_many(hprlp_solver **h, int count, const double *in, double *sigma_out) {
    return guarded(-1, [&] {
        if (!in) throw std::runtime_error("hprlp_solver_restart_many: null in");
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_restart_many");
        restart_many(s.data(), count, in, sigma_out);
        return 0;
    });
}

// hprlp_solver_ray_step for every member of a group (many.cpp: ray_step_many)
extern "C" int hprlp_solver_ray_step_many(hprlp_solver **h, int count, const int *restart, double *out, int *tested) {
    return guarded(-1, [&] {
        // (the plain arguments first, so that a wrong call is refused whatever the handles are)
        if (!restart) throw std::runtime_error("hprlp_solver_ray_step_many: null restart");
        if (!out) throw std::runtime_error("hprlp_solver_ray_step_many: null out");
        if (!tested) throw std::runtime_error("hprlp_solver_ray_step_many: null tested");
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_ray_step_many");
        ray_step_many(s.data(), count, restart, out, tested);
        return 0;
    });
}

// counts of the calling thread's last hprlp_solver_run_many / hprlp_solve_many (hprlp_last_run_many_counts)
static thread_local long g_many_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static void keep_many_counts(const GroupCounts &gc) {
    keep_counts(g_many_counts, {gc.rounds, gc.waits, gc.group_launches, gc.copies, gc.own, gc.served, gc.ray_served, gc.certs_served});
}

extern "C" int hprlp_last_run_many_counts(long out[8]) { return read_counts(g_many_counts, out); }

static void free_results_arrays(HPRLP_results *out, int count) {
    for (int k = 0; k < count; ++k) {
        std::free(out[k].x); std::free(out[k].y); std::free(out[k].z);
        out[k].x = out[k].y = out[k].z = nullptr;
    }
}

extern "C" int hprlp_solver_run_many(hprlp_solver **h, int count, HPRLP_results *out) {
    return guarded(-1, [&] {
        std::vector<Solver *> s = group_members(h, count, "hprlp_solver_run_many");
        if (!out) throw std::runtime_error("hprlp_solver_run_many: null results");
        for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
        keep_many_counts(GroupCounts());
        try {
            GroupCounts gc;
            run_many(s.data(), count, out, &gc);
            keep_many_counts(gc);
        } catch (...) {
            free_results_arrays(out, count);
            throw;
        }
        return 0;
    });
}

// ---- group re-solve, group matrix values, group device re-solve (DESIGN.md "Many small LPs") ------------------------------------
// counts of the calling thread's last hprlp_solver_set_data_many / _resolve_many (hprlp_last_resolve_many_counts) and
// hprlp_solver_set_matrix_values_many (hprlp_last_values_many_counts); the device entries put theirs in the same blocks, and what
// only a device call has in g_device_counts (hprlp_last_many_device_counts), which many.cpp fills as the call proceeds
static thread_local long g_resolve_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static thread_local long g_values_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static thread_local DeviceCounts g_device_counts;
static void keep_resolve_counts(const ResolveCounts &rc) {
    keep_counts(g_resolve_counts, {rc.h2d, rc.d2h, rc.waits, rc.launches, rc.memsets, rc.served, rc.own, rc.loop_own});
}
static void keep_values_counts(const ValuesCounts &vc) {
    keep_counts(g_values_counts, {vc.h2d, vc.d2h, vc.waits, vc.launches, vc.memsets, vc.served, vc.own, vc.maps});
}

extern "C" int hprlp_last_resolve_many_counts(long out[8]) { return read_counts(g_resolve_counts, out); }
extern "C" int hprlp_last_values_many_counts(long out[8]) { return read_counts(g_values_counts, out); }
extern "C" int hprlp_last_many_device_counts(long out[8]) {
    const DeviceCounts &d = g_device_counts;
    const long v[8] = {d.pointers, d.lookups, d.check_launches, d.flags, d.served, d.own, d.waits_before_write, 0};
    return read_counts(v, out);
}

extern "C" int hprlp_solver_set_data_many(hprlp_solver **h, int count, const hprlp_member_data *data) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_data_many";
        check_group_args(h, count, data, "data", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberData> d = private_members<MemberData>(data, count);
        keep_resolve_counts(ResolveCounts());
        ResolveCounts rc;
        set_data_many(s.data(), count, d.data(), &rc);
        keep_resolve_counts(rc);
        return 0;
    });
}

extern "C" int hprlp_solver_resolve_many(hprlp_solver **h, int count, const hprlp_member_start *start, HPRLP_results *out) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_resolve_many";
        check_group_args(h, count, out, "results", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberStart> b = private_members<MemberStart>(start, count);
        check_starts(s.data(), count, b.data(), who, true);  // (before the results are touched: a refusal leaves the output arrays as they were)
        for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
        keep_resolve_counts(ResolveCounts());
        try {
            ResolveCounts rc;
            resolve_many(s.data(), count, b.data(), out, &rc);
            keep_resolve_counts(rc);
        } catch (...) {
            free_results_arrays(out, count);
            throw;
        }
        return 0;
    });
}

extern "C" int hprlp_solver_set_matrix_values_many(hprlp_solver **h, int count, const hprlp_member_values *data) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_matrix_values_many";
        keep_values_counts(ValuesCounts());
        check_group_args(h, count, data, "data", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberValues> d = private_members<MemberValues>(data, count);
        ValuesCounts vc;
        set_matrix_values_many(s.data(), count, d.data(), &vc);
        keep_values_counts(vc);
        return 0;
    });
}

extern "C" int hprlp_solver_set_data_many_device(hprlp_solver **h, int count, const hprlp_member_data *data, void *stream) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_data_many_device";
        g_device_counts = DeviceCounts();
        keep_resolve_counts(ResolveCounts());
        check_group_args(h, count, data, "data", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberData> d = private_members<MemberData>(data, count);
        ResolveCounts rc;
        set_data_many_device(s.data(), count, d.data(), static_cast<hipStream_t>(stream), &rc, &g_device_counts);
        keep_resolve_counts(rc);
        return 0;
    });
}

extern "C" int hprlp_solver_resolve_many_device(hprlp_solver **h, int count, const hprlp_member_start *start, const hprlp_member_out *dst,
                                                void *stream, HPRLP_results *out) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_resolve_many_device";
        g_device_counts = DeviceCounts();
        keep_resolve_counts(ResolveCounts());
        check_group_args(h, count, out, "results", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberStart> b = private_members<MemberStart>(start, count);
        const std::vector<MemberOut> o = private_members<MemberOut>(dst, count);
        check_starts(s.data(), count, b.data(), who, false);  // (the starts' entries are the device check's)
        // (a refusal leaves the output array as it was: the results are touched once the call goes through)
        std::vector<HPRLP_results> res(static_cast<size_t>(count), make_error_result("ERROR"));
        ResolveCounts rc;
        resolve_many_device(s.data(), count, b.data(), o.data(), static_cast<hipStream_t>(stream), res.data(), &rc, &g_device_counts);
        keep_resolve_counts(rc);
        for (int k = 0; k < count; ++k) out[k] = res[k];  // (x, y, z are NULL: nothing for hprlp_free_results to free)
        return 0;
    });
}

extern "C" int hprlp_solver_set_matrix_values_many_device(hprlp_solver **h, int count, const hprlp_member_values *data, void *stream) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_matrix_values_many_device";
        g_device_counts = DeviceCounts();
        keep_values_counts(ValuesCounts());
        check_group_args(h, count, data, "data", who);
        std::vector<Solver *> s = group_members(h, count, who);
        const std::vector<MemberValues> d = private_members<MemberValues>(data, count);
        ValuesCounts vc;
        set_matrix_values_many_device(s.data(), count, d.data(), static_cast<hipStream_t>(stream), &vc, &g_device_counts);
        keep_values_counts(vc);
        return 0;
    });
}

// phases of the calling thread's last hprlp_solve_many (hprlp_last_solve_many_phases)
static thread_local double g_many_phases[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_solve_many_phases(double out[8]) { return read_counts(g_many_phases, out); }

// hprlp_solve_many, hprlp_solve_many_detect and hprlp_solve_many_wide (`who`, for the error messages; wide: every member is marked
// wide before the group's scaling).  det null: no detection.  certs (may be null):
// count entries, each cleared to its member's m and n on entry (hprlp_solve_detect's contract) and filled where detection ran.
static int solve_many_entry(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                            HPRLP_results *out, hprlp_certificate *certs, const char *who_, bool wide = false) {
    return guarded(-1, [&] {
        const std::string w(who_);
        if (!models) throw std::runtime_error(w + ": null model list");
        if (count <= 0) throw std::runtime_error(w + ": count must be positive");
        if (!out) throw std::runtime_error(w + ": null results");
        for (int k = 0; k < count; ++k)
            if (!models[k]) throw std::runtime_error(w + ": model " + std::to_string(k) + " is null");
        Detection dsel;
        bool with_det = false;
        try {
            with_det = detection_from(det, &dsel);  // (a negative eps: refused before anything is created)
        } catch (const std::exception &e) {  // (the same refusal under the entry's name)
            throw std::runtime_error(w + ": " + e.what());
        }
        if (certs)
            for (int k = 0; k < count; ++k) clear_certificate(&certs[k], models[k]->m, models[k]->n);
        HPRLP_parameters dflt;
        const HPRLP_parameters *p = param ? param : &dflt;
        const auto t_call = time_now();
        for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
        for (int i = 0; i < 8; ++i) g_many_phases[i] = 0.0;
        keep_many_counts(GroupCounts());
        for (int i = 0; i < 8; ++i) g_setup_counts[i] = 0;
        // set-up and scaling of the whole group (create_group, scale_many); a model that fails its set-up stays "ERROR" and the others
        // go on.  HPRLP_NO_GROUP_SETUP=1 (test hook, A/B runs): member by member, as hprlp_solver_create + hprlp_solver_scale.
        const char *ngs = env_get("HPRLP_NO_GROUP_SETUP");
        const bool together = !(ngs && ngs[0] == '1');
        std::vector<hprlp_solver *> owned(static_cast<size_t>(count), nullptr);
        struct Teardown {  // (the members' device state goes when the call ends, however it ends)
            std::vector<hprlp_solver *> &h;
            ~Teardown() {
                for (hprlp_solver *m : h)
                    if (m) {
                        destroy_group(h.data(), static_cast<int>(h.size()));
                        return;
                    }
            }
        } teardown{owned};
        std::vector<Solver *> s;
        std::vector<int> who;
        const auto t_setup = time_now();
        create_group(models, count, p, owned.data(), who_, together);
        g_many_phases[0] = time_since(t_setup);
        for (int k = 0; k < count; ++k)
            if (owned[k]) {
                owned[k]->s.group_wide = wide;  // (hprlp_solve_many_wide: every member asks for the group launches)
                s.push_back(&owned[k]->s);
                who.push_back(k);
            }
        const int ng = static_cast<int>(s.size());
        if (ng > 0) {
            const auto t_scale = time_now();
            SetupCounts sc;
            if (together) {
                scale_many(s.data(), ng, &sc);
            } else {
                const long l0 = scaling_launch_count();
                for (int g = 0; g < ng; ++g) {
                    const long f0 = s[g]->fetches;
                    s[g]->scale();
                    sc.scale_waits += s[g]->fetches - f0 + 1;
                    ++sc.own;
                }
                sc.scale_launches = scaling_launch_count() - l0;
            }
            keep_scale_counts(sc);
            g_many_phases[1] = time_since(t_scale);
            std::vector<HPRLP_results> res(static_cast<size_t>(ng));
            for (auto &r : res) r = make_error_result("ERROR");
            try {
                const auto t_pw = time_now();
                std::vector<double> lam(static_cast<size_t>(ng));
                power_iteration_many(s.data(), ng, 5000, 1e-4, lam.data(), nullptr);  // src/HPRLP.cu:81-97
                for (int g = 0; g < ng; ++g) {
                    s[g]->lambda_max = lam[g] * 1.01;
                    s[g]->init_iteration_state();
                    if (with_det) s[g]->detect = dsel;
                }
                g_many_phases[2] = time_since(t_pw);
                const WideCounts pw = last_wide_counts();
                const auto t_loop = time_now();
                GroupCounts gc;
                run_many(s.data(), ng, res.data(), &gc);
                if (wide) last_wide_counts().power_launches = pw.power_launches, last_wide_counts().power_waits = pw.power_waits;
                g_many_phases[3] = time_since(t_loop);  // (the loop and the solutions' way back)
                g_many_phases[5] = static_cast<double>(gc.rounds);
                g_many_phases[6] = static_cast<double>(gc.waits);
                g_many_phases[7] = static_cast<double>(gc.launches);
                keep_many_counts(gc);
                if (with_det && certs)
                    for (int g = 0; g < ng; ++g)
                        if (!export_certificate(s[g]->cert, &certs[who[g]], models[who[g]]->m, models[who[g]]->n)) {
                            for (int k = 0; k < count; ++k) hprlp_free_certificate(&certs[k]);
                            throw std::runtime_error(w + ": host allocation of a certificate failed");
                        }
            } catch (...) {
                free_results_arrays(res.data(), ng);
                throw;
            }
            for (int g = 0; g < ng; ++g) out[who[g]] = res[g];
        }
        destroy_group(owned.data(), count);  // (the members' device state goes here: part of the call's wall time)
        g_many_phases[4] = time_since(t_call);
        return 0;
    });
}

extern "C" int hprlp_solve_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, HPRLP_results *out) {
    return solve_many_entry(models, count, param, nullptr, out, nullptr, "hprlp_solve_many");
}

extern "C" int hprlp_solve_many_detect(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                                       HPRLP_results *out, hprlp_certificate *certs) {
    return solve_many_entry(models, count, param, det, out, certs, "hprlp_solve_many_detect");
}

// ---- wide members (many.cpp; DESIGN.md "Many small LPs", wide members) -------------------------------------------------------
extern "C" int hprlp_solver_set_group_wide(hprlp_solver *h, int on) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_group_wide";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "a sharded solver (hprlp_solver_create_dist* / _local*) joins no group; a group runs on one GPU", nullptr);
        s.group_wide = on != 0;
        if (s.use_small && !s.comm) return 1;  // (it joins anyway)
        return on != 0 && s.joins_group() ? 1 : 0;
    });
}

extern "C" int hprlp_solve_many_wide(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                                     HPRLP_results *out, hprlp_certificate *certs) {
    return solve_many_entry(models, count, param, det, out, certs, "hprlp_solve_many_wide", true);
}

extern "C" int hprlp_last_many_wide_counts(long out[8]) {
    const WideCounts &wc = last_wide_counts();
    const long v[8] = {wc.joined, wc.refused, wc.normal_launches, wc.segments, wc.member_iterations, wc.power_launches, wc.power_waits, 0};
    return read_counts(v, out);
}
