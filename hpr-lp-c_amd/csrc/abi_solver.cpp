// abi_solver.cpp -- extern "C" boundary, the step-level extension on one hprlp_solver handle (include/hprlp_amd.h): create and
// destroy, the sharded and local constructors with their transport, the steps of a solve, vectors, scalars and facts by name,
// detection, warm start, re-solve and matrix values with their device twins.  Group calls (*_many) are in abi_many.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "abi_common.h"

using namespace hprlp;

extern "C" hprlp_solver *hprlp_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param) {
    if (!model) {
        set_last_error("null model");
        return nullptr;
    }
    hprlp_solver *h = nullptr;
    hprlp_solver *made = guarded(static_cast<hprlp_solver *>(nullptr), [&] {
        HPRLP_parameters dflt;
        h = new hprlp_solver();
        h->s.verbose = false;
        h->s.setup(model, param ? param : &dflt);
        return h;
    });
    if (!made) delete h;
    return made;
}

void hprlp::destroy_handle(hprlp_solver *h) {
    if (!h) return;
    Comm *c = h->comm, *x = h->xcomm;
    delete h;  // the solver first: its device state (and a background tiling job) goes before the transport
    delete x;
    delete c;
}

extern "C" void hprlp_solver_destroy(hprlp_solver *h) {
    try {
        destroy_handle(h);
    } catch (...) {
    }
}

// ---- sharded solvers: ranks of a process group, or of an in-process group -----------------------------------------------------
extern "C" hprlp_local_group *hprlp_local_group_create(int size) {
    return guarded(static_cast<hprlp_local_group *>(nullptr), [&] {
        auto *h = new hprlp_local_group();
        h->g = make_local_group(size);
        return h;
    });
}
extern "C" void hprlp_local_group_destroy(hprlp_local_group *h) {
    if (!h) return;
    free_local_group(h->g);
    delete h;
}

// A launcher that hands over TWO unique ids (256 bytes, hprlp_dist_unique_id with a 256-byte buffer) gets a second
// communicator for the exchange stream: the exchanges that overlap the local part of a half-step are enqueued on another
// stream than the collectives of the check iterations, and one RCCL communicator must not be driven from two streams.
static void make_exchange_comm(hprlp_solver *h, int rank, int size, const void *unique_id, int id_bytes, int device) {
    if (!unique_id || id_bytes < 256) return;
    // a launcher that padded ONE id to 256 bytes: bytes 128..255 hold no id -- single communicator (the documented fallback)
    bool any = false;
    for (int k = 128; k < 256; ++k) any = any || static_cast<const unsigned char *>(unique_id)[k] != 0;
    if (!any) return;
    h->xcomm = make_rccl_comm(rank, size, static_cast<const char *>(unique_id) + 128, 128, device);
    h->s.xcomm = h->xcomm;
}

// The transport a (rank, size, id) names: a shared-memory group of processes (id made under HPRLP_DIST_TRANSPORT=shm; staging
// room = one full-length vector per rank) or RCCL communicators (one, or two when the launcher handed over two ids).
static void make_transport(hprlp_solver *h, int m, int n, int rank, int size, const void *unique_id, int id_bytes, int device) {
    if (is_shm_unique_id(unique_id, static_cast<size_t>(id_bytes))) {
        const size_t area = (static_cast<size_t>(std::max(m, n)) + 64u * static_cast<size_t>(size)) * sizeof(double) + 4096u * static_cast<size_t>(size + 1);
        h->comm = make_shm_comm(rank, size, unique_id, static_cast<size_t>(id_bytes), area, device);
        return;
    }
    h->comm = make_rccl_comm(rank, size, unique_id, static_cast<size_t>(id_bytes), device);
    make_exchange_comm(h, rank, size, unique_id, id_bytes, device);
}

// Rank `rank` of `size` from its shard (no rank ever holds the whole matrix: SURVEY.md 8d, config 5 "generated per shard"):
// RCCL or shared-memory transport from unique_id, or (group != NULL) the in-process group.  The shard stays the caller's.  A
// failure destroys the handle before this returns: a background tiling job may still read the shard arrays (the solver's
// destructor joins it), so the caller may free them afterwards.
static hprlp_solver *create_from_shard(const hprlp_shard *sh, const HPRLP_parameters *param, int rank, int size, const void *unique_id,
                                       int id_bytes, hprlp_local_group *group) {
    hprlp_solver *h = nullptr;
    hprlp_solver *made = guarded(static_cast<hprlp_solver *>(nullptr), [&] {
        if (!sh || !sh->A_rowptr || !sh->AT_rowptr || (sh->m_loc > 0 && !(sh->AL && sh->AU)) || (sh->n_loc > 0 && !(sh->l && sh->u && sh->c)))
            throw std::runtime_error("incomplete shard");
        if (sh->A_rowptr[sh->m_loc] > 0 && !(sh->A_col && sh->A_val)) throw std::runtime_error("incomplete shard (A)");
        if (sh->AT_rowptr[sh->n_loc] > 0 && !(sh->AT_col && sh->AT_val)) throw std::runtime_error("incomplete shard (A^T)");
        HPRLP_parameters dflt;
        const HPRLP_parameters *p = param ? param : &dflt;
        h = new hprlp_solver();
        h->sharded = true;
        h->s.verbose = false;
        HIP_CHECK(hipSetDevice(p->device_number));
        if (group) {
            h->comm = make_local_comm(group->g, rank);
        } else if (size > 1 || (unique_id && id_bytes >= 128)) {
            // a unique id given with size 1 builds a one-rank RCCL communicator (exercises the collective path)
            make_transport(h, sh->m, sh->n, rank, size, unique_id, id_bytes, p->device_number);
        }
        h->s.setup_shard(sh->m, sh->n, sh->row_off, sh->m_loc, sh->col_off, sh->n_loc, sh->A_rowptr, sh->A_col, sh->A_val, sh->AT_rowptr,
                         sh->AT_col, sh->AT_val, sh->AL, sh->AU, sh->l, sh->u, sh->c, sh->obj_constant, p, h->comm);
        return h;
    });
    if (!made) destroy_handle(h);
    return made;
}

// The same from the whole model: this rank's shard is cut out, used and freed (after the handle, should the set-up fail)
static hprlp_solver *create_sharded(const LP_info_cpu *model, const HPRLP_parameters *param, int rank, int size,
                                    const void *unique_id, int id_bytes, hprlp_local_group *group) {
    if (!model) {
        set_last_error("null model");
        return nullptr;
    }
    hprlp_shard sh;
    std::memset(&sh, 0, sizeof(sh));
    if (hprlp_extract_shard(model, rank, size, &sh) != 0) return nullptr;  // (its message stands; it has freed what it had)
    hprlp_solver *h = create_from_shard(&sh, param, rank, size, unique_id, id_bytes, group);
    hprlp_free_shard(&sh);
    return h;
}

extern "C" hprlp_solver *hprlp_solver_create_dist(const LP_info_cpu *model, const HPRLP_parameters *param, int rank,
                                                  int size, const void *unique_id, int id_bytes) {
    return create_sharded(model, param, rank, size, unique_id, id_bytes, nullptr);
}

extern "C" hprlp_solver *hprlp_solver_create_dist_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                             const void *unique_id, int id_bytes) {
    return create_from_shard(shard, param, rank, size, unique_id, id_bytes, nullptr);
}

extern "C" hprlp_solver *hprlp_solver_create_local_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                              hprlp_local_group *group) {
    if (!group) {
        set_last_error("null local group");
        return nullptr;
    }
    return create_from_shard(shard, param, rank, size, nullptr, 0, group);
}

extern "C" hprlp_solver *hprlp_solver_create_local(const LP_info_cpu *model, const HPRLP_parameters *param, int rank,
                                                   int size, hprlp_local_group *group) {
    if (!group) {
        set_last_error("null local group");
        return nullptr;
    }
    return create_sharded(model, param, rank, size, nullptr, 0, group);
}

// out = {halo_m sparse?, entries sent, entries received, halo_n sparse?, sent, received, requests m, requests n}
extern "C" int hprlp_solver_dist_info(hprlp_solver *h, long out[8]) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_dist_info", out, "output");
        out[0] = s.halo_m.sparse; out[1] = s.halo_m.nsend; out[2] = s.halo_m.nrecv;
        out[3] = s.halo_n.sparse; out[4] = s.halo_n.nsend; out[5] = s.halo_n.nrecv;
        out[6] = s.halo_m.total_requests; out[7] = s.halo_n.total_requests;
        return 0;
    });
}

// out = {ranks / this rank / device as the main communicator reports them (RCCL: ncclCommCount, ncclCommUserRank,
//        ncclCommCuDevice), the same three of the exchange stream's communicator (0, -1, -1 if there is none), the
//        solver's HIP device, 1 if the exchange overlaps the local part of the half-steps}
extern "C" int hprlp_solver_dist_comm_info(hprlp_solver *h, long out[8]) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_dist_comm_info", out, "output");
        for (int i = 0; i < 8; ++i) out[i] = 0;
        out[1] = out[2] = out[4] = out[5] = -1;
        if (s.comm) { out[0] = s.comm->reported_ranks(); out[1] = s.comm->reported_rank(); out[2] = s.comm->reported_device(); }
        if (s.xcomm) { out[3] = s.xcomm->reported_ranks(); out[4] = s.xcomm->reported_rank(); out[5] = s.xcomm->reported_device(); }
        out[6] = s.prm.device_number;
        out[7] = s.overlap_enabled ? 1 : 0;
        return 0;
    });
}

// One grouped send/recv of `count` doubles from this rank to ITSELF through the solver's communicator (pattern
// i -> 3 i + 1), checked on the host: exercises the point-to-point entry points of the transport (RCCL: ncclGroupStart /
// ncclSend / ncclRecv / ncclGroupEnd) on a box where no second rank can exist.  0 = delivered intact.
extern "C" int hprlp_solver_dist_loopback(hprlp_solver *h, int count) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_dist_loopback");
        if (!s.comm) throw std::runtime_error("solver has no communicator");
        if (count <= 0) throw std::runtime_error("count must be positive");
        std::vector<double> src(static_cast<size_t>(count)), dst(static_cast<size_t>(count), -1.0);
        for (int i = 0; i < count; ++i) src[i] = 3.0 * i + 1.0;
        DBuf<double> a(src.size()), b(dst.size());
        a.upload(src.data(), src.size());
        b.upload(dst.data(), dst.size());
        const P2P op{s.comm->rank, a.p, src.size() * sizeof(double), b.p, dst.size() * sizeof(double)};
        s.comm->exchange(&op, 1, s.stream);
        HIP_CHECK(hipStreamSynchronize(s.stream));
        b.download(dst.data(), dst.size());
        for (int i = 0; i < count; ++i)
            if (dst[i] != src[i]) throw std::runtime_error("loopback send/recv delivered wrong data at element " + std::to_string(i));
        return 0;
    });
}

// ---- the steps of a solve -------------------------------------------------------------------------------------------------
extern "C" void hprlp_solver_set_verbose(hprlp_solver *h, int verbose) {
    guarded(0, [&] {
        solver_of(h, "hprlp_solver_set_verbose").verbose = verbose != 0;
        return 0;
    });
}

extern "C" int hprlp_solver_scale(hprlp_solver *h) {
    return guarded(-1, [&] {
        solver_of(h, "hprlp_solver_scale").scale();
        return 0;
    });
}

extern "C" double hprlp_solver_power_iteration(hprlp_solver *h, int max_iter, double tol, int *iters_out) {
    return guarded(-1.0, [&] { return solver_of(h, "hprlp_solver_power_iteration").power_iteration(max_iter, tol, iters_out); });
}

extern "C" int hprlp_solver_init(hprlp_solver *h, double sigma, double lambda_max) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_init");
        s.lambda_max = lambda_max;
        if (sigma > 0) s.set_sigma_lambda(sigma, lambda_max, true);
        else s.init_iteration_state();
        HIP_CHECK(hipStreamSynchronize(s.stream));
        return 0;
    });
}

extern "C" int hprlp_solver_reset_iterates(hprlp_solver *h) {
    return guarded(-1, [&] {
        solver_of(h, "hprlp_solver_reset_iterates").reset_iterates();
        return 0;
    });
}

extern "C" int hprlp_solver_iterate(hprlp_solver *h, int normal, int then_check) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_iterate");
        if (then_check) s.run_normal_then_check(normal);
        else s.run_normal(normal);
        HIP_CHECK(hipStreamSynchronize(s.stream));
        return 0;
    });
}

extern "C" int hprlp_solver_residuals(hprlp_solver *h, int iter, int compute_gap, double out[8]) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_residuals");
        Residuals r;
        RestartState rs;
        s.compute_residuals(iter, compute_gap != 0, &r, &rs);
        out[0] = r.err_Rp; out[1] = r.err_Rd; out[2] = r.primal_obj; out[3] = r.dual_obj;
        out[4] = r.rel_gap; out[5] = r.kkt; out[6] = rs.current_gap; out[7] = s.lambda_max;
        return 0;
    });
}

extern "C" int hprlp_solver_restart(hprlp_solver *h, const double in[6], double *sigma_out) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_restart");
        RestartState rs;
        rs.flag = 1;
        rs.first = false;
        rs.current_gap = in[0]; rs.best_gap = in[1]; rs.best_sigma = in[2];
        Residuals r;
        r.err_Rd = in[3]; r.err_Rp = in[4]; r.rel_gap = in[5];
        s.update_sigma_and_restart(&rs, r);
        HIP_CHECK(hipStreamSynchronize(s.stream));
        if (sigma_out) *sigma_out = s.sigma;
        return 0;
    });
}

extern "C" double hprlp_solver_weighted_norm(hprlp_solver *h) {
    return guarded(-1.0, [&] { return solver_of(h, "hprlp_solver_weighted_norm").weighted_norm_after_restart(); });
}

extern "C" int hprlp_solver_run(hprlp_solver *h, HPRLP_results *out, hprlp_trace_row *trace, int max_trace,
                                int *n_trace) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_run");
        TraceScope scope(s, trace, max_trace);
        s.solve_loop(out);
        s.collect_solution(out);
        if (n_trace) *n_trace = s.trace_n;
        return 0;
    });
}

// ---- vectors by name, scalars, info -------------------------------------------------------------------------------------------
namespace {
struct VecRef {
    double *p;
    long n;
    char kind;  // 'r': per row of A, 'c': per column, '-': raw (matrix values)
};
VecRef find_vector(Solver &s, const std::string &name) {
    if (name == "x") return {s.x.p, s.n_loc, 'c'};
    if (name == "last_x") return {s.last_x.p, s.n_loc, 'c'};
    if (name == "x_hat") return {s.x_hat, s.n_loc, 'c'};
    if (name == "x_bar") return {s.x_bar, s.n_loc, 'c'};
    if (name == "z_bar") return {s.z_bar.p, s.n_loc, 'c'};
    if (name == "x_temp") return {s.x_temp, s.n_loc, 'c'};
    if (name == "y") return {s.y, s.m_loc, 'r'};
    if (name == "last_y") return {s.last_y.p, s.m_loc, 'r'};
    if (name == "y_bar") return {s.y_bar, s.m_loc, 'r'};
    if (name == "y_obj") return {s.y_obj.p, s.m_loc, 'r'};
    if (name == "y_temp") return {s.y_temp.p, s.m_loc, 'r'};
    if (name == "AL") return {s.AL.p, s.m_loc, 'r'};
    if (name == "AU") return {s.AU.p, s.m_loc, 'r'};
    if (name == "l") return {s.l.p, s.n_loc, 'c'};
    if (name == "u") return {s.u.p, s.n_loc, 'c'};
    if (name == "c") return {s.c.p, s.n_loc, 'c'};
    if (name == "row_norm") return {s.row_norm.p, s.m_loc, 'r'};
    if (name == "col_norm") return {s.col_norm.p, s.n_loc, 'c'};
    if (name == "A_val") return {s.A.val.p, s.A.view.nnz, '-'};
    if (name == "AT_val") return {s.AT.val.p, s.AT.view.nnz, '-'};
    // the power iteration's two scratch vectors (the scaling's gathered ones), this rank's slices: zero between the phases
    if (name == "gsm") return {s.gsm.p + s.row_off, s.m_loc, 'r'};
    if (name == "gsn") return {s.gsn.p + s.col_off, s.n_loc, 'c'};
    if (s.ray_prev_x.p) {  // the ray test's vectors, once Solver::ray_begin has allocated them (scaled units)
        if (name == "ray_d") return {s.ray_d.p, s.n_loc, 'c'};
        if (name == "ray_prev_x") return {s.ray_prev_x.p, s.n_loc, 'c'};
        if (name == "ray_y") return {s.ray_y.p, s.m_loc, 'r'};
        if (name == "ray_prev_y") return {s.ray_prev_y.p, s.m_loc, 'r'};
    }
    return {nullptr, -1, '-'};
}
// the permutation (device index -> caller's index) that applies to a vector, or null
const std::vector<int> *perm_of(const Solver &s, const VecRef &v) {
    if (v.kind == 'r' && !s.perm_r.empty()) return &s.perm_r;
    if (v.kind == 'c' && !s.perm_c.empty()) return &s.perm_c;
    return nullptr;
}
}  // namespace

// Vectors travel in the caller's numbering: with a set-up time locality ordering in place (solver.h: perm_r / perm_c)
// the device order is un-permuted on the way out and permuted on the way in.  A_val / AT_val are the device arrays as
// they are (entries of the permuted matrix).
extern "C" long hprlp_solver_get_vector(hprlp_solver *h, const char *name, double *out, long cap) {
    return guarded(-1L, [&] {
        Solver &s = solver_of(h, "hprlp_solver_get_vector");
        VecRef v = find_vector(s, name ? name : "");
        if (v.n < 0) throw std::runtime_error(std::string("unknown vector name: ") + (name ? name : "(null)"));
        if (cap < v.n) throw std::runtime_error("output buffer too small");
        HIP_CHECK(hipStreamSynchronize(s.stream));
        if (v.n > 0) {
            if (const std::vector<int> *perm = perm_of(s, v)) {
                std::vector<double> tmp(static_cast<size_t>(v.n));
                HIP_CHECK(hipMemcpy(tmp.data(), v.p, sizeof(double) * v.n, hipMemcpyDeviceToHost));
                for (long i = 0; i < v.n; ++i) out[(*perm)[i]] = tmp[i];
            } else {
                HIP_CHECK(hipMemcpy(out, v.p, sizeof(double) * v.n, hipMemcpyDeviceToHost));
            }
        }
        return v.n;
    });
}

extern "C" int hprlp_solver_set_vector(hprlp_solver *h, const char *name, const double *in, long len) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_set_vector");
        VecRef v = find_vector(s, name ? name : "");
        if (v.n < 0) throw std::runtime_error(std::string("unknown vector name: ") + (name ? name : "(null)"));
        if (len != v.n) throw std::runtime_error("length mismatch");
        s.invalidate_far();
        HIP_CHECK(hipStreamSynchronize(s.stream));
        if (v.n > 0) {
            if (const std::vector<int> *perm = perm_of(s, v)) {
                std::vector<double> tmp(static_cast<size_t>(v.n));
                for (long i = 0; i < v.n; ++i) tmp[i] = in[(*perm)[i]];
                HIP_CHECK(hipMemcpy(v.p, tmp.data(), sizeof(double) * v.n, hipMemcpyHostToDevice));
            } else {
                HIP_CHECK(hipMemcpy(v.p, in, sizeof(double) * v.n, hipMemcpyHostToDevice));
            }
        }
        if (v.p == s.l.p || v.p == s.u.p || v.p == s.AL.p || v.p == s.AU.p) {  // the bound codes follow the arrays
            s.refresh_bound_codes();
            HIP_CHECK(hipStreamSynchronize(s.stream));
        }
        return 0;
    });
}

extern "C" int hprlp_solver_get_scalars(hprlp_solver *h, double out[16]) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_get_scalars");
        Ctrl ck;
        HIP_CHECK(hipStreamSynchronize(s.stream));
        HIP_CHECK(hipMemcpy(&ck, s.ctrl.p, sizeof(Ctrl), hipMemcpyDeviceToHost));
        const double v[16] = {s.b_scale, s.c_scale, s.norm_b, s.norm_c, s.norm_b_org, s.norm_c_org, s.sigma, s.lambda_max,
                              s.setup_time, s.scaling_time, s.power_time, static_cast<double>(s.power_iters),
                              static_cast<double>(ck.kx), static_cast<double>(ck.ky), 0, 0};
        for (int i = 0; i < 16; ++i) out[i] = v[i];
        return 0;
    });
}

extern "C" int hprlp_solver_info(hprlp_solver *h, long out[8]) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_info");
        s.finish_tiling();  // report the kernels that will actually run
        out[0] = s.m; out[1] = s.n; out[2] = s.A.view.nnz;
        out[3] = s.A.view.nblk; out[4] = s.AT.view.nblk;
        out[5] = s.A.view.grid(); out[6] = s.AT.view.grid();
        // bit0: A tiled, bit1: A^T tiled, bit2: normal iterations run in the single-workgroup small-LP kernel
        // bit3: a set-up time locality ordering is in place (the device works on P A Q)
        out[7] = (s.A.view.tiled.valid ? 1 : 0) + (s.AT.view.tiled.valid ? 2 : 0) + (s.use_small && !s.comm ? 4 : 0) + (s.perm_r.empty() ? 0 : 8);
        return 0;
    });
}

// ---- detection, ray step, warm start ------------------------------------------------------------------------------------------
extern "C" int hprlp_solver_set_detection(hprlp_solver *h, const hprlp_detection *det) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_detection";
        Solver &s = solver_of(h, who);
        if (det) single_gpu_only(h, who, "infeasibility detection runs on one GPU only");
        Detection d;
        detection_from(det, &d);
        s.detect = d;
        return 0;
    });
}

// One ray test outside the loop: the evaluation a periodic check of solve_loop runs (residuals with the gap, then the ray test,
// one fetch), so the nine slots come the way the loop reads them.  Solver::detect is not touched.
extern "C" int hprlp_solver_ray_step(hprlp_solver *h, int restart, double out[9]) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_ray_step";
        Solver &s = solver_of(h, who, out, "output");
        single_gpu_only(h, who, "infeasibility detection runs on one GPU only");
        if (restart) s.ray_begin();
        else if (!s.ray_prev_x.p) throw std::runtime_error("hprlp_solver_ray_step: the first step of a solver needs restart != 0");
        Residuals r;
        RestartState rs;
        bool ray = false;
        s.compute_residuals(1, true, &r, &rs, &ray);
        if (!ray) return 0;
        const int slots[9] = {S_RAY_DY, S_RAY_CD, S_RAY_VY, S_RAY_WD, S_RAY_YN, S_RAY_DN, S_RAY_DZ, S_RAY_VZ, S_RAY_WQ};
        for (int k = 0; k < 9; ++k) out[k] = s.scal_h[slots[k]];
        return 1;
    });
}

extern "C" int hprlp_solver_set_start(hprlp_solver *h, const double *x0, const double *y0) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_start";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "warm start runs on one GPU only");
        check_start(x0, s.n, "x0");
        check_start(y0, s.m, "y0");
        s.set_start(x0, y0);
        return 0;
    });
}

extern "C" int hprlp_solver_get_certificate(hprlp_solver *h, hprlp_certificate *cert) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_get_certificate", cert, "certificate");
        if (!export_certificate(s.cert, cert, s.m, s.n)) throw std::runtime_error("host allocation of the certificate failed");
        return 0;
    });
}

// ---- re-solve (DESIGN.md "Re-solve"): new data for the resident LP, then a further solve on the same solver ------------------
extern "C" int hprlp_solver_set_data(hprlp_solver *h, const double *c, const double *obj_constant, const double *AL, const double *AU,
                                     const double *l, const double *u) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_data";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "new data for a resident model runs on one GPU only");
        s.set_data(c, obj_constant, AL, AU, l, u);
        return 0;
    });
}

extern "C" int hprlp_solver_resolve(hprlp_solver *h, double sigma, const double *x0, const double *y0, HPRLP_results *out,
                                    hprlp_trace_row *trace, int max_trace, int *n_trace) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_resolve";
        Solver &s = solver_of(h, who, out, "result");
        single_gpu_only(h, who, "a re-solve runs on one GPU only");
        if (std::isnan(sigma)) throw std::runtime_error("hprlp_solver_resolve: sigma is NaN");
        check_start(x0, s.n, "x0");
        check_start(y0, s.m, "y0");
        TraceScope scope(s, trace, max_trace);
        s.resolve(sigma, x0, y0, out);
        if (n_trace) *n_trace = s.trace_n;
        return 0;
    });
}

extern "C" int hprlp_solver_data_seconds(hprlp_solver *h, double out[3]) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_data_seconds", out, "output");
        for (int i = 0; i < 3; ++i) out[i] = s.data_time[i];
        return 0;
    });
}

// Matrix values (DESIGN.md "Matrix values"): new values on the resident pattern, then hprlp_solver_power_iteration / _init / _resolve
extern "C" int hprlp_solver_set_matrix_values(hprlp_solver *h, const double *val, long nnz, const double *c, const double *obj_constant,
                                              const double *AL, const double *AU, const double *l, const double *u) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_matrix_values";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "new matrix values for a resident model run on one GPU only", "them");
        s.set_matrix_values(val, nnz, c, obj_constant, AL, AU, l, u);
        return 0;
    });
}

extern "C" int hprlp_solver_matrix_seconds(hprlp_solver *h, double out[6]) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_matrix_seconds", out, "output");
        for (int i = 0; i < 5; ++i) out[i] = s.matrix_time[i];
        out[5] = static_cast<double>(s.matrix_calls);
        return 0;
    });
}

// Device-resident re-solve (DESIGN.md "Device-resident re-solve"): the three entries above with the vectors in device memory
extern "C" int hprlp_solver_set_data_device(hprlp_solver *h, const double *dc, const double *obj_constant, const double *dAL,
                                            const double *dAU, const double *dl, const double *du, void *stream) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_data_device";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "new data for a resident model runs on one GPU only");
        s.set_data_device(dc, obj_constant, dAL, dAU, dl, du, static_cast<hipStream_t>(stream));
        return 0;
    });
}

extern "C" int hprlp_solver_resolve_device(hprlp_solver *h, double sigma, const double *dx0, const double *dy0, void *stream, double *dx,
                                           double *dy, double *dz, HPRLP_results *out, hprlp_trace_row *trace, int max_trace,
                                           int *n_trace) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_resolve_device";
        Solver &s = solver_of(h, who, out, "result");
        single_gpu_only(h, who, "a re-solve runs on one GPU only");
        if (std::isnan(sigma)) throw std::runtime_error("hprlp_solver_resolve_device: sigma is NaN");
        TraceScope scope(s, trace, max_trace);
        s.resolve_device(sigma, dx0, dy0, static_cast<hipStream_t>(stream), dx, dy, dz, out);
        if (n_trace) *n_trace = s.trace_n;
        return 0;
    });
}

extern "C" int hprlp_solver_set_matrix_values_device(hprlp_solver *h, const double *dval, long nnz, const double *dc,
                                                     const double *obj_constant, const double *dAL, const double *dAU, const double *dl,
                                                     const double *du, void *stream) {
    return guarded(-1, [&] {
        const char *who = "hprlp_solver_set_matrix_values_device";
        Solver &s = solver_of(h, who);
        single_gpu_only(h, who, "new matrix values for a resident model run on one GPU only", "them");
        s.set_matrix_values_device(dval, nnz, dc, obj_constant, dAL, dAU, dl, du, static_cast<hipStream_t>(stream));
        return 0;
    });
}

extern "C" int hprlp_solver_transfer(hprlp_solver *h, long out[4]) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_transfer", out, "output");
        for (int i = 0; i < 4; ++i) out[i] = s.transfer[i];
        return 0;
    });
}

// ---- value maps, ordering, power start, describe, form facts, timing ------------------------------------------------------------
// The value maps as the solver built them (built here if no hprlp_solver_set_matrix_values call has done it yet); mapA / mapAT
// receive nnz ints each.  Returns nnz.
extern "C" long hprlp_solver_value_maps(hprlp_solver *h, int *mapA, int *mapAT, long cap) {
    return guarded(-1L, [&] {
        Solver &s = solver_of(h, "hprlp_solver_value_maps", mapA && mapAT ? mapA : nullptr, "output");
        if (h->sharded) throw std::runtime_error("hprlp_solver_value_maps: one GPU only; a sharded solver has no value maps");
        const long nnz = s.A.view.nnz;
        if (cap < nnz) throw std::runtime_error("hprlp_solver_value_maps: output buffers too small");
        s.build_value_maps();
        HIP_CHECK(hipStreamSynchronize(s.stream));
        if (nnz > 0) {
            if (s.map_A.p) HIP_CHECK(hipMemcpy(mapA, s.map_A.p, sizeof(int) * nnz, hipMemcpyDeviceToHost));
            else
                for (long e = 0; e < nnz; ++e) mapA[e] = static_cast<int>(e);
            HIP_CHECK(hipMemcpy(mapAT, s.map_AT.p, sizeof(int) * nnz, hipMemcpyDeviceToHost));
        }
        return nnz;
    });
}

// The locality ordering a solver applied: row_new2old (m) / col_new2old (n) as perm_r / perm_c hold them.  Returns 1 with the
// arrays filled, 0 without an ordering (arrays untouched).
extern "C" int hprlp_solver_ordering(hprlp_solver *h, int *row_new2old, int *col_new2old) {
    return guarded(-1, [&] {
        const Solver &s = solver_of(h, "hprlp_solver_ordering", row_new2old && col_new2old ? row_new2old : nullptr, "output");
        if (s.perm_r.empty()) return 0;
        std::copy(s.perm_r.begin(), s.perm_r.end(), row_new2old);
        std::copy(s.perm_c.begin(), s.perm_c.end(), col_new2old);
        return 1;
    });
}

// The power iteration's start vector as Solver::power_start leaves it on the device, in the caller's numbering.
extern "C" int hprlp_solver_power_start(hprlp_solver *h, double *out, int cap) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_power_start", out, "output");
        if (s.comm) throw std::runtime_error("hprlp_solver_power_start: single-GPU solvers only");
        if (cap < s.m_loc) throw std::runtime_error("hprlp_solver_power_start: output too short");
        s.power_start(s.sm1.p);
        std::vector<double> z(static_cast<size_t>(std::max(s.m_loc, 1)));
        HIP_CHECK(hipMemcpy(z.data(), s.sm1.p, sizeof(double) * static_cast<size_t>(s.m_loc), hipMemcpyDeviceToHost));
        for (int i = 0; i < s.m_loc; ++i) out[s.perm_r.empty() ? i : s.perm_r[i]] = z[i];
        return s.m_loc;
    });
}

// One line per matrix saying which kernel form runs and on what structure (bench.py's ladder, tools/run_mps_dir.py)
extern "C" int hprlp_solver_describe(hprlp_solver *h, char *buf, int cap) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_describe", cap > 0 ? buf : nullptr, "buffer");
        s.finish_tiling();
        auto one = [](const char *name, const DeviceMatrix &M) {
            const TiledDev &t = M.view.tiled;
            std::string d = std::string(name) + ": ";
            if (!t.valid) {
                d += "stream kernel (k_spmv_fused, " + std::to_string(M.view.nblk) + " row blocks, " + std::to_string(M.view.nlong) + " split rows)";
                d += no_tiled_note(M.outcome.why);
                return d;
            }
            d += t.n_pieces > 0 ? "tiled, piece form (k_tiled_part + k_tiled_finish, " + std::to_string(t.n_pieces) + " pieces)"
                 : t.rem_cap == kPbRemCap ? "tiled, all-remainder form (k_pb_fused, grid " + std::to_string(t.grid) + ")"
                                          : "tiled, fused (k_tiled_fused, grid " + std::to_string(t.grid) + ")";
            d += ", " + std::to_string(t.nsb) + " super-blocks, " + std::to_string(M.tiled.n_steps) + " steps";
            if (t.R != kTileRows || t.T != kTileCols) d += " (" + std::to_string(t.R) + " rows, tiles of " + std::to_string(t.T) + " columns)";
            const double all = static_cast<double>(M.tiled.dense_entries) + static_cast<double>(M.tiled.n_rem);
            if (all > 0) d += ", " + std::to_string(static_cast<int>(100.0 * M.tiled.dense_entries / all + 0.5)) + " % of the entries in staged tiles";
            if (t.f_rk) d += ", source-side run tables";
            if (t.f_work) d += ", pre-pass work list of " + std::to_string(t.n_work) + " workgroups for " + std::to_string(t.n_groups) + " source groups";
            if (t.side_nblk > 0) d += ", long rows aside (" + std::to_string(t.side_nblk) + " blocks through the stream kernel)";
            if (t.repeats) d += ", repeats";  // (some tile has several steps: the <.., REP = true> instantiations run)
            return d;
        };
        std::string d = one("A", s.A) + "; " + one("A^T", s.AT);
        if (s.use_small && !s.comm) d += "; normal iterations in the single-workgroup kernel (k_small_iterations)";
        if (!s.perm_r.empty()) d += "; locality ordering applied at set-up";
        // (anything but the default path says so: the switches this solver was set up under, and hooks that were set but not honoured)
        if (!s.env_at_setup.empty()) d += "; switches: " + s.env_at_setup;
        if (!s.env_ignored_at_setup.empty()) d += "; ignored without HPRLP_TEST_HOOKS=1: " + s.env_ignored_at_setup;
        std::snprintf(buf, static_cast<size_t>(cap), "%s", d.c_str());
        return static_cast<int>(d.size());
    });
}

extern "C" int hprlp_solver_form_facts(hprlp_solver *h, int which, hprlp_form_facts out[2]) {
    return guarded(-1, [&] {
        if (!h || !out || which < 0 || which > 1) throw std::runtime_error("hprlp_solver_form_facts: null solver / buffer, or no such matrix");
        Solver &s = solver_of(h, "hprlp_solver_form_facts");
        s.finish_tiling();
        const DeviceMatrix &M = which ? s.AT : s.A;
        out[0] = M.facts;
        out[1] = M.facts_pb;
        return M.passes;
    });
}

extern "C" int hprlp_solver_time_iterations(hprlp_solver *h, int warmup, int steps, int mode, double *total_ms,
                                            double *xhalf_ms, double *yhalf_ms) {
    return guarded(-1, [&] {
        Solver &s = solver_of(h, "hprlp_solver_time_iterations");
        if (steps <= 0) throw std::runtime_error("steps must be positive");
        s.run_normal(warmup);
        HIP_CHECK(hipStreamSynchronize(s.stream));
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        double tx = 0, ty = 0;
        float ms = 0;
        // events before / between / after the two halves of every step; the halves' times summed into tx / ty
        std::vector<hipEvent_t> ev(mode == 0 ? 0 : static_cast<size_t>(steps) * 3);
        for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
        if (mode == 2) s.invalidate_far();
        HIP_CHECK(hipEventRecord(e0, s.stream));
        if (mode == 0) {
            s.run_normal(steps);
        } else if (mode == 2) {
            // the bare SpMVs of the path (A^T y into scratch, A x_hat into scratch): no half-step update, no state change
            for (int i = 0; i < steps; ++i) {
                HIP_CHECK(hipEventRecord(ev[3 * i], s.stream));
                launch_spmv_plain(s.AT.view, s.gy.p, s.sn1.p, nullptr, false, nullptr, 0, s.stream);
                HIP_CHECK(hipEventRecord(ev[3 * i + 1], s.stream));
                launch_spmv_plain(s.A.view, s.gxh.p, s.sm1.p, nullptr, false, nullptr, 0, s.stream);
                HIP_CHECK(hipEventRecord(ev[3 * i + 2], s.stream));
            }
        } else {
            // the solver's own normal pair (with the multi-GPU overlap when it is on)
            for (int i = 0; i < steps; ++i) s.launch_normal_pair(i + 1 < steps, &ev[3 * static_cast<size_t>(i)], s.x_mode_of(i, steps));
        }
        HIP_CHECK(hipEventRecord(e1, s.stream));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        for (size_t i = 0; i < ev.size(); i += 3) {
            float a = 0, b = 0;
            HIP_CHECK(hipEventElapsedTime(&a, ev[i], ev[i + 1]));
            HIP_CHECK(hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]));
            tx += a;
            ty += b;
        }
        for (auto &e : ev) (void)hipEventDestroy(e);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (total_ms) *total_ms = ms;
        if (xhalf_ms) *xhalf_ms = tx;
        if (yhalf_ms) *yhalf_ms = ty;
        return 0;
    });
}
