// abi_batched.cpp -- extern "C" boundary, one matrix and many right-hand sides: hprlp_solve_batched_detect / _warm, the batched
// certificates, every hprlp_batched_solver_* entry (the resident solver: batches, streams, their device twins) and
// hprlp_batched_prepare_host*.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "abi_common.h"
#include "batch_prep.h"
#include "stream_schedule.h"

using namespace hprlp;

// sizes and zeroed per-member arrays (kind 0 for every member), no ray arrays
bool hprlp::clear_batched_certificates(hprlp_batched_certificates *c, int B, int m, int n) {
    std::memset(c, 0, sizeof(*c));
    c->batch_size = B;
    c->m = m;
    c->n = n;
    if (B <= 0) return true;
    c->kind = static_cast<int *>(std::calloc(B, sizeof(int)));
    c->iter = static_cast<int *>(std::calloc(B, sizeof(int)));
    c->objective = static_cast<double *>(std::calloc(B, sizeof(double)));
    c->violation = static_cast<double *>(std::calloc(B, sizeof(double)));
    return c->kind && c->iter && c->objective && c->violation;
}

// one Certificate per member -> column-major arrays (a member's columns stay zero where its kind does not use them)
bool hprlp::export_batched_certificates(const std::vector<Certificate> &k, hprlp_batched_certificates *c) {
    const int B = c->batch_size;
    const size_t m = static_cast<size_t>(c->m), n = static_cast<size_t>(c->n);
    bool any_y = false, any_d = false;
    for (int j = 0; j < B && j < static_cast<int>(k.size()); ++j) {
        c->kind[j] = k[j].kind;
        c->iter[j] = k[j].iter;
        c->objective[j] = k[j].objective;
        c->violation[j] = k[j].violation;
        any_y = any_y || k[j].kind == 1;
        any_d = any_d || k[j].kind == 2;
    }
    auto panel = [B](size_t rows, double **out) {
        *out = static_cast<double *>(std::calloc(std::max<size_t>(rows * B, 1), sizeof(double)));
        return *out != nullptr;
    };
    if ((any_y && (!panel(m, &c->y) || !panel(n, &c->z))) || (any_d && !panel(n, &c->d))) return false;
    for (int j = 0; j < B && j < static_cast<int>(k.size()); ++j) {
        if (k[j].kind == 1) {
            std::memcpy(c->y + j * m, k[j].y.data(), sizeof(double) * m);
            std::memcpy(c->z + j * n, k[j].z.data(), sizeof(double) * n);
        } else if (k[j].kind == 2) {
            std::memcpy(c->d + j * n, k[j].d.data(), sizeof(double) * n);
        }
    }
    return true;
}

extern "C" void hprlp_free_batched_certificates(hprlp_batched_certificates *certs) {
    if (!certs) return;
    for (void *p : {static_cast<void *>(certs->kind), static_cast<void *>(certs->iter), static_cast<void *>(certs->objective),
                    static_cast<void *>(certs->violation), static_cast<void *>(certs->y), static_cast<void *>(certs->z),
                    static_cast<void *>(certs->d)})
        std::free(p);
    certs->kind = certs->iter = nullptr;
    certs->objective = certs->violation = certs->y = certs->z = certs->d = nullptr;
}

// certs (may be null) cleared to the call's sizes; without memory nothing stays allocated
static void clear_or_throw(hprlp_batched_certificates *certs, int B, int m, int n) {
    if (!certs || clear_batched_certificates(certs, B, m, n)) return;
    hprlp_free_batched_certificates(certs);
    throw std::runtime_error("host allocation of the certificates failed");
}

// hprlp_solve_batched_detect and hprlp_solve_batched_warm (`who`, for the error messages), as solve_entry: no detection and no
// starts are exactly solve_batched(); the certificates are cleared on entry and filled only when detection ran
static HPRLP_batched_results solve_batched_entry(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                                 const double *AU, const double *l, const double *u, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *X0, const double *Y0,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs, const char *who) {
    const int m = model ? model->m : 0, n = model ? model->n : 0, B = std::max(batch_size, 0);
    const bool warm = X0 || Y0;
    try {
        clear_or_throw(certs, B, m, n);
        if (!det && !warm) return solve_batched(model, batch_size, C, AL, AU, l, u, obj_constants, param);
        if (warm) {
            if (!model) throw std::runtime_error("null model");
            check_start(X0, static_cast<long>(n) * B, "X0");
            check_start(Y0, static_cast<long>(m) * B, "Y0");
        }
        Detection d;
        const bool with_det = detection_from(det, &d);
        std::vector<Certificate> k;
        HPRLP_batched_results r = solve_batched_impl(model, batch_size, C, AL, AU, l, u, obj_constants, param, with_det ? &d : nullptr,
                                                     with_det && certs ? &k : nullptr, X0, Y0);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            free_batched_results(&r);
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        return r;
    } catch (const std::exception &e) {  // (not guarded(): the fail value is built from the sizes, and the failure is printed)
        set_last_error(e.what());
        std::cerr << "[error] " << who << " failed: " << e.what() << std::endl;
        return make_batched_error("ERROR", m, n, B);
    }
}

extern "C" HPRLP_batched_results hprlp_solve_batched_detect(const LP_info_cpu *model, int batch_size, const double *C,
                                                            const double *AL, const double *AU, const double *l, const double *u,
                                                            const double *obj_constants, const HPRLP_parameters *param,
                                                            const hprlp_detection *det, hprlp_batched_certificates *certs) {
    return solve_batched_entry(model, batch_size, C, AL, AU, l, u, obj_constants, param, nullptr, nullptr, det, certs,
                               "hprlp_solve_batched_detect");
}

extern "C" HPRLP_batched_results hprlp_solve_batched_warm(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                                          const double *AU, const double *l, const double *u,
                                                          const double *obj_constants, const HPRLP_parameters *param,
                                                          const double *X0, const double *Y0, const hprlp_detection *det,
                                                          hprlp_batched_certificates *certs) {
    if (!X0 && !Y0) return hprlp_solve_batched_detect(model, batch_size, C, AL, AU, l, u, obj_constants, param, det, certs);
    return solve_batched_entry(model, batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, det, certs,
                               "hprlp_solve_batched_warm");
}

// ---- resident batches (DESIGN.md "Resident batches"): a sequence of batches over one matrix ------------------------------------
extern "C" hprlp_batched_solver *hprlp_batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param) {
    hprlp_batched_solver *h = nullptr;
    hprlp_batched_solver *made = guarded(static_cast<hprlp_batched_solver *>(nullptr), [&] {
        if (!model || !model->A) throw std::runtime_error("hprlp_batched_solver_create: null model");
        int count = 0;
        if (hipInit(0) != hipSuccess || hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
            (void)hipGetLastError();
            throw std::runtime_error("hprlp_batched_solver_create: no usable GPU");
        }
        h = new hprlp_batched_solver();
        h->s = batched_solver_create(model, param);
        return h;
    });
    if (!made) delete h;
    return made;
}

extern "C" void hprlp_batched_solver_destroy(hprlp_batched_solver *h) {
    if (!h) return;
    batched_solver_destroy(h->s);
    delete h;
}

// The certificate side of the four resident solves.  certs (may be null) is cleared to B members of the solver's sizes, the
// host starts (null: none, or the solver's own check) and the detection are checked, `call` runs with the detection and the
// place for the members' certificates (either may be null: not wanted), and the certificates are exported.  A call that fails
// after the clearing leaves no allocation in certs; `discard` drops what `call` produced when the export is what failed.
template <class Call, class Discard>
static void resident_solve(BatchedSolver *s, int B, const double *X0, const double *Y0, const hprlp_detection *det,
                           hprlp_batched_certificates *certs, Call &&call, Discard &&discard) {
    long mn[8];
    batched_solver_info(s, mn);
    const int m = static_cast<int>(mn[0]), n = static_cast<int>(mn[1]);
    clear_or_throw(certs, B, m, n);
    try {
        check_start(X0, static_cast<long>(n) * B, "X0");
        check_start(Y0, static_cast<long>(m) * B, "Y0");
        Detection d;
        const bool with_det = detection_from(det, &d);
        std::vector<Certificate> k;
        call(with_det ? &d : nullptr, with_det && certs ? &k : nullptr);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            discard();
            throw std::runtime_error("host allocation of the certificates failed");
        }
    } catch (...) {
        hprlp_free_batched_certificates(certs);
        throw;
    }
}

// The device entries: resident_solve with the caller's device buffers and host scalar arrays as a DeviceBatch (the statuses
// zeroed first), and the call's four times handed back.
template <class Call>
static void resident_solve_device(BatchedSolver *s, int B, const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                  double *dx, double *dy, double *dz, hprlp_batched_scalars *out, Call &&call) {
    DeviceBatch db;
    resident_solve(s, B, nullptr, nullptr, det, certs, [&](const Detection *d, std::vector<Certificate> *k) {
        db.stream = stream;
        db.x = dx; db.y = dy; db.z = dz;
        db.primal_obj = out->primal_obj; db.residuals = out->residuals; db.gap = out->gap; db.iter = out->iter; db.status = out->status;
        if (out->status && B > 0) std::memset(out->status, 0, static_cast<size_t>(B) * 64);
        call(d, k, &db);
    }, [] {});
    out->time = db.time; out->setup_time = db.setup_time; out->solve_time = db.solve_time; out->power_time = db.power_time;
}

extern "C" int hprlp_batched_solver_solve(hprlp_batched_solver *h, int batch_size, const double *C, const double *AL, const double *AU,
                                          const double *l, const double *u, const double *obj_constants, const HPRLP_parameters *param,
                                          const double *X0, const double *Y0, int carry, const hprlp_detection *det,
                                          hprlp_batched_certificates *certs, HPRLP_batched_results *out) {
    return guarded(-1, [&] {
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve");
        if (!out) throw std::runtime_error("hprlp_batched_solver_solve: null results");
        HPRLP_batched_results r;
        resident_solve(s, std::max(batch_size, 0), X0, Y0, det, certs, [&](const Detection *d, std::vector<Certificate> *k) {
            batched_solver_solve(s, batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, carry != 0, d, k, &r);
        }, [&] { free_batched_results(&r); });
        *out = r;
        return 0;
    });
}

// ---- streamed batches (DESIGN.md "Streamed batches") ---------------------------------------------------------------------------
// What can be told from the arguments alone is refused first, so that those refusals need no solver (and no GPU).
extern "C" int hprlp_batched_solver_solve_stream(hprlp_batched_solver *h, int count, int width, const double *C, const double *AL,
                                                 const double *AU, const double *l, const double *u, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *X0, const double *Y0,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs,
                                                 HPRLP_batched_results *out) {
    return guarded(-1, [&] {
        // (with param NULL the solver's own parameters decide, and the solver asks again)
        stream_check_call(out != nullptr, count, width, C && AL && AU && l && u, param ? param->max_iter : 0, param ? param->check_iter : 1);
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve_stream");
        HPRLP_batched_results r;
        // (the starts' finite entries: the solver checks them, before it changes)
        resident_solve(s, count, nullptr, nullptr, det, certs, [&](const Detection *d, std::vector<Certificate> *k) {
            batched_solver_solve_stream(s, count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, d, k, &r);
        }, [&] { free_batched_results(&r); });
        *out = r;
        return 0;
    });
}

extern "C" int hprlp_batched_solver_stream_record(hprlp_batched_solver *h, int *slot, int *event_in, int *event_out) {
    return guarded(-1, [&] { return batched_solver_stream_record(solver_of(h, "hprlp_batched_solver_stream_record"), slot, event_in, event_out); });
}

extern "C" int hprlp_batched_solver_stream_info(hprlp_batched_solver *h, long out[8]) {
    return guarded(-1, [&] {
        batched_solver_stream_info(solver_of(h, "hprlp_batched_solver_stream_info", out, "output"), out, nullptr);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_stream_seconds(hprlp_batched_solver *h, double out[2]) {
    return guarded(-1, [&] {
        long counts[8];
        batched_solver_stream_info(solver_of(h, "hprlp_batched_solver_stream_seconds", out, "output"), counts, out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_lambda(hprlp_batched_solver *h, double out[2]) {
    return guarded(-1, [&] {
        batched_solver_lambda(solver_of(h, "hprlp_batched_solver_lambda", out, "output"), out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_solve_device(hprlp_batched_solver *h, int batch_size, const double *dC, const double *dAL,
                                                 const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *dX0, const double *dY0, int carry,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                                 double *dx, double *dy, double *dz, hprlp_batched_scalars *out) {
    return guarded(-1, [&] {
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve_device");
        if (!out) throw std::runtime_error("hprlp_batched_solver_solve_device: null scalars");
        resident_solve_device(s, std::max(batch_size, 0), det, certs, stream, dx, dy, dz, out,
                              [&](const Detection *d, std::vector<Certificate> *k, DeviceBatch *db) {
                                  batched_solver_solve_device(s, batch_size, dC, dAL, dAU, dl, du, obj_constants, param, dX0, dY0, carry != 0, d, k, db);
                              });
        return 0;
    });
}

// ---- device-resident streams (DESIGN.md "Device-resident streams") -----------------------------------------------------------------
// As the host stream: what the arguments alone tell is refused first, with its words, and needs no solver.
extern "C" int hprlp_batched_solver_solve_stream_device(hprlp_batched_solver *h, int count, int width, const double *dC, const double *dAL,
                                                        const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                                        const HPRLP_parameters *param, const double *dX0, const double *dY0,
                                                        const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                                        double *dx, double *dy, double *dz, hprlp_batched_scalars *out) {
    return guarded(-1, [&] {
        stream_check_call(out && dx && dy && dz, count, width, dC && dAL && dAU && dl && du, param ? param->max_iter : 0,
                          param ? param->check_iter : 1);
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve_stream_device");
        resident_solve_device(s, count, det, certs, stream, dx, dy, dz, out,
                              [&](const Detection *d, std::vector<Certificate> *k, DeviceBatch *db) {
                                  batched_solver_solve_stream_device(s, count, width, dC, dAL, dAU, dl, du, obj_constants, param, dX0, dY0, d, k, db);
                              });
        return 0;
    });
}

// ---- streams with parents (DESIGN.md "Streamed batches", "Parents") --------------------------------------------------------------
// Beside their twins: the twins' refusals first, then a NULL parent and the pairing of X0 / Y0, all before the solver is looked at;
// the parent array's values are refused by the solver, before it changes (stream_schedule.h: stream_check_parents_call).
extern "C" int hprlp_batched_solver_solve_stream_parents(hprlp_batched_solver *h, int count, int width, const double *C, const double *AL,
                                                         const double *AU, const double *l, const double *u, const double *obj_constants,
                                                         const HPRLP_parameters *param, const double *X0, const double *Y0,
                                                         const int *parent, const hprlp_detection *det, hprlp_batched_certificates *certs,
                                                         HPRLP_batched_results *out) {
    return guarded(-1, [&] {
        stream_check_call(out != nullptr, count, width, C && AL && AU && l && u, param ? param->max_iter : 0, param ? param->check_iter : 1);
        stream_check_parents_call(parent, X0 != nullptr, Y0 != nullptr);
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve_stream_parents");
        HPRLP_batched_results r;
        resident_solve(s, count, nullptr, nullptr, det, certs, [&](const Detection *d, std::vector<Certificate> *k) {
            batched_solver_solve_stream_parents(s, count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, parent, d, k, &r, nullptr);
        }, [&] { free_batched_results(&r); });
        *out = r;
        return 0;
    });
}

extern "C" int hprlp_batched_solver_solve_stream_parents_device(hprlp_batched_solver *h, int count, int width, const double *dC,
                                                                const double *dAL, const double *dAU, const double *dl, const double *du,
                                                                const double *obj_constants, const HPRLP_parameters *param,
                                                                const double *dX0, const double *dY0, const int *parent,
                                                                const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                                                double *dx, double *dy, double *dz, hprlp_batched_scalars *out) {
    return guarded(-1, [&] {
        stream_check_call(out && dx && dy && dz, count, width, dC && dAL && dAU && dl && du, param ? param->max_iter : 0,
                          param ? param->check_iter : 1);
        stream_check_parents_call(parent, dX0 != nullptr, dY0 != nullptr);
        BatchedSolver *s = solver_of(h, "hprlp_batched_solver_solve_stream_parents_device");
        resident_solve_device(s, count, det, certs, stream, dx, dy, dz, out,
                              [&](const Detection *d, std::vector<Certificate> *k, DeviceBatch *db) {
                                  batched_solver_solve_stream_parents(s, count, width, dC, dAL, dAU, dl, du, obj_constants, param, dX0, dY0,
                                                                      parent, d, k, nullptr, db);
                              });
        return 0;
    });
}

extern "C" int hprlp_batched_solver_stream_parents_info(hprlp_batched_solver *h, long out[4]) {
    return guarded(-1, [&] {
        batched_solver_stream_parents_info(solver_of(h, "hprlp_batched_solver_stream_parents_info", out, "output"), out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_stream_memory(hprlp_batched_solver *h, long out[4]) {
    return guarded(-1, [&] {
        batched_solver_stream_memory(solver_of(h, "hprlp_batched_solver_stream_memory", out, "output"), out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_set_norms(hprlp_batched_solver *h, int rule) {
    return guarded(-1, [&] {
        batched_solver_set_norms(solver_of(h, "hprlp_batched_solver_set_norms"), rule);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_scalars(hprlp_batched_solver *h, double *out) {
    return guarded(-1, [&] { return batched_solver_scalars(solver_of(h, "hprlp_batched_solver_scalars", out, "output"), out); });
}

extern "C" int hprlp_batched_solver_transfer(hprlp_batched_solver *h, long out[4]) {
    return guarded(-1, [&] {
        batched_solver_transfer(solver_of(h, "hprlp_batched_solver_transfer", out, "output"), out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_info(hprlp_batched_solver *h, long out[8]) {
    return guarded(-1, [&] {
        batched_solver_info(solver_of(h, "hprlp_batched_solver_info", out, "output"), out);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_seconds(hprlp_batched_solver *h, double out[6]) {
    return guarded(-1, [&] {
        batched_solver_seconds(solver_of(h, "hprlp_batched_solver_seconds", out, "output"), out);
        return 0;
    });
}

// One ray test outside the loop on the resident batched solver, and its panels by name (batched.hip: batched_solver_ray_step)
extern "C" int hprlp_batched_solver_ray_step(hprlp_batched_solver *h, const int *active, int restart, double *out, int *tested) {
    return guarded(-1, [&] { return batched_solver_ray_step(solver_of(h, "hprlp_batched_solver_ray_step"), active, restart != 0, out, tested); });
}

extern "C" long hprlp_batched_solver_get_panel(hprlp_batched_solver *h, const char *name, double *out, long len) {
    return guarded(-1L, [&] { return batched_solver_get_panel(solver_of(h, "hprlp_batched_solver_get_panel"), name, out, len); });
}

extern "C" int hprlp_batched_solver_set_panel(hprlp_batched_solver *h, const char *name, const double *in, long len) {
    return guarded(-1, [&] {
        batched_solver_set_panel(solver_of(h, "hprlp_batched_solver_set_panel"), name, in, len);
        return 0;
    });
}

extern "C" int hprlp_batched_solver_set_matrix_values(hprlp_batched_solver *h, const double *val, long nnz) {
    return guarded(-1, [&] {
        batched_solver_set_matrix_values(solver_of(h, "hprlp_batched_solver_set_matrix_values"), val, nnz);
        return 0;
    });
}

// ---- host only: what solve_batched does to a batch's vectors before anything is uploaded (batch_prep.h), on plain arrays ------
extern "C" int hprlp_batched_prepare_host(int m, int n, int B, const double *rn, const double *cn, const double *C, const double *AL,
                                          const double *AU, const double *l, const double *u, const double *X0, const double *Y0,
                                          int use_bc_scaling, hprlp_batched_prepared *out) {
    return hprlp_batched_prepare_host_rule(m, n, B, rn, cn, C, AL, AU, l, u, X0, Y0, use_bc_scaling, kNormRuleReference, out);
}

extern "C" int hprlp_batched_prepare_host_rule(int m, int n, int B, const double *rn, const double *cn, const double *C,
                                               const double *AL, const double *AU, const double *l, const double *u, const double *X0,
                                               const double *Y0, int use_bc_scaling, int norm_rule, hprlp_batched_prepared *out) {
    return guarded(-1, [&] {
        if (m <= 0 || n <= 0 || B <= 0 || !rn || !cn || !C || !AL || !AU || !l || !u || !out) throw std::runtime_error("bad arguments");
        const BatchData d = prepare_batch(m, n, B, C, AL, AU, l, u, nullptr, 0.0, rn, cn, use_bc_scaling != 0, norm_rule);
        const size_t nB = static_cast<size_t>(n) * B, mB = static_cast<size_t>(m) * B;
        auto give = [](const std::vector<double> &v, double *dst) {
            if (dst) std::copy(v.begin(), v.end(), dst);
        };
        give(d.C, out->C); give(d.AL, out->AL); give(d.AU, out->AU); give(d.L, out->l); give(d.U, out->u);
        const std::vector<double> *scalars[7] = {&d.b_scale, &d.c_scale, &d.norm_b, &d.norm_c, &d.norm_b_org, &d.norm_c_org, &d.sigma};
        for (int i = 0; i < 7 && out->scalars; ++i) give(*scalars[i], out->scalars + static_cast<size_t>(i) * B);
        // a start into scaled units, and from there back as a solution goes
        auto there_and_back = [B](const double *v0, size_t len, int rows, const double *norm, const std::vector<double> &scale,
                                  double *scaled, double *back) {
            if (!v0) return;
            std::vector<double> v(v0, v0 + len);
            start_to_scaled(v.data(), rows, B, norm, scale);
            if (scaled) std::copy(v.begin(), v.end(), scaled);
            point_to_caller(v.data(), rows, B, norm, scale);
            if (back) std::copy(v.begin(), v.end(), back);
        };
        there_and_back(X0, nB, n, cn, d.b_scale, out->X0, out->X_back);
        there_and_back(Y0, mB, m, rn, d.c_scale, out->Y0, out->Y_back);
        if (out->z_back) {  // z = (Z * cn) * c_scale of the scaled C
            give(d.C, out->z_back);
            reduced_cost_to_caller(out->z_back, n, B, cn, d.c_scale);
        }
        out->Bp = padded_batch(B);
        out->Bc = choose_chunk(m, n, out->Bp);
        const Geo geo = make_geo(out->Bp, out->Bc);
        std::vector<double> panel;
        to_panel(d.C, n, B, geo, out->pad, panel);
        give(panel, out->panel);
        if (out->panel_back) from_panel(panel, n, B, geo, out->panel_back);
        for (int k = 0; k < B && out->panel_index; ++k)
            for (int i = 0; i < n; ++i) out->panel_index[static_cast<size_t>(k) * n + i] = static_cast<long>(panel_index(geo, n, i, k));
        return 0;
    });
}
