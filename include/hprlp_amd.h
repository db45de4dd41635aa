/*
 * hprlp_amd.h -- step-level C ABI of the MI355X HPR-LP library (extension of HPRLP.h).
 *
 * The reference exposes its solver phases only as C++-linkage functions on a CUDA workspace struct
 * (reference include/preprocess.h, scaling.h, power_iteration.h, main_iterate.h).  These entry
 * points expose the same phases over an opaque handle with plain pointers and sizes, so that the
 * parity tests, bench.py and a multi-GPU launcher can drive them from any language.  Each function
 * cites the reference function it stands for.  All functions return 0 / a valid value on success
 * and a negative value (or NULL) on failure with the message available from hprlp_last_error();
 * none throws across the boundary.
 */
#ifndef HPRLP_AMD_H
#define HPRLP_AMD_H

#include "HPRLP.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hprlp_solver hprlp_solver; /* opaque: device-resident scaled LP + iteration state */

/* One row per residual evaluation = one line of the reference's iteration log (src/HPRLP.cu:207-218). */
typedef struct hprlp_trace_row {
    int iter, restart_flag;
    double err_Rp, err_Rd, primal_obj, dual_obj, gap, kkt, sigma, current_gap, lambda_max;
} hprlp_trace_row;

const char *hprlp_last_error(void);
const char *hprlp_backend(void); /* "hip-gfx950" */
/* Warm-up: start the HIP runtime, create the device context and a first stream and load the library's code objects NOW instead
 * of inside the first solve of the process (0.10 s there against a 0.04 s solve of a Netlib-scale LP, profiles/r04_cold_start.txt).
 * For callers that serve many solves: call once at start-up.  Returns 0; -1 without a usable GPU or for a device
 * outside [0, device count); -2 when a code object did not load (hprlp_last_error() says which).
 * hprlp_warmup_seconds: {runtime start-up, device context + first stream, code objects, total} of the last call. */
int hprlp_warmup(int device);
int hprlp_warmup_seconds(double out[4]);

/* The library keeps freed device blocks of 1 MiB and more for its next solver (a hipMalloc of a multi-GB set-up temporary right
 * behind a large hipFree stalls for up to a second on this platform); this returns them all to the driver.  HPRLP_NO_ALLOC_CACHE=1
 * disables the cache. */
void hprlp_release_device_cache(void);
/* Bookkeeping self-test of that cache without a GPU (blocks are filed under the device that owns them, the cap is per
 * device): 0 = passed, else the number of the failed check. */
int hprlp_alloc_cache_selftest(void);

/* copy_lpinfo_to_device + allocate_memory (reference src/preprocess.cu:66-256): uploads A, builds A^T
 * and the wave row-block descriptors, allocates the work vectors.  Does not scale. */
hprlp_solver *hprlp_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param);
void hprlp_solver_destroy(hprlp_solver *s);
void hprlp_solver_set_verbose(hprlp_solver *s, int verbose);

/* scaling() (reference src/scaling.cu:88-216) */
int hprlp_solver_scale(hprlp_solver *s);
/* power_method_cusparse() (reference src/power_iteration.cu:20-119); returns lambda (not x1.01) */
double hprlp_solver_power_iteration(hprlp_solver *s, int max_iter, double tol, int *iters_out);
/* sigma_0, Halpern reset (reference src/HPRLP.cu:154-167).  sigma<=0: norm_b/norm_c rule. */
int hprlp_solver_init(hprlp_solver *s, double sigma, double lambda_max);
/* All iterates and work vectors back to zero -- the state after create + scale + power iteration (the reference starts every
 * solve from zero vectors, src/preprocess.cu:41-101 allocate_memory); follow with hprlp_solver_init.  Collective-free. */
int hprlp_solver_reset_iterates(hprlp_solver *s);
/* `normal` normal iterations then, if then_check, one check-variant iteration
 * (reference update_zx_*_gpu + update_y_*_gpu, src/main_iterate.cu:422-481) */
int hprlp_solver_iterate(hprlp_solver *s, int normal, int then_check);
/* compute_residuals() (reference src/main_iterate.cu:229-309):
 * out = {err_Rp, err_Rd, primal_obj, dual_obj, rel_gap, kkt, weighted_norm (if compute_gap), lambda_max} */
int hprlp_solver_residuals(hprlp_solver *s, int iter, int compute_gap, double out[8]);
/* update_sigma + do_restart as if check_restart had raised a flag (reference main_iterate.cu:312-404);
 * in = {current_gap, best_gap, best_sigma, err_Rd, err_Rp, rel_gap}; returns new sigma in *sigma_out */
int hprlp_solver_restart(hprlp_solver *s, const double in[6], double *sigma_out);
/* compute_weighted_norm() (reference main_iterate.cu:486-515) */
double hprlp_solver_weighted_norm(hprlp_solver *s);
/* the whole loop from the current state (reference src/HPRLP.cu:154-310) + collect_solution */
int hprlp_solver_run(hprlp_solver *s, HPRLP_results *out, hprlp_trace_row *trace, int max_trace, int *n_trace);

/* ---- infeasibility detection (opt-in, one GPU; DESIGN.md "Infeasibility and unboundedness") ------------------------------
 * At every periodic evaluation (iter % check_iter == 0, iter > 0) the differences of the projected iterates since the previous
 * one, d = x_bar - x_bar' and y = y_bar - y_bar', are put to the Farkas ratio tests in the caller's units:
 *   primal infeasible: D(y) > 0 and V(y) <= eps_primal_infeasible * D(y), with z = -A^T y,
 *     D = sum_{y_i>0} AL_i y_i + sum_{y_i<0} AU_i y_i + sum_{z_j>0} l_j z_j + sum_{z_j<0} u_j z_j (finite bounds only),
 *     V = the largest multiplier whose bound is infinite;
 *   dual infeasible: c'd < 0 and W(d) <= eps_dual_infeasible * (-c'd), W = the largest step of Ad or d out of a finite bound.
 * A verdict ends the solve with status "PRIMAL_INFEASIBLE" / "DUAL_INFEASIBLE" (OPTIMAL takes precedence, both take precedence
 * over ITER_LIMIT / TIME_LIMIT); x, y, z of the result are the last iterate.  PDLP's tolerance 1e-8 is a good default. */
typedef struct hprlp_detection {
    double eps_primal_infeasible, eps_dual_infeasible;
} hprlp_detection;
/* kind 0: no verdict; 1: primal infeasible, y (m) and z = -A^T y (n); 2: dual infeasible, d (n).  The ray is scaled to infinity
 * norm 1; objective = D(y) resp. c'd of it, violation = V(y) resp. W(d).  iter: the evaluation that found it.  y, z, d are
 * malloc'd (NULL where the kind does not use them): release with hprlp_free_certificate. */
typedef struct hprlp_certificate {
    int kind;
    int iter, m, n;
    double objective, violation;
    double *y, *z, *d;
} hprlp_certificate;
/* solve() with detection.  det == NULL: exactly solve().  cert (may be NULL) always gets m, n of `model` and kind 0 unless a
 * verdict was reached.  With use_presolve and a reduced model whose solve ends in a verdict, the original model is solved
 * again with detection within the remaining time and iteration limits: a certificate always refers to the model passed. */
HPRLP_results hprlp_solve_detect(const LP_info_cpu *model, const HPRLP_parameters *param, const hprlp_detection *det,
                                 hprlp_certificate *cert);
void hprlp_free_certificate(hprlp_certificate *cert);
/* detection for the following hprlp_solver_run calls (NULL: off).  -1 + hprlp_last_error() for a sharded solver
 * (hprlp_solver_create_dist*, hprlp_solver_create_local*). */
int hprlp_solver_set_detection(hprlp_solver *s, const hprlp_detection *det);
/* the certificate of the last hprlp_solver_run (kind 0 without a verdict) */
int hprlp_solver_get_certificate(hprlp_solver *s, hprlp_certificate *cert);
/* One ray test on the current x_bar / y_bar, as a periodic evaluation of hprlp_solver_run enqueues it (after the residual
 * kernels, its scalars on the same fetch).  restart != 0 forgets the stored iterate first.  Returns 1: tested, out = the raw
 * sums and maxima {D rows, c'd, V rows, W columns, |y|_inf, |d|_inf, D columns, V columns, W rows} (D = out[0] + out[6],
 * V = max(out[2], out[7]), W = max(out[3], out[8])); 0: only the iterate was stored (the first call after a restart), out
 * untouched; -1 + hprlp_last_error(), a sharded solver among the errors.  The detection setting of later hprlp_solver_run calls
 * stays as it was.  After the first call the vectors "ray_d", "ray_prev_x" (n) and "ray_y", "ray_prev_y" (m) can be read with
 * hprlp_solver_get_vector (scaled units). */
int hprlp_solver_ray_step(hprlp_solver *s, int restart, double out[9]);

/* ---- the same detection for solve_batched (DESIGN.md "Batched detection") ----------------------------------------------------
 * The tests above, member by member in that member's units, at the same evaluations.  A member with a verdict is frozen as an
 * OPTIMAL one is: status "PRIMAL_INFEASIBLE" / "DUAL_INFEASIBLE", iter = the verdict's evaluation, x, y, z its last iterate; the
 * batch ends when the last member has a status.  Per-member precedence: OPTIMAL, the two verdicts, then the limits.
 * Arrays are malloc'd and column-major; a member's columns are zero wherever its kind does not use them.  kind, iter, objective
 * and violation have batch_size entries; y (m x batch_size) and z (n x batch_size) are NULL unless some member has kind 1, d
 * (n x batch_size) unless some member has kind 2.  Release with hprlp_free_batched_certificates. */
typedef struct hprlp_batched_certificates {
    int batch_size, m, n;
    int *kind;         /* 0 none, 1 primal infeasible, 2 dual infeasible */
    int *iter;         /* the evaluation that found it (0 for kind 0) */
    double *objective; /* D(y) resp. c'd of the normalised ray */
    double *violation; /* V(y) resp. W(d) */
    double *y, *z;
    double *d;
} hprlp_batched_certificates;
/* solve_batched() with detection.  det == NULL: exactly solve_batched() (same bits, same statuses).  certs (may be NULL) always
 * gets batch_size, m, n and kind 0 for every member unless that member reached a verdict.  A negative eps is an error. */
HPRLP_batched_results hprlp_solve_batched_detect(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                                 const double *AU, const double *l, const double *u, const double *obj_constants,
                                                 const HPRLP_parameters *param, const hprlp_detection *det,
                                                 hprlp_batched_certificates *certs);
void hprlp_free_batched_certificates(hprlp_batched_certificates *certs);

/* ---- warm start (DESIGN.md "Warm start") ----------------------------------------------------------------------------------
 * A start is x0 (length model->n) and / or y0 (length model->m) in the caller's units and numbering -- the dimensions of
 * HPRLP_results.x / .y; NULL means zeros, a non-finite entry is an error.  It is projected (x0 clamped into [l, u]; y0 onto the
 * sign its row's sides allow: y_i > 0 means the row sits at AL) and becomes the first iterate and the Halpern anchor.  The
 * iteration-0 evaluation is the KKT error of the start itself, with z the dual completion of y0 (z_j = (c - A^T y0)_j where its
 * sign has a finite bound of column j to lean on, else 0): a start that meets stop_tol ends OPTIMAL at iteration 0.  With
 * use_presolve the start is carried into the reduced model by hprlp_presolve_forward.  Sharded solvers refuse a start. */
/* hprlp_solve_detect from a start.  x0 == y0 == NULL: exactly hprlp_solve_detect (and so exactly solve() with det == NULL). */
HPRLP_results hprlp_solve_warm(const LP_info_cpu *model, const HPRLP_parameters *param, const double *x0, const double *y0,
                               const hprlp_detection *det, hprlp_certificate *cert);
/* solve_batched() / hprlp_solve_batched_detect() from per-member starts: X0 is n x B and Y0 is m x B, column-major like C, each
 * member's in its own units (either may be NULL: zeros).  Each member is projected, seeded and evaluated at iteration 0; a member
 * that meets stop_tol there ends OPTIMAL with iter 0, the others iterate as before.  X0 == Y0 == NULL: exactly
 * hprlp_solve_batched_detect (and so exactly solve_batched() with det == NULL). */
HPRLP_batched_results hprlp_solve_batched_warm(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                               const double *AU, const double *l, const double *u, const double *obj_constants,
                                               const HPRLP_parameters *param, const double *X0, const double *Y0,
                                               const hprlp_detection *det, hprlp_batched_certificates *certs);

/* ---- resident batches: a sequence of batches over one matrix (DESIGN.md "Resident batches") ---------------------------------
 * What solve_batched() redoes at every call although only the batch has changed -- the shared matrix' set-up and scaling, the
 * power iteration, the launch-order tables, the panels' allocation, the graph captures -- stays with the handle. */
typedef struct hprlp_batched_solver hprlp_batched_solver; /* opaque */

/* set-up of the shared matrix exactly as solve_batched does it (zero vectors, b/c scaling off, no reordering, no presolve),
 * scale(), row_norm / col_norm to the host, lambda_max = 1.01 x power iteration (test hook HPRLP_BATCH_LAMBDA is read HERE).
 * NULL + hprlp_last_error() on failure (no GPU included). */
hprlp_batched_solver *hprlp_batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param);
void hprlp_batched_solver_destroy(hprlp_batched_solver *h);

/* One batch.  Arguments as hprlp_solve_batched_warm.  param (NULL: create's) supplies max_iter, stop_tol, time_limit, check_iter
 * and use_bc_scaling only.  carry != 0: every member starts from the PREVIOUS batch's solution of the same member, taken from
 * the panels still on the device (needs X0 == Y0 == NULL, a previous successful solve on this handle, and the same batch_size;
 * refused when that solution holds a non-finite value).  The results equal those of a fresh hprlp_solve_batched_warm call with
 * the same arguments (carry: with X0 / Y0 = the previous results' x / y) bit for bit, whatever the handle has solved before.
 * out->setup_time is this call's preparation, out->solve_time its loop, out->power_time 0, out->time their sum.
 * 0, or -1 + hprlp_last_error() with the handle unchanged and still usable. */
int hprlp_batched_solver_solve(hprlp_batched_solver *h, int batch_size, const double *C, const double *AL, const double *AU,
                               const double *l, const double *u, const double *obj_constants, const HPRLP_parameters *param,
                               const double *X0, const double *Y0, int carry, const hprlp_detection *det,
                               hprlp_batched_certificates *certs, HPRLP_batched_results *out);

/* out = {m, n, solves so far, Bp, Bc of the last solve, graph captures in total, graphs alive,
 *        panel (re)allocations in total} */
int hprlp_batched_solver_info(hprlp_batched_solver *h, long out[8]);

/* seconds: {create: set-up + scaling, create: power iteration,
 *           last solve: host prep, staging upload + panel kernels + start, loop, results' way back} */
int hprlp_batched_solver_seconds(hprlp_batched_solver *h, double out[6]);

/* ---- streamed batches: refill finished slots from a queue of LPs (DESIGN.md "Streamed batches") --------------------------------
 * count problems over the handle's matrix through `width` slots.  C, l, u: n x count; AL, AU: m x count; X0 / Y0 as in
 * hprlp_batched_solver_solve (either NULL), all column-major, host memory.  out: an HPRLP_batched_results of `count` members
 * (free_batched_results), certs as hprlp_solve_batched_detect's with batch_size = count.
 *
 * The panel geometry is that of a plain solve of min(width, count) members; slots 0 .. min(width, count)-1 take problems 0, 1, ...
 * At every multiple of check_iter every occupied slot is evaluated by its member's LOCAL iteration (the loop's iteration minus
 * check_iter x event_in); a member that received a status is taken out before its slot is touched; the freed slots, ascending,
 * take the queued problems, ascending, and the new members get their iteration-0 evaluation within the same event (one that
 * ends there hands its slot on at once).  For a problem that sat in slot k, status, iter, x, y, z, primal_obj, residuals, gap and
 * certificate are bit for bit those of a plain hprlp_batched_solver_solve of min(width, count) members whose slot k holds it,
 * provided neither call raised lambda_max (hprlp_batched_solver_stream_info, hprlp_batched_solver_lambda); with count <= width
 * the call is exactly the plain solve.  lambda_max is shared: a raise applies to every member in flight and to every later one of
 * the call; the next call starts from the created value.
 *
 * max_iter is each member's own; time_limit is the call's: at the limit the running members get TIME_LIMIT with their local iter,
 * the queued ones TIME_LIMIT, iter 0, zero vectors and event_in -1.  Refused with -1 + hprlp_last_error() before anything
 * changes: a non-positive count or width, NULL vectors, a non-finite start, and a max_iter that is not a multiple of check_iter
 * (every member's last event has to be a periodic event of the loop).  There is no carry; the device entry is
 * hprlp_batched_solver_solve_stream_device below.  After a stream
 * call, carry, hprlp_batched_solver_ray_step and the panels by name are refused until the next plain solve, which gives the bits
 * of a handle that never streamed.
 *
 * Device memory of a call beside the workspace of min(width, count) members: the staged queue, (3 n + 2 m) x count doubles (plus
 * n x count / m x count for X0 / Y0) and 3 x count scalars, and the result block, (2 n + m) x count doubles (twice that with
 * detection); one pinned host block of the larger of the two.  Host memory beside it: the scaled queue once more while the call
 * runs, and the returned results. */
int hprlp_batched_solver_solve_stream(hprlp_batched_solver *h, int count, int width, const double *C, const double *AL,
                                      const double *AU, const double *l, const double *u, const double *obj_constants,
                                      const HPRLP_parameters *param, const double *X0, const double *Y0, const hprlp_detection *det,
                                      hprlp_batched_certificates *certs, HPRLP_batched_results *out);
/* per problem of the last stream call (count entries each): slot, the evaluation at which it entered and left (global loop
 * iteration / check_iter; event_in -1: never started, then slot and event_out are -1 too).  Returns count, or -1. */
int hprlp_batched_solver_stream_record(hprlp_batched_solver *h, int *slot, int *event_in, int *event_out);
/* {count, width, loop iterations of the call, evaluations, evaluations at which a slot was refilled, refills (entries after the
 *  initial fill), iteration-0 evaluation passes added for refills (cascades included), lambda bumps} */
int hprlp_batched_solver_stream_info(hprlp_batched_solver *h, long out[8]);
/* wall seconds of the last stream call's loop: {its refill passes (harvest, refill, the new members' evaluation), the rest} */
int hprlp_batched_solver_stream_seconds(hprlp_batched_solver *h, double out[2]);
/* {lambda_max as created, lambda_max at the end of the last successful call of either kind (the created one before any)} */
int hprlp_batched_solver_lambda(hprlp_batched_solver *h, double out[2]);
/* host only, no GPU: the schedule the loop follows, from each problem's length in evaluations (iter / check_iter; 0: it ends at
 * its iteration-0 evaluation).  slot / event_in / event_out: count entries each.  Returns the makespan in evaluations (the
 * largest event_out), or -1 + hprlp_last_error() (a non-positive count or width, a NULL array, a negative length). */
int hprlp_stream_schedule_host(int count, int width, const int *events, int *slot, int *event_in, int *event_out);

/* ---- device-resident batches: tensors in, tensors out (DESIGN.md "Device-resident batches") ------------------------------------
 * hprlp_batched_solver_solve with the batch's vectors already in device memory and the solution wanted there.  dC, dl, du
 * (n x B), dAL, dAU (m x B), dX0 (n x B) / dY0 (m x B; either may be NULL) are DEVICE arrays, column-major like the host entry's;
 * dx, dz (n x B) and dy (m x B) are device buffers that receive the solution in the caller's units.  obj_constants (B or NULL),
 * param, det, certs and `out` are host memory.  The per-member scaling and its norms run in kernels, the results are written
 * straight into dx / dy / dz, and only the per-member scalars cross the bus.
 *   Pointers: before anything is launched every device pointer is looked up with hipPointerGetAttributes.  It passes only as
 * device memory of the handle's device and, where the runtime reports the allocation's range, with room for rows * B doubles;
 * a host address, another device's memory, a short buffer or an address the runtime does not know is refused.
 *   Ordering: `stream` is the hipStream_t (NULL: the default stream) on which the inputs were produced; the solver's own stream
 * waits for an event recorded on it before its first read, and the call returns after its own stream has drained: the outputs
 * are complete on return.
 *   Bits: the norms follow the "tree" rule (norm rule 1), whose order of additions is fixed by the vector's length alone; with
 * hprlp_batched_solver_set_norms(h, 1) the host entry follows it too, and the two entries then agree bit for bit.  carry,
 * detection and param behave as in hprlp_batched_solver_solve, and the two entries may alternate on one handle, carry included.
 * A non-finite entry of dX0 / dY0 is refused after the scaling kernels, before the loop.
 * 0, or -1 + hprlp_last_error() with the handle as it was and still usable. */
typedef struct hprlp_batched_scalars { /* host; the arrays are the caller's (NULL: not wanted) */
    double *primal_obj, *residuals, *gap; /* B each */
    int *iter;                            /* B */
    char *status;                         /* 64 x B */
    double time, setup_time, solve_time, power_time; /* out, as in HPRLP_batched_results */
} hprlp_batched_scalars;
int hprlp_batched_solver_solve_device(hprlp_batched_solver *h, int batch_size, const double *dC, const double *dAL, const double *dAU,
                                      const double *dl, const double *du, const double *obj_constants, const HPRLP_parameters *param,
                                      const double *dX0, const double *dY0, int carry, const hprlp_detection *det,
                                      hprlp_batched_certificates *certs, void *stream, double *dx, double *dy, double *dz,
                                      hprlp_batched_scalars *out);
/* ---- device-resident streams: a queue in device memory (DESIGN.md "Device-resident streams") ----------------------------------
 * hprlp_batched_solver_solve_stream with the queue already in device memory and the solutions wanted there.  dC, dl, du, dX0,
 * dx, dz are n x count and dAL, dAU, dY0, dy are m x count, column-major DEVICE arrays like hprlp_batched_solver_solve_device's
 * with `count` in place of B (dX0 / dY0 may be NULL); obj_constants (count or NULL), param, det, certs and `out` (arrays of
 * `count`) are host memory.
 *   Rule: the host stream's, word for word -- slots, events, local iteration numbers, limits, and what a later call may do (carry,
 * hprlp_batched_solver_ray_step and the panels by name are refused until the next plain solve).  _stream_record, _stream_info,
 * _stream_seconds, _lambda, _transfer and _scalars report on this call as on its host twin.
 *   No copy of the queue: the per-problem norms are taken from the caller's arrays where they lie, a problem is scaled in the
 * launch that puts it into its slot, and x, y, z of a harvested problem go straight into column p of dx, dy, dz (zeroed at entry
 * on the solver's stream: a problem that never started has zero columns).  Beside the workspace the call holds no device memory
 * that grows with n x count or m x count, except, with detection, the ray block of (2 n + m) x count doubles.  Across the bus go
 * the header of the slots, the refill passes' tables, 7 x count scalars with their flag words, the loop's scalar fetches and the
 * rays of the problems with a verdict.
 *   Pointers and ordering: hprlp_batched_solver_solve_device's.  Every device pointer is looked up with hipPointerGetAttributes
 * before anything is launched (the room checked is rows x count), the solver's stream waits for an event recorded on `stream`,
 * and the outputs are complete on return.
 *   Refusals: everything the host stream refuses, with its words, and every pointer that fails the lookup.  A non-finite entry of
 * dX0 / dY0 anywhere in the queue -- in a problem that would only enter at a refill too -- is found by the norm passes and
 * refused before any panel or control value is written.  After any refusal the handle is what it was; a carry that was valid
 * before stays valid.
 *   Bits: the norms follow the tree rule (norm rule 1).  Against the host stream on a handle with
 * hprlp_batched_solver_set_norms(h, 1) and the same arguments, every problem has the same status, iter, x, y, z, primal_obj,
 * residuals, gap and certificate bit for bit, the record and the stream_info counts (lambda bumps included) are the same; with
 * count <= width the call is hprlp_batched_solver_solve_device of `count` members.
 * 0, or -1 + hprlp_last_error(). */
int hprlp_batched_solver_solve_stream_device(hprlp_batched_solver *h, int count, int width, const double *dC, const double *dAL,
                                             const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                             const HPRLP_parameters *param, const double *dX0, const double *dY0,
                                             const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream, double *dx,
                                             double *dy, double *dz, hprlp_batched_scalars *out);
/* of the last successful stream call of either kind:
 * {device bytes the call held for queue VECTORS (host entry: the staged queue; device entry: 0),
 *  device bytes of its result / ray block, device bytes of per-problem scalars, partials and tables, pinned host bytes} */
int hprlp_batched_solver_stream_memory(hprlp_batched_solver *h, long out[4]);
/* ---- streams with parents: queued problems start from earlier ones' solutions (DESIGN.md "Streamed batches", "Parents") ---------
 * hprlp_batched_solver_solve_stream / _solve_stream_device with one more argument, parent: a HOST array of `count` ints in both
 * entries.  parent[p] == -1: problem p is a root; else 0 <= parent[p] < p, and p starts from the x, y that problem parent[p]
 * returned, whatever its status (OPTIMAL, ITER_LIMIT, a verdict's iterate) -- a rolling horizon's period t+1 from period t, a search
 * tree's node from its parent -- in ONE call, without a level waiting for its slowest member.
 *   Starts: X0 / Y0 are given together or not at all.  With them a root starts from its own columns; without them a root is a cold
 * member, bit for bit a cold plain member.  A child ignores its own columns.  A start is scaled on its way into the slot by the
 * kernel that reads it (kb_slot_start): from the parent's column of the results on the device, or the root's column of X0 / Y0.
 *   Rule: p is READY when it is a root or its parent has been harvested, in an earlier pass or in the very pass that is being
 * assigned.  In one refill pass the FREE slots -- those just harvested and those that stood empty -- in ascending order take the
 * ready problems in ascending number, as many as both last.  The initial fill is a pass of event 0 with every slot free, in which
 * only roots are ready; slots without a problem stay empty and inactive until a pass gives them one.  The geometry is a plain
 * solve's of min(width, count) members.  A member that ends at its iteration-0 evaluation frees its slot, and readies its children,
 * for the same event's next pass.  Everything else -- events, local iteration numbers, limits, the record, what a later call may
 * do -- is the stream's.
 *   Never entered: once the time is up nothing enters, and a problem that never entered is TIME_LIMIT, iter 0, zero vectors,
 * event_in -1.  Where a parent's final residuals, primal_obj or gap is not finite, its children do not enter: they and their
 * descendants are ERROR, iter 0, zero vectors, event_in -1.
 *   Bits: for problem p in slot k, status, iter, x, y, z, primal_obj, residuals, gap and certificate are those of a plain solve of
 * min(width, count) members whose slot k holds p -- cold for a cold root, else warm with X0[:, k], Y0[:, k] equal to the returned
 * x, y of p's parent (a started root: its own columns) -- provided neither call raised lambda_max.  With parent all -1 the results
 * and the record are those of the twin without parents.
 *   Refused with -1 + hprlp_last_error() before anything changes: everything the twin refuses, a NULL parent, one of X0 / Y0 without
 * the other, and a parent[p] outside -1 .. p-1 (the message names p and the value; no device call is made for it). */
int hprlp_batched_solver_solve_stream_parents(hprlp_batched_solver *h, int count, int width, const double *C, const double *AL,
                                              const double *AU, const double *l, const double *u, const double *obj_constants,
                                              const HPRLP_parameters *param, const double *X0, const double *Y0, const int *parent,
                                              const hprlp_detection *det, hprlp_batched_certificates *certs, HPRLP_batched_results *out);
/* the device twin: hprlp_batched_solver_solve_stream_device's arguments plus parent (host).  A child's start is read from the
 * caller's dx, dy, where its parent's harvest wrote it on the solver's stream; nothing of a start crosses the bus. */
int hprlp_batched_solver_solve_stream_parents_device(hprlp_batched_solver *h, int count, int width, const double *dC, const double *dAL,
                                                     const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                                     const HPRLP_parameters *param, const double *dX0, const double *dY0,
                                                     const int *parent, const hprlp_detection *det, hprlp_batched_certificates *certs,
                                                     void *stream, double *dx, double *dy, double *dz, hprlp_batched_scalars *out);
/* of the last stream call, which was one with parents (else -1): {roots that entered, cold members among them, children that
 * entered, slot-events: summed over the loop's evaluations after which it went on, the slots that stood empty while a problem was
 * still waiting for its parent} */
int hprlp_batched_solver_stream_parents_info(hprlp_batched_solver *h, long out[4]);
/* host only, no GPU: hprlp_stream_schedule_host for a queue with parents (parent as above; all -1: hprlp_stream_schedule_host's
 * arrays and makespan).  -1 + hprlp_last_error() also for a NULL parent or a parent[p] outside -1 .. p-1. */
int hprlp_stream_schedule_parents_host(int count, int width, const int *events, const int *parent, int *slot, int *event_in,
                                       int *event_out);
/* The norm rule of the HOST entry of this handle: 0 = the reference's long double sums (the default), 1 = the tree rule. */
int hprlp_batched_solver_set_norms(hprlp_batched_solver *h, int rule);
/* out (7 x B): b_scale, c_scale, norm_b, norm_c, norm_b_org, norm_c_org, first sigma of the last successful solve, either entry.
 * Returns that call's B, or -1. */
int hprlp_batched_solver_scalars(hprlp_batched_solver *h, double *out);
/* out = {staging bytes host -> device, staging bytes device -> host of the last successful solve (the batch's way in and its
 *        solution's way out; the loop's scalar fetches are not counted), 1 if that solve was a device-entry call,
 *        device-entry solves so far} */
int hprlp_batched_solver_transfer(hprlp_batched_solver *h, long out[4]);
/* One ray test of the detection OUTSIDE the loop (the step-level entry the value tests use; DESIGN.md "Batched detection"), on
 * the panels the last successful solve left on the device: its B members, its panel geometry, its scales.  active (B ints):
 * the members that take part, as the loop's active mask.  restart != 0: the stored iterate and the rays are forgotten and the
 * step only stores X_bar / Y_bar of the active members (returns 0); the first step after a solve needs it.  Otherwise (returns 1):
 * rays = X_bar / Y_bar minus the stored iterate, the iterate is stored, and out receives the nine device scalars per member,
 * slot-major (out[s * B + k]) in the order DY, CD, VY, WD, YN, DN, DZ, VZ, WQ; tested[k] = 1 where member k was active (0: its
 * slots are not meaningful).  A later solve on the handle gives the bits of a handle that never stepped.
 * -1 + hprlp_last_error(): no successful solve on the handle, or no stored iterate and restart == 0. */
int hprlp_batched_solver_ray_step(hprlp_batched_solver *h, const int *active, int restart, double *out, int *tested);
/* A panel of the last successful solve by name, the first B members column-major rows x B in SCALED units: C, L, U, X_bar, ray_d,
 * ray_prev_x (n rows), AL, AU, Y_bar, ray_y, ray_prev_y (m rows) -- infinite sides and bounds read +-1e100 -- and ray_z
 * (n rows: the product A^T ray_y of the certificates, computed by the call); row_norm (m values) / col_norm (n values).  Read
 * only, for the warm start's value tests: X, X_hat, last_X, Z_bar (n rows) and Y, last_Y, Y_obj (m rows).  "raw:"
 * before a panel's name: the whole padded panel in the device's layout, rows x Bp.  out NULL: only the count.  Returns the count
 * of values (len must equal it), or -1 + hprlp_last_error() (an unknown name; a ray_* name before a detecting solve or a step). */
long hprlp_batched_solver_get_panel(hprlp_batched_solver *h, const char *name, double *out, long len);
/* X_bar or Y_bar of the first B members from column-major rows x B (scaled units); no other name can be written.  carry is
 * refused until the next successful solve.  0, or -1 + hprlp_last_error(). */
int hprlp_batched_solver_set_panel(hprlp_batched_solver *h, const char *name, const double *in, long len);
/* After hprlp_solver_init, before hprlp_solver_run: the start of the next run (caller's units; both NULL: the zero start,
 * evaluated as a start).  -1 + hprlp_last_error() for a sharded solver or a non-finite entry. */
int hprlp_solver_set_start(hprlp_solver *s, const double *x0, const double *y0);

/* ---- re-solve: a sequence of LPs over one matrix on one resident solver (one GPU; DESIGN.md "Re-solve") -----------------------
 * Everything that depends on A alone -- device set-up, kernel forms, ordering, the scaling factors, lambda_max -- is kept; the
 * vectors are scaled by the solver's cumulative row / column factors and get their own b_scale, c_scale and norms.
 *   objective group: c (n) and / or obj_constant; NULL keeps the current one bit for bit.
 *   bounds group:    AL, AU (m), l, u (n), all four or none (b_scale couples them); NULL keeps them, and the bound codes, bit for bit.
 * Caller's units and numbering, host memory; infinite entries stay infinite.  After hprlp_solver_scale.  No presolve on this
 * path: hprlp_solver_create never presolved, and a reduced model does not survive a change of c or of the bounds in general.
 * 0, or -1 + hprlp_last_error() (solver unchanged): a sharded solver, a NaN, an incomplete bounds group. */
int hprlp_solver_set_data(hprlp_solver *s, const double *c, const double *obj_constant,
                          const double *AL, const double *AU, const double *l, const double *u);
/* solve again from zero or from (x0, y0); sigma <= 0: the norm_b / norm_c rule.  lambda_max is the solver's current one.
 * Detection as set by hprlp_solver_set_detection.  Same outputs as hprlp_solver_run; out->time counts the set_data calls since
 * the previous run and this loop, and no power iteration. */
int hprlp_solver_resolve(hprlp_solver *s, double sigma, const double *x0, const double *y0, HPRLP_results *out,
                         hprlp_trace_row *trace, int max_trace, int *n_trace);
/* seconds of the last set_data: {upload, kernels + fetch, total} */
int hprlp_solver_data_seconds(hprlp_solver *s, double out[3]);

/* ---- matrix values: new coefficients on the resident sparsity pattern (DESIGN.md "Matrix values") -------------------------------
 * val: the nnz values of the model's CSR in the caller's order, i.e. at the positions of the rowPtr / colIndex the solver was
 * created from; the pattern is not passed and cannot change (a stored zero switches an entry off).  All five vectors are
 * required -- every scaled vector depends on the row and column factors, which change with A, and the solver keeps no copy in
 * the caller's units; obj_constant NULL keeps the current one.  Caller's units and numbering, host memory; infinite sides and
 * bounds are legal.  After the call the solver is, bit for bit, a fresh hprlp_solver_create on the changed model followed by
 * hprlp_solver_scale: index arrays, ordering, kernel forms, tiled layouts and captured graphs stay, the iterates are zero.  The
 * caller's next steps are those after hprlp_solver_scale: hprlp_solver_power_iteration, hprlp_solver_init, then
 * hprlp_solver_resolve, whose out->time counts this call's seconds as it counts set_data's.
 * The first call builds the solver's two value maps (internal entry -> caller's position, for A and for A^T) and keeps them: 4
 * bytes per entry each.  A solver with a locality ordering also holds the caller's index arrays on the device (4 bytes per entry)
 * from its creation until that first call.
 * 0, or -1 + hprlp_last_error() with the solver unchanged bit for bit and still usable: a NULL argument, nnz other than the
 * model's, a sharded solver (one GPU only), a solver never scaled, a NaN in a vector, a non-finite value (found on the device in
 * the staging block before anything the solver reads is written). */
int hprlp_solver_set_matrix_values(hprlp_solver *s, const double *val, long nnz, const double *c, const double *obj_constant,
                                   const double *AL, const double *AU, const double *l, const double *u);
/* the last successful call: {map construction (first call only, else 0), upload + check, value + vector kernels, scale(), total,
 *                            calls so far} */
int hprlp_solver_matrix_seconds(hprlp_solver *s, double out[6]);

/* ---- device-resident re-solve: tensors in, tensors out (one GPU; DESIGN.md "Device-resident re-solve") --------------------------
 * hprlp_solver_set_data, hprlp_solver_resolve and hprlp_solver_set_matrix_values with the vectors already in device memory and
 * the solution wanted there.  The d* arguments are DEVICE arrays in the caller's units and numbering (dc, dl, du, dx0, dx, dz: n;
 * dAL, dAU, dy0, dy: m; dval: nnz); obj_constant, out, trace and n_trace are host memory.  Semantics are those of the host
 * entries, argument for argument: the groups of set_data (dc and / or obj_constant; dAL, dAU, dl, du together or not at all), all
 * six arrays for the matrix values, sigma <= 0 for the norm rule, NULL starts for a cold re-solve; detection, trace, out->time and
 * hprlp_solver_data_seconds / hprlp_solver_matrix_seconds as there ("upload" holds the pointer checks and the device check).
 *   Results: dx, dz and dy receive the solution in the caller's units and numbering; any of the three may be NULL (not wanted).
 * out->x, out->y, out->z are NULL (hprlp_free_results stays legal), every scalar field of out is filled as by hprlp_solver_resolve.
 * dx may be the same buffer as dx0 and dy the same as dy0: the start is consumed before the loop and the results are written
 * after it -- what a loop that carries one solve's x and y into the next wants.
 *   Pointers: before anything is launched every non-NULL device pointer is looked up.  It passes only as device memory of the
 * solver's device, 8-byte aligned and, where the runtime reports the allocation's range, with room for its length; a host
 * address, another device's or managed memory, a short buffer or an address the runtime does not know is refused.
 *   Ordering: `stream` is the hipStream_t (NULL: the default stream) on which the inputs were produced; the solver's own stream
 * waits for an event recorded on it before its first read, and the call returns after its own stream has drained: the outputs
 * are complete on return.
 *   Bits: the kernels of the host entries read the caller's buffers where they read the staging block, and the results kernel
 * does the host entry's three operations in its order: a device-entry call gives the bits of the host-entry call with the same
 * numbers, and the entries may alternate on one handle.  A NaN in a vector, a non-finite value or a non-finite entry of a start
 * is found by a kernel before anything the solver reads is written.
 * 0, or -1 + hprlp_last_error() with the solver as it was, bit for bit, and still usable: what the host entries refuse (a sharded
 * solver, a solver never scaled, an incomplete bounds group, a wrong nnz, a NaN) and a pointer that does not pass. */
int hprlp_solver_set_data_device(hprlp_solver *s, const double *dc, const double *obj_constant, const double *dAL,
                                 const double *dAU, const double *dl, const double *du, void *stream);
int hprlp_solver_resolve_device(hprlp_solver *s, double sigma, const double *dx0, const double *dy0, void *stream, double *dx,
                                double *dy, double *dz, HPRLP_results *out, hprlp_trace_row *trace, int max_trace, int *n_trace);
int hprlp_solver_set_matrix_values_device(hprlp_solver *s, const double *dval, long nnz, const double *dc,
                                          const double *obj_constant, const double *dAL, const double *dAU, const double *dl,
                                          const double *du, void *stream);
/* The last successful set_data*, set_matrix_values* or resolve* call, either entry: out = {bytes of model data and solution host
 * -> device, the same device -> host, 1 if that call was a device entry, device-entry calls so far}.  Counted are the vectors,
 * the values, the starts and the solution; not counted are the loop's scalar fetches, the 8-byte check flag and the one-time
 * upload of a locality ordering's permutations.  A device entry therefore reports 0 / 0. */
int hprlp_solver_transfer(hprlp_solver *s, long out[4]);
/* the value maps as the solver built them (built now if no set_matrix_values call has): mapA[e] / mapAT[k] = the caller's CSR
 * position of entry e of A / entry k of A^T in the solver's internal numbering; cap >= nnz ints each.  Returns nnz, or -1. */
long hprlp_solver_value_maps(hprlp_solver *s, int *mapA, int *mapAT, long cap);
/* the locality ordering in place: row_new2old (m), col_new2old (n).  1: filled; 0: no ordering, arrays untouched; -1: error */
int hprlp_solver_ordering(hprlp_solver *s, int *row_new2old, int *col_new2old);
/* Test infrastructure: the power iteration's start vector as this solver forms it on the device, read back in the caller's
 * numbering (m entries; behind a locality ordering the vector is defined in the caller's numbering).  Returns m. */
int hprlp_solver_power_start(hprlp_solver *s, double *out, int cap);
/* Host only, no GPU: the rule of the maps restated.  Without an ordering (both NULL) mapA is the identity and mapAT the
 * row-stable transpose's entry permutation; with one, mapA is the entry permutation of P A Q with every row's columns ascending
 * (ties in the caller's order) and mapAT that of its row-stable transpose. */
int hprlp_value_maps_host(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                          int *mapA, int *mapAT);
/* The same for the resident batched solver: the shared matrix takes the values and is scaled again (zero vectors, b/c scaling
 * off), the norms and the created lambda_max follow (HPRLP_BATCH_LAMBDA is read here as at create); panels, staging blocks,
 * order tables and workspace stay.  The seconds are added to the create's two.  Every later call gives the bits of a fresh
 * hprlp_batched_solver_create on the changed model followed by the same call; carry is refused until the next successful solve.
 * 0, or -1 + hprlp_last_error() with the handle unchanged: NULL, a wrong nnz, a non-finite value. */
int hprlp_batched_solver_set_matrix_values(hprlp_batched_solver *h, const double *val, long nnz);

/* ---- many small LPs at once (one GPU; DESIGN.md "Many small LPs") --------------------------------------------------------------
 * A Netlib-scale LP (nnz < 12288, m, n <= 2048, rows and columns of at most 256 entries) runs as ONE workgroup and occupies one
 * compute unit of 256.  These entry points advance a group of independent solvers -- each with its own matrix -- in lock-step:
 * the normal iterations and the power iterations of all small-path members go in one launch per kernel class (workgroup b =
 * member b).  Check step, evaluation and restart go in one launch per kernel for the whole group (a workgroup runs the single
 * kernel's code as workgroup lb of lg of its member), and one copy and one host wait serve the scalars of all members: a round of
 * hprlp_solver_run_many has one wait, three if some member restarts in it, and a number of launches that does not depend on the
 * count.  The stopping test, restart rule, sigma update and detection stay the member's own host code, so every member gets the
 * bits it gets alone.  Members off the small path are legal (they issue their own launches inside the same lock-step), and a
 * member's iteration-0 evaluation (hprlp_solver_resolve_many apart) is always its own.  With detection on, the ray tests of the
 * members that join ride in the evaluation's launches (three kernels more per periodic round, whatever the count, and no wait),
 * and the certificates of a round's verdicts come back through one device block, one copy and one wait; a member outside the
 * group launches keeps its own ray test and certificate.  The group runs quietly (hprlp_solver_set_verbose is ignored).
 * All of them return 0, or -1 + hprlp_last_error(); nothing is launched when the arguments are wrong: a NULL pointer, count <= 0,
 * the same handle twice, a sharded solver (hprlp_solver_create_dist* / _local*), a solver that was never scaled, members on
 * different devices, a negative normal[k] or iter[k]. */
/* hprlp_solver_power_iteration for every member: lambda_out[k] (lambda, not lambda x 1.01), iters_out[k] (may be NULL) */
int hprlp_solver_power_iteration_many(hprlp_solver **s, int count, int max_iter, double tol, double *lambda_out, int *iters_out);
/* hprlp_solver_iterate for every member: normal[k] normal iterations of member k, then one check step each if then_check */
int hprlp_solver_iterate_many(hprlp_solver **s, int count, const int *normal, int then_check);
/* hprlp_solver_residuals for every member: iter[k], compute_gap[k] as its arguments, out[8 * k .. 8 * k + 8) as its out.  A member
 * with iter[k] = 0 (the bound violation of iteration 0) is evaluated by its own launches. */
int hprlp_solver_residuals_many(hprlp_solver **s, int count, const int *iter, const int *compute_gap, double *out /* 8 x count */);
/* hprlp_solver_restart for every member: in[6 * k .. 6 * k + 6) as its in, sigma_out[k] (may be NULL) the member's new sigma */
int hprlp_solver_restart_many(hprlp_solver **s, int count, const double *in /* 6 x count */, double *sigma_out /* count */);
/* hprlp_solver_run for every member, from its current state (detection, a start, changed data are honoured): out[k] as
 * hprlp_solver_run fills it (x, y, z malloc'd), no trace; certificates from hprlp_solver_get_certificate member by member.  A
 * finished member drops out, the call returns with the last one.  out[k].time = the member's power-iteration (or set_data) time
 * + the group loop's wall time up to the member's last event; time_limit applies to that value. */
int hprlp_solver_run_many(hprlp_solver **s, int count, HPRLP_results *out);
/* What HPRLP_main_solve does, for `count` models at once: hprlp_solver_create_many, hprlp_solver_scale_many, the power iterations
 * together (lambda x 1.01), the loop together, solutions, hprlp_solver_destroy_many.  NO presolve on this path: param->use_presolve is ignored, as in
 * solve_batched.  A model that fails its set-up gets status "ERROR" (and hprlp_last_error() names it); the others are solved. */
int hprlp_solve_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, HPRLP_results *out);
/* hprlp_solve_many with infeasibility detection on for every member (hprlp_solve_detect's twin; no presolve, as on the whole
 * path).  det == NULL: exactly hprlp_solve_many.  certs (count entries, may be NULL): certs[k] always gets the member's m and n,
 * and kind 0 unless the member reached a verdict (status PRIMAL_INFEASIBLE / DUAL_INFEASIBLE); each entry is released with
 * hprlp_free_certificate.  A member whose set-up fails keeps status "ERROR" and kind 0.  A negative eps is refused before
 * anything is created. */
int hprlp_solve_many_detect(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                            HPRLP_results *out, hprlp_certificate *certs);
/* hprlp_solver_ray_step for every member: the evaluation with the gap, then the ray test, one fetch for the whole group, through
 * the group launches for the members that join.  restart[k] as that entry's restart; tested[k] = 1 or 0 as its return value;
 * out[9 * k .. 9 * k + 9) as its out, untouched where tested[k] is 0.  The members' detection settings are not touched.  Refused
 * before anything is launched, naming the entry point and `member k`: the group rules above, NULL arrays, a first step of a
 * member without restart[k]. */
int hprlp_solver_ray_step_many(hprlp_solver **s, int count, const int *restart, double *out /* 9 x count */, int *tested /* count */);
/* Group form of creation, scaling and destruction: every member ends bit for bit the solver that hprlp_solver_create +
 * hprlp_solver_scale give it alone.  The members of a _create_many call whose set-up only allocates and uploads (Netlib-scale
 * models) share one arena -- a few device blocks, one pinned block, one stream, one copy per block -- which goes when the last
 * of them is destroyed, in any order, by either destroy call; _scale_many issues one launch per kernel kind and scaling step for
 * the members on the small path and three host waits for the whole group, every other member scales on its own inside the call.
 * Refused before anything is launched or allocated: a NULL list, count <= 0, a handle given twice, a sharded solver, members on
 * different devices. */
/* hprlp_solver_create for every model, on param->device_number; out[k] = NULL where model k failed.  Returns the number created, -1 on bad arguments. */
int  hprlp_solver_create_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, hprlp_solver **out);
/* hprlp_solver_scale for every member; handles from hprlp_solver_create are as welcome as those from _create_many */
int  hprlp_solver_scale_many(hprlp_solver **s, int count);
/* hprlp_solver_destroy for every non-NULL entry */
void hprlp_solver_destroy_many(hprlp_solver **s, int count);
/* calling thread's last create_many / scale_many / destroy_many (each fills its own slots):
 * {device allocations, pinned allocations, host-to-device copies, scaling launches, scaling host waits,
 *  members served by group scaling launches, members that scaled on their own, device frees} */
int  hprlp_last_setup_many_counts(long out[8]);
/* bookkeeping self-test of the arena, no GPU needed: 0, or the number of the failed check */
int  hprlp_arena_selftest(void);
/* Wall-clock phases [s] of the calling thread's last hprlp_solve_many: out = {set-up of the group, scaling of the group, power
 * iterations + init, loop + solutions' way back, whole call (teardown included), evaluation rounds, host waits, group launches of
 * the normal iterations (every kind: hprlp_last_run_many_counts)} */
int hprlp_last_solve_many_phases(double out[8]);
/* Counts of the calling thread's last hprlp_solver_run_many / hprlp_solve_many: out = {evaluation rounds, host waits, group
 * launches of every kind (normal iterations, check, evaluation, restart, packing of the scalars), copies of the scalars to the host,
 * operations issued for ONE member (an own evaluation, check step or restart piece; the ray test or the certificate of a member
 * outside the group launches), member-evaluations served by group launches, member ray tests served by group launches,
 * certificates collected through the group's block (a round with such a verdict adds one wait and one copy)} */
int hprlp_last_run_many_counts(long out[8]);

/* ---- wide members: solvers past the single-workgroup size iterate as a group (DESIGN.md "Many small LPs", wide members) -------
 * Off the small path (nnz >= 12 288, m or n > 2 048, a row or column longer than 256) a member of a *_many call issues its own
 * launches inside the lock-step, serialised on the group's stream.  A solver marked wide joins the group launches instead: its
 * normal iterations run in group launches of k_spmv_fused_many (two launches per iteration for all such members of a round, in
 * segments where their iteration counts differ), its regular-kernel power iteration in group launches as well (ten iterations and
 * the error terms per host wait for all of them), and check step, evaluation, restart, ray test, certificate, scaling, new data,
 * re-solve and new matrix values in the group kinds the small-path members use -- those run a member's own grid at any size.
 * Every member still gets the bits of its own solve.  Opt-in, per solver; without it every path is what it was.
 * Where it pays (profiles/many_wide_ab.txt: one MI355X, K resident solvers, 2000 iterations each, run_many with the setting on
 * against run_many without it, median of three rounds, spreads below 4 %): 2500 x 4000 with 15 000 entries: 2.9 x at K = 4,
 * 9.1 x at K = 16, 18.6 x at K = 64; 20 000 x 30 000 with 150 000 entries: 2.0 x at K = 4, 3.4 x at K = 16; 33 874 x 105 728 with
 * 230 000 entries (the largest size measured): 1.16 x at K = 2, 1.51 x at K = 4, 1.86 x at K = 8 (the largest K measured there).
 * With ONE wide member in a call the member runs its own path and nothing is gained or lost (1.00 at K = 1 on all three shapes);
 * no point was measured at which the setting loses.  The power iteration of the same groups: 1.1 x to 3.8 x.  A member with a
 * tiled copy (from 458 752 columns on, where the kernel-form rules try one) or with a row past 4096 entries cannot join. */
/* Let a solver off the small path join the group launches of the *_many entries ("wide" member).
 * on = 0 switches it off.
 * Returns 1 when the solver will join, 0 when the setting is stored but the solver cannot join, -1 + hprlp_last_error().
 * A solver cannot join when a matrix of it has a tiled copy or rows past kSplitRow (4096 entries).
 * Such a solver keeps going its own way, as today.
 * A sharded solver is refused with -1.
 * A small-path solver returns 1: it joins anyway, and the setting changes nothing for it.
 * Waits for a tiled copy that is still being built (the answer depends on it).
 * It pays from two wide members in a call on, more the smaller the members and the larger K: 18.6 x at 2500 x 4000 and K = 64,
 * 1.86 x at 33 874 x 105 728 and K = 8, the largest size and K measured; with one wide member it changes nothing (figures above). */
int hprlp_solver_set_group_wide(hprlp_solver *s, int on);

/* hprlp_solve_many_detect with every member wide.
 * det == NULL: no detection.
 * certs may be NULL. */
int hprlp_solve_many_wide(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param,
                          const hprlp_detection *det, HPRLP_results *out, hprlp_certificate *certs);

/* The calling thread's last *_many call that had a wide member (a solver off the small path with the setting on; a call without
 * one leaves the block as it is).  hprlp_solve_many_wide reports its loop, with its power iteration's two slots.
 * out = {wide members that joined,
 *        wide members that could not,
 *        normal-iteration group launches (two per iteration of a segment),
 *        iteration segments,
 *        member-iterations served by them,
 *        group launches of the power iteration,
 *        its host waits,
 *        0} */
int hprlp_last_many_wide_counts(long out[8]);

/* The segments of a round's normal iterations (wide members), no GPU needed.  counts[0..n): iterations owed per member, >= 0.
 * With c_1 < ... < c_J the distinct positive counts and c_0 = 0, segment j runs seg_len[j] = c_j - c_{j-1} iterations with the
 * members whose count is >= seg_min_count[j] = c_j.  Both arrays hold cap entries.  Returns J, or -1: a null array, n < 0, a
 * negative count, more than cap segments. */
int hprlp_group_iteration_plan(const int *counts, int n, int *seg_len, int *seg_min_count, int cap);

/* ---- group re-solve: new data, starts and solutions for the whole group (DESIGN.md "Many small LPs", group re-solve) ----------
 * The callers of a group -- scenario sets, MPC horizons, search-tree nodes -- change c and the bounds of K resident solvers and
 * solve again, over and over.  The two entries below are hprlp_solver_set_data and hprlp_solver_resolve for every member, with
 * the work on either side of the loop issued for the group: all given vectors travel in ONE pinned block and one copy, the data
 * passes, the zeroing, the bound codes, ctrl, the starts, the iteration-0 evaluations and the solutions run in one launch per
 * kernel for all members that join (small path, stream kernel alone, no locality ordering, bound-code arrays in place; two at
 * least), and the host waits once per call outside the loop -- none of it grows with the count.  Every member ends bit for bit
 * where its own call leaves it (the rule of the group launches: a workgroup runs the single kernel's code as workgroup lb of its
 * member's own grid).  A member that cannot join runs its own set_data / resolve pieces inside the same call; the ray tests
 * and certificates of the loop are the group's as in hprlp_solver_run_many.  Refusals (-1 + hprlp_last_error(), naming the entry point and `member k`) come before anything is written or
 * launched for any member: the group rules above, NULL data / out, an incomplete bounds group, a NaN in a data vector or
 * obj_constant, a NaN sigma, a non-finite start entry. */
typedef struct hprlp_member_data {   /* hprlp_solver_set_data's arguments for one member; all NULL: nothing changes */
    const double *c, *obj_constant, *AL, *AU, *l, *u;
} hprlp_member_data;
typedef struct hprlp_member_start {  /* hprlp_solver_resolve's arguments for one member */
    const double *x0, *y0;           /* NULL: zeros; both NULL: a cold re-solve */
    double sigma;                    /* > 0 overrides the norm_b / norm_c rule */
} hprlp_member_start;
/* hprlp_solver_set_data for every member: scaled vectors, bound codes, scales and norms as its own call leaves them, the group
 * that was not given untouched, the captured graphs kept.  A member whose entry is all NULL is skipped.  The seconds a member
 * reports for it (hprlp_solver_data_seconds, and the start of its next out.time) are the group call's wall time. */
int hprlp_solver_set_data_many(hprlp_solver **s, int count, const hprlp_member_data *data);
/* hprlp_solver_resolve for every member (start NULL: all cold): out[k] as hprlp_solver_run_many fills it (x, y, z malloc'd), no
 * trace; certificates from hprlp_solver_get_certificate.  out[k].time = the member's set_data time since its previous loop + the
 * group loop's wall time up to the member's last event.  For a member served by the group launches that wall time includes the
 * zeroing, bound-code, ctrl and start kernels: they run in front of the loop's first evaluation, after the loop's clock has
 * started, where hprlp_solver_resolve runs them before it starts its clock.  Results are not affected. */
int hprlp_solver_resolve_many(hprlp_solver **s, int count, const hprlp_member_start *start, HPRLP_results *out);
/* Counts of the calling thread's last hprlp_solver_set_data_many / hprlp_solver_resolve_many (whichever came last; each zeroes
 * and fills the slots), everything OUTSIDE the loop and with the operations of members that went their own way included:
 * out = {host-to-device copies (staging blocks and task tables), device-to-host copies, host waits, kernel launches, memsets,
 * members served by group launches, members that went their own way, resolve_many only: the loop's operations issued for ONE
 * member (hprlp_last_run_many_counts)}.  A member that gave nothing, or obj_constant only, is neither served nor on its own.
 * What the group issues is counted where it is issued; the operations of a member on its own are NOMINAL: what its single
 * entries issue in the common case (no locality ordering, bound-code arrays in place). */
int hprlp_last_resolve_many_counts(long out[8]);
/* self-test of the packing layout of the group's staging and result blocks, no GPU needed: 0, or the number of the failed check */
int hprlp_group_pack_selftest(void);
/* self-test of the table builder of the group launches (stage order, table block, launch list), no GPU needed: 0, or the number
 * of the failed check */
int hprlp_group_table_selftest(void);

/* ---- group matrix values: new coefficients on the resident patterns of the whole group (DESIGN.md "Many small LPs", group
 * matrix values) ------------------------------------------------------------------------------------------------------------
 * hprlp_solver_set_matrix_values for every member: an MPC horizon that re-linearises its dynamics, a scenario set that redraws
 * its coefficients.  Every member that gave values ends bit for bit where its own hprlp_solver_set_matrix_values leaves it -- a
 * fresh hprlp_solver_create on the changed model followed by hprlp_solver_scale: iterates zero; index arrays, kernel forms and
 * captured graphs kept.  The next steps are those after hprlp_solver_scale_many: hprlp_solver_power_iteration_many, init,
 * hprlp_solver_resolve_many.  The values and vectors of all members travel in ONE pinned block and one copy; the values of all
 * of them are checked on the device by one launch, one copy of one flag word per member and one wait; the members that join
 * (values given, the group re-solve's conditions, hprlp_solver_scale_many's; two at least) get scatter, gather, zeroing and the
 * whole scaling in one launch per kernel and stage, three more waits -- none of it grows with the count (the value maps apart: a
 * member builds its own at its first call).  A member that cannot join runs its own set_matrix_values inside the same call,
 * after the common check.  A member's hprlp_solver_matrix_seconds and the start of its next out.time are the group call's wall
 * times; hprlp_solver_transfer reports the member's own words.
 * Refusals (-1 + hprlp_last_error(), naming the entry point and `member k`): the group rules (NULL list or data, count <= 0, a
 * handle twice, a sharded member, a member never scaled, different devices); per member the single entry's rules with its
 * messages (some but not all of val, c, AL, AU, l, u; nnz other than the member's; a NaN in a vector or obj_constant), all before
 * the first upload; a non-finite value, found on the device in the staging block: `val[i]` with the smallest such i of the
 * lowest such member.  After ANY refusal EVERY member of the call is unchanged bit for bit and still usable. */
typedef struct hprlp_member_values {  /* hprlp_solver_set_matrix_values' arguments for one member; val NULL and all others NULL: skipped */
    const double *val; long nnz;
    const double *c, *obj_constant, *AL, *AU, *l, *u;
} hprlp_member_values;
int hprlp_solver_set_matrix_values_many(hprlp_solver **s, int count, const hprlp_member_values *data);
/* Counts of the calling thread's last hprlp_solver_set_matrix_values_many: out = {host-to-device copies (staging block and task
 * tables), device-to-host copies, host waits, kernel launches, memsets, members served by group launches, members that went
 * their own way (their operations are included: scaling launches and scalar fetches as the solver counts them, the rest nominal,
 * as hprlp_last_resolve_many_counts does), members whose value maps were built in this call (the map construction's own
 * operations are not counted)}. */
int hprlp_last_values_many_counts(long out[8]);

/* ---- group device re-solve: the three group entries from device memory, tensors in and out (DESIGN.md "Many small LPs", group
 * device re-solve) ------------------------------------------------------------------------------------------------------------
 * The callers of a group produce c, the bounds and the re-linearised coefficients on the GPU, consume x and y there and carry one
 * solve's x, y into the next as its start.  The three entries below are hprlp_solver_set_data_many, hprlp_solver_resolve_many and
 * hprlp_solver_set_matrix_values_many with every VECTOR pointer of the member structs a DEVICE array in the caller's units and
 * numbering (c, l, u, x0: n; AL, AU, y0: m; val: nnz); obj_constant stays a host pointer and sigma a host value, as in the single
 * device entries.  Semantics are those of the host group entries, argument for argument: an all-NULL member is skipped, the bounds
 * come together or not at all, start == NULL means all cold.  Nothing crosses the bus but scalars: no vector, start or solution is
 * copied; what travels is the task tables, one flag word per member and the packed scalars.
 *   Results: dst[k].x, .z (n) and .y (m) receive member k's solution; any may be NULL, dst == NULL or an all-NULL dst[k] means the
 * solution is not wanted and nothing is launched for it.  out[k].x, .y, .z are NULL (hprlp_free_results stays legal); every scalar
 * field of out[k] is as hprlp_solver_resolve_many fills it.  dst[k].x may be start[k].x0 and dst[k].y may be start[k].y0: the
 * group's start kernels run in front of the loop, the solution kernel behind it.  Buffers of DIFFERENT members must not overlap
 * (not checked).  hprlp_solver_transfer of every member reports 0 / 0 / 1.
 *   Pointers: before anything is launched or written every non-NULL device pointer of every member passes the single device
 * entries' rule (device memory of the group's device, 8-byte aligned, room for its length where the runtime reports the range).
 * A pointer that lies with its length inside a range the runtime has already reported in this call costs no second lookup, so a
 * group cut from a few packed tensors costs a few lookups whatever the count.  One exception to the 8 bytes: `val` of a member
 * that joins the group launches must be 16-byte aligned (its scatter loads the values in pairs).
 *   Ordering: one event is recorded on `stream` (the hipStream_t the inputs were produced on; NULL: the default stream), the
 * group's stream waits for it before its first read, and the call returns after the group's stream has drained.
 *   The device check: ONE launch checks the vectors of all members where they lie -- a NaN in c, AL, AU, l, u (set_data, matrix
 * values; the values themselves in the same stage), a non-finite entry of x0 / y0 (resolve; none launched when all are cold) --
 * into one flag word per member, one copy and one wait bring the verdicts back, and nothing a solver reads is written before
 * that wait.  The message is the host group entry's for the same numbers (`<entry>: member k: c[i] is NaN`: the lowest member,
 * then the order c, AL, AU, l, u, then the smallest index; a vector's NaN of any member wins over a non-finite value).  A NaN
 * obj_constant or sigma is refused on the host.
 *   Bits: every member ends bit for bit where the host group entry with the same numbers leaves it, hence where its own single
 * call leaves it; host and device entries may alternate on one group.  A member that cannot join the group launches (off the
 * small path, a locality ordering, bound-code arrays not in place; a group of fewer than two) runs its own
 * hprlp_solver_set_data_device / _resolve_device / _set_matrix_values_device inside the same call, on the same caller stream,
 * after the common checks.
 * 0, or -1 + hprlp_last_error() naming the entry point and `member k`: the group rules, NULL data / out, a pointer that does not
 * pass, an incomplete group, a wrong nnz, the device check.  After ANY refusal every member is unchanged bit for bit and usable.
 * hprlp_last_resolve_many_counts / hprlp_last_values_many_counts are filled with their meanings (host-to-device copies are then
 * task tables only; a member on its own adds its device entry's nominal operations). */
typedef struct hprlp_member_out { double *x, *y, *z; } hprlp_member_out;   /* device; any may be NULL: not wanted */
int hprlp_solver_set_data_many_device(hprlp_solver **s, int count, const hprlp_member_data *data, void *stream);
int hprlp_solver_resolve_many_device(hprlp_solver **s, int count, const hprlp_member_start *start, const hprlp_member_out *dst,
                                     void *stream, HPRLP_results *out);
int hprlp_solver_set_matrix_values_many_device(hprlp_solver **s, int count, const hprlp_member_values *data, void *stream);
/* The calling thread's last device group call (a refused one: up to its refusal): out = {device pointers checked, lookups issued
 * to the runtime, check-kernel launches, flag words copied back, members served by group launches, members on their own, waits
 * before the first write, 0} */
int hprlp_last_many_device_counts(long out[8]);

/* Named device vectors: x y x_hat x_bar y_bar z_bar x_temp y_temp y_obj last_x last_y AL AU l u c
 * row_norm col_norm A_val AT_val.  get returns the length (or -1); cap is the capacity of out. */
long hprlp_solver_get_vector(hprlp_solver *s, const char *name, double *out, long cap);
int hprlp_solver_set_vector(hprlp_solver *s, const char *name, const double *in, long len);
/* out = {b_scale, c_scale, norm_b, norm_c, norm_b_org, norm_c_org, sigma, lambda_max,
 *        setup_time, scaling_time, power_time, power_iters, kx, ky} */
int hprlp_solver_get_scalars(hprlp_solver *s, double out[16]);
/* out = {m, n, nnz, row blocks of A, row blocks of A^T, grid of y-half, grid of x-half,
 *        tiled flags (bit0: A, bit1: A^T use the column-tiled kernel)} */
int hprlp_solver_info(hprlp_solver *s, long out[8]);

/* Wall-clock phases [s] of the calling thread's last HPRLP_main_solve (what solve() runs after presolve):
 * out = {device set-up (upload, transpose, tiled copies, ordering), scaling, power iteration, loop, solution's way back,
 *        teardown of the device state, whole call, warm start (hprlp_solve_warm: upload, projection and the two SpMVs of
 *        the iteration-0 evaluation; 0 for a cold start)}.  The reference's instrument covers power iteration + loop only
 * (HPRLP_results.time, src/HPRLP.cu:150,246). */
int hprlp_last_solve_phases(double out[8]);

/* Human-readable: which kernel form runs on A and on A^T (stream / tiled fused / tiled pieces), super-blocks, steps, share of the
 * entries in staged tiles, long rows kept aside, small-LP kernel, locality ordering.  Returns the length (truncated to cap). */
int hprlp_solver_describe(hprlp_solver *s, char *buf, int cap);
/* Every environment switch the library reads, one per line: "<name>\t<integrator|hook>\t<what>" (returns the text's length; buf
 * may be NULL).  "integrator" switches are always honoured; "hook" switches (tests, measurements) only when HPRLP_TEST_HOOKS=1 is
 * set too.  hprlp_solver_describe ends with the switches a solver was set up under, so a non-default path is never silent. */
int hprlp_env_switches(char *buf, int cap);

/* Timed normal iterations for bench.py.  mode 0: graph replay as the product runs it; wall time by
 * HIP events around the whole batch.  mode 1: eager launches with an event pair around every kernel
 * on the solver's stream; xhalf_ms / yhalf_ms are the SUMS of the x-half / y-half kernel durations.  mode 2: the
 * bare SpMVs A^T y and A x_hat into scratch (no update, iterate untouched), timed like mode 1. */
int hprlp_solver_time_iterations(hprlp_solver *s, int warmup, int steps, int mode, double *total_ms,
                                 double *xhalf_ms, double *yhalf_ms);

/* ---- benchmark utility -------------------------------------------------------------------------
 * Rows [row0,row0+rows) of the banded-random matrix of BASELINE.json config 5 (per_row entries per
 * row, 95 % within +-band of the diagonal, 5 % anywhere, N(0,1) values).  Each row depends only on
 * (seed,row).  rowptr has rows+1 entries, col/val rows*per_row.  Not part of the solve path. */
int hprlp_gen_banded_csr(int m, int n, int per_row, int band, unsigned long long seed, int row0, int rows,
                         int *rowptr, int *col, double *val, int nthreads);

/* Rows [col_off, col_off + n_loc) of the TRANSPOSE of that matrix (= the columns a rank of a row-partitioned run owns:
 * hprlp_shard::AT_*), produced by sweeping all m rows of the generator and keeping the owned columns -- no rank holds the whole
 * matrix and nothing is communicated.  Equal entry for entry to the stable host transpose (reference src/utils.cu:203-232) of the
 * matrix generated whole.  trp: n_loc + 1 entries; *tci / *tv are malloc'd (release with hprlp_host_free); *nnz = their length. */
int hprlp_gen_banded_csr_transposed(int m, int n, int per_row, int band, unsigned long long seed, int col_off, int n_loc,
                                    int *trp, int **tci, double **tv, long *nnz, int nthreads);
void hprlp_host_free(void *p);

/* Benchmark utility: P A Q on the host (row i of the result = row row_new2old[i] of A, columns renumbered by col_old2new and
 * sorted) -- builds the randomly permuted variant of config 5 that the set-up time locality ordering has to undo. */
int hprlp_permute_csr_host(int m, int n, const int *rowptr, const int *col, const double *val, const int *row_new2old,
                           const int *col_old2new, int *rowptr_out, int *col_out, double *val_out, int nthreads);

/* ---- row-partitioned multi-GPU solve (new design; the reference is single-GPU) -----------------
 * Rank p owns rows [p*ceil(m/P),...) of A with y/AL/AU and rows [p*ceil(n/P),...) of A^T with
 * x/c/l/u; one in-place RCCL all-gather of the fresh vector slice follows each half-step. */
typedef struct hprlp_shard {
    int m, n;              /* global sizes */
    int row_off, m_loc;    /* rows of A owned by the rank */
    int col_off, n_loc;    /* rows of A^T (= columns of A) owned by the rank */
    int *A_rowptr, *A_col; /* m_loc x n, global column indices */
    double *A_val;
    int *AT_rowptr, *AT_col; /* n_loc x m, global column (= row of A) indices */
    double *AT_val;
    double *AL, *AU;       /* m_loc */
    double *l, *u, *c;     /* n_loc */
    double obj_constant;
} hprlp_shard;

/* block partition of `total` items over `parts` ranks: returns the chunk size ceil(total/parts) */
int hprlp_partition(int total, int parts, int rank, int *offset, int *count);
/* host only: cut this rank's shard out of a full model (arrays malloc'd; release with hprlp_free_shard) */
int hprlp_extract_shard(const LP_info_cpu *model, int rank, int size, hprlp_shard *out);
void hprlp_free_shard(hprlp_shard *s);
/* rank 0: create the RCCL unique id(s), 128 bytes each; the launcher broadcasts them (bench.py: torch.distributed).
 * bytes >= 256 yields TWO ids: hprlp_solver_create_dist* called with id_bytes >= 256 then builds a second communicator
 * for the exchange stream (exchanges that overlap the local part of a half-step), so that no communicator is driven
 * from two streams; with one id the single communicator serves both. */
int hprlp_dist_unique_id(void *out, int bytes);
/* HPRLP_DIST_TRANSPORT=shm in the environment of hprlp_dist_unique_id's caller: the id names a POSIX shared-memory segment and
 * hprlp_solver_create_dist* given that id build a host-staged group of processes on ONE node (device -> pinned shared area ->
 * the reader's device; no RCCL, no device IPC handle): the transport of last resort, and the multi-process form a one-GPU box
 * can run.  hprlp_shm_transport_selftest: the protocol alone on host buffers (no GPU): `rounds` rounds of all-gather, scalar
 * all-reduce and a ragged neighbour exchange, every payload checked; hang_rank >= 0 leaves half-way without a word (the others
 * must fail after HPRLP_DIST_TIMEOUT_S seconds, default 120).  0, or -1 + hprlp_last_error(). */
int hprlp_shm_transport_selftest(const void *unique_id, int id_bytes, int rank, int size, int rounds, int hang_rank);
/* every rank: create the solver for its shard of `model` (param->device_number selects the GPU).
 * get_vector/run then return this rank's slices; scalars/residuals are global. */
hprlp_solver *hprlp_solver_create_dist(const LP_info_cpu *model, const HPRLP_parameters *param, int rank, int size,
                                       const void *unique_id, int id_bytes);
/* The same from a shard the caller assembled itself -- rows [row_off, row_off + m_loc) of A and rows [col_off, col_off + n_loc)
 * of A^T in the block partition of hprlp_partition(), global column indices, arrays owned by the caller (copied to the
 * device during the call).  No rank has to hold the whole matrix (config 5 is generated per shard);
 * hpr-lp-c_amd/shard.py builds the A^T rows of every rank from the ranks' A rows with one all-to-all. */
hprlp_solver *hprlp_solver_create_dist_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                  const void *unique_id, int id_bytes);
/* How the fresh slices travel: if the shards' column indices name at most half of the remote entries
 * (banded / block-structured LPs) each rank sends exactly the entries its peers read (pack kernel, one grouped
 * RCCL send/recv, scatter kernel); otherwise one in-place all-gather.  HPRLP_DIST_EXCHANGE=sparse|allgather
 * overrides (same value on every rank).
 * out = {m-vectors sparse?, entries sent, received, n-vectors sparse?, sent, received, all ranks' requests m, n} */
int hprlp_solver_dist_info(hprlp_solver *s, long out[8]);
/* What the transport itself reports: out = {ranks, this rank, device of the main communicator (RCCL: ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice), the same three of the exchange stream's communicator (0, -1, -1 without one),
 * the solver's HIP device, 1 if exchanges overlap the half-steps}.  bench.py prints these as rccl_ranks / devices. */
int hprlp_solver_dist_comm_info(hprlp_solver *s, long out[8]);
/* Test hook: one grouped send/recv of `count` doubles from this rank to itself through the solver's communicator,
 * verified on the host (0 = intact).  Exercises the point-to-point transport calls where no second rank exists. */
int hprlp_solver_dist_loopback(hprlp_solver *s, int count);
/* The same multi-rank solver with `size` ranks as host THREADS of one process on one GPU, exchanging through
 * device copies and host barriers instead of RCCL: lets the sharded path run on a one-GPU box (tests). Every
 * rank's thread must make the same sequence of solver calls. */
typedef struct hprlp_local_group hprlp_local_group;
hprlp_local_group *hprlp_local_group_create(int size);
void hprlp_local_group_destroy(hprlp_local_group *g);
hprlp_solver *hprlp_solver_create_local(const LP_info_cpu *model, const HPRLP_parameters *param, int rank, int size,
                                        hprlp_local_group *group);
hprlp_solver *hprlp_solver_create_local_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                   hprlp_local_group *group);

/* ---- presolve / postsolve as separate host-side steps (what solve() does around the iteration when
 * use_presolve is set; replaces the reference's forked PSLP worker, src/pslp_integration.cpp:628-787).
 * hprlp_presolve_run returns NULL when the model is left unchanged or looks infeasible/unbounded.
 * LIFETIME: the handle keeps a pointer to `model` (postsolve reads the original rows and costs); the model must stay
 * alive and unchanged until hprlp_presolve_free(). */
typedef struct hprlp_presolve hprlp_presolve;
hprlp_presolve *hprlp_presolve_run(const LP_info_cpu *model);
const LP_info_cpu *hprlp_presolve_reduced(const hprlp_presolve *p); /* owned by p */
/* out = {reduced m, reduced n, fixed cols, empty cols, singleton rows, empty rows, redundant rows, passes,
 *        dual-fixed cols, slack cols, parallel rows, parallel cols, forcing rows, doubleton rows, tightened bounds,
 *        rounds of the chain} */
int hprlp_presolve_stats(const hprlp_presolve *p, int out[16]);
/* (xr, yr, zr) of the reduced model -> (x, y, z) in the original dimensions */
int hprlp_presolve_postsolve(const hprlp_presolve *p, const double *xr, const double *yr, const double *zr, double *x,
                             double *y, double *z);
/* (x, y) in the original dimensions -> (xr, yr) of the reduced model, link by link: restriction, except where the postsolve
 * combines values (a folded parallel column, a slack substitution, a folded parallel row), where it applies the inverse -- a
 * primal-dual optimum of the original maps onto one of the reduced model.  Host only. */
int hprlp_presolve_forward(const hprlp_presolve *p, const double *x, const double *y, double *xr, double *yr);
void hprlp_presolve_free(hprlp_presolve *p);
/* out = {primal infeasibility, dual infeasibility, gap (all relative), primal objective, dual objective} on the
 * model as given (reference compute_original_kkt_metrics, src/pslp_integration.cpp:499-580) */
int hprlp_original_kkt(const LP_info_cpu *model, const double *x, const double *y, const double *z, double out[5]);

/* Set-up time locality ordering (host; hpr-lp-c_amd/csrc/reorder.cpp): row / column permutations (new -> old) that make
 * the pattern band-like so that the column-tiled kernels apply; the solver runs it by itself when a large matrix
 * fails the tiling test in its given order (HPRLP_NO_REORDER=1 disables) and returns x, y, z in the caller's numbering
 * like the reference's collect_solution (src/utils.cu:143-200).  out = {accepted, tiled share before, after, clusters,
 * components, seconds}. */
int hprlp_locality_ordering(int m, int n, const int *rowptr, const int *col, int *row_new2old, int *col_new2old, double out[6]);
/* Test infrastructure: the ordering step by step, on the host (on_device = 0: the functions of reorder.cpp) or on the device
 * (1: the pattern is uploaded and goes through device_cluster_positions, device_refine_order and device_tiling_dense_fraction,
 * the functions a solver's set-up calls), with `sweeps` refinement sweeps and NONE of the acceptance gates of
 * hprlp_locality_ordering / a solver's set-up.  Every output may be NULL: lab_r (m) / lab_c (n) the cluster labels after the two
 * majority rounds (-1 = unlabelled); pos0_r / pos0_c the positions before refinement (cluster positions); pos_r / pos_c the
 * positions after the sweeps (ranks); row_new2old / col_new2old; stats = {clusters, components, BFS levels, tiling share
 * before, after} by that side's own tiling test.  HPRLP_REORDER_CLUSTER (test hook) sizes the clusters on both sides. */
int hprlp_reorder_steps(int m, int n, const int *rowptr, const int *col, int on_device, int sweeps, int *lab_r, int *lab_c,
                        double *pos0_r, double *pos0_c, double *pos_r, double *pos_c, int *row_new2old, int *col_new2old,
                        double stats[5]);
/* Test infrastructure: P A Q as a solver's set-up forms it on the device (device_permute_csr): rows in the new order, the
 * entries of a row by new column, duplicates in their old order.  rp_out (m + 1), ci_out / val_out (nnz). */
int hprlp_permute_csr_device(int m, int n, const int *rowptr, const int *col, const double *val, const int *row_new2old,
                             const int *col_new2old, int *rp_out, int *ci_out, double *val_out);
/* Test infrastructure: the tiling test -- share of the entries in (row / 8192, column / 2048) pairs of at least 256 entries --
 * of a pattern as given (both permutations NULL) or permuted, by the host's or the device's form. */
int hprlp_tiling_share(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                       int on_device, double *share);
/* host only: the stream kernel's row blocks of a CSR pattern, built and checked as a solver's set-up does (dense rows cut by
 * column eighths when with_cuts != 0); out = {blocks, split rows, chunk slots, rows cut, longest chunk, entries covered};
 * -1 + hprlp_last_error() when the block list would be refused. */
int hprlp_row_block_plan(int m, int n, const int *rowptr, const int *col, int with_cuts, long out[6]);
/* host only: the column-tiled copy of a CSR pattern as the host builder lays it out (super-blocks of R rows: a multiple of 64 up to
 * 8192; tiles of T = 2048 or 1024 columns; min_dense: least share of the entries in staged tiles), verified entry by entry -- every
 * entry exactly once, codes name their entries, one chunk per accumulator inside a step, at most four layers per tile.
 * out = {tile entries incl. padding, remainder entries, steps, padding, most consecutive steps of one tile, staged share x 1e6};
 * -1 + hprlp_last_error() on the first violation or when the build declines the pattern. */
int hprlp_tiled_host_check(int m, int n, const int *rowptr, const int *col, int R, int T, double min_dense, long out[6]);

/* host only: what solve_batched does to a batch's vectors before anything is uploaded (hpr-lp-c_amd/csrc/batch_prep.h).  rn (m) /
 * cn (n): the row / column scaling of the shared matrix; C, l, u (n x B), AL, AU (m x B), X0 (n x B) / Y0 (m x B; either may be
 * NULL) column-major as solve_batched takes them.  The arrays of `out` are the caller's (NULL: not wanted). */
typedef struct hprlp_batched_prepared {
    double *C, *AL, *AU, *l, *u; /* the vectors in scaled units, infinite sides and bounds replaced by +-1e100 */
    double *scalars;             /* 7 x B, one after the other: b_scale, c_scale, norm_b, norm_c, norm_b_org, norm_c_org, first sigma */
    double *X0, *Y0;             /* the starts in scaled units ... */
    double *X_back, *Y_back;     /* ... and those mapped back as a solution's x and y are */
    double *z_back;              /* the scaled C mapped as a solution's z is (n x B) */
    int Bp, Bc;                  /* out: the padded batch and the chunk width of the device panels (HPRLP_BATCH_CHUNK is honoured) */
    double pad;                  /* in: the value of `panel`'s padding */
    double *panel;               /* n x Bp: the scaled C as a device panel */
    double *panel_back;          /* n x B: that panel's first B members, column-major again */
    long *panel_index;           /* n x B: [k * n + i] = where (row i, member k) sits in an n-row panel */
} hprlp_batched_prepared;
int hprlp_batched_prepare_host(int m, int n, int B, const double *rn, const double *cn, const double *C, const double *AL,
                               const double *AU, const double *l, const double *u, const double *X0, const double *Y0,
                               int use_bc_scaling, hprlp_batched_prepared *out);
/* ... with the norm rule named: 0 = exactly hprlp_batched_prepare_host, 1 = the tree rule of the device entry (csrc/batch_prep.h) */
int hprlp_batched_prepare_host_rule(int m, int n, int B, const double *rn, const double *cn, const double *C, const double *AL,
                                    const double *AU, const double *l, const double *u, const double *X0, const double *Y0,
                                    int use_bc_scaling, int norm_rule, hprlp_batched_prepared *out);

/* ---- which kernel form a matrix gets (hpr-lp-c_amd/csrc/form_select.h) as plain data ----------------
 * The rules are host-only functions of the records below; a solver's set-up measures the facts and asks them. */
typedef struct hprlp_form_built { /* a tiled copy as its builder left it */
    long ok;                      /* -1: no such build ran; 0: the builder declined the pattern; 1: built */
    long n_pieces, dense_entries, n_rem; /* pieces of the piece form (0: fused), entries in staged tiles / in the remainder lists */
    double rem_top_share;         /* share of the remainder that gathers from the 2 MB of most popular columns */
} hprlp_form_built;
typedef struct hprlp_form_facts { /* what the rules look at, for one pass over one matrix */
    long rows, cols, nnz, longest_row;
    double long_row_share;        /* share of the entries in rows of more than 256 entries (0 below 100 000 rows) */
    double line_density;          /* distinct 64-byte lines of the gathered vector per entry (1: not sampled) */
    double xcd_gather_bytes;      /* bytes of the gathered vector an XCD's eighth of the rows reads (0: not estimated) */
    long sb_rows, slots;          /* super-block height of the copy; workgroup slots of the device (CUs x resident workgroups) */
    double min_dense_override;    /* >= 0: the all-remainder request (a copy without a dense-tile requirement); < 0: none */
    long sharded;                 /* the matrix is a row shard of a multi-GPU solver */
    /* measured only when the earlier rules have not decided; -1: not measured */
    long heaviest_block;          /* entries of the heaviest block of sb_rows consecutive rows */
    double tiling_share;          /* cheap tiling test: share of the entries that would sit in dense tiles */
    long n_long_rows, long_rows_nnz; /* rows of more than 1024 entries and their entries */
    hprlp_form_built side, whole; /* the copy built without its long rows / of the whole matrix */
    double popular_share;         /* share of the entries on the 32 768 most popular 64-byte lines of the gathered vector */
    long heaviest_pb_block;       /* entries of the heaviest block of 4096 consecutive rows */
} hprlp_form_facts;
typedef struct hprlp_form_hook_value {
    int set;
    double value;
} hprlp_form_hook_value;
typedef struct hprlp_form_hooks { /* the test hooks (HPRLP_<NAME>, csrc/env.h) that influence the selection; all zero: none set */
    int no_tiled, tiled_anyway, pieces_anyway, host_tiling, no_long_side, no_pb_fallback, no_pb_long_rows, no_pb_kernel;
    int tiling_check;             /* 0: unset, 1: "1", 2: set to anything else */
    hprlp_form_hook_value tiled_min_rows, tiled_min_dense, tiled_min_cols, pb_min_cols, pb_min_nnz, tile_rows, tile_cols;
} hprlp_form_hooks;
typedef struct hprlp_form_decision { /* the staged decisions of one pass */
    int min_rows, min_cols;       /* before the build: fewest rows / columns of a matrix that is tried in a tiled form ... */
    double min_dense;             /* ... and the least share of the entries in staged tiles */
    int route;                    /* 0: nothing to do, 1: stream kernel after the cheap tiling test (thin rows), 2: not attempted
                                   * (shape), 3: too few rows, 4: build on the device, 5: the host builder, 6: built with the long
                                   * rows aside and kept */
    int side_tried;               /* the long-rows-aside build was attempted */
    int kept;                     /* after the build: a tiled copy is in place */
    int form;                     /* 0: stream kernel, 1: tiled fused, 2: tiled piece form, 3: tiled all-remainder form */
    int why;                      /* why there is no tiled copy (0: there is one, or no reason to give; form_select.h: NoTiled) */
    int long_rows_alone;          /* ... not attempted for the length of its rows alone (an input of rule 13) */
    int all_remainder_wanted;     /* the all-remainder form follows (a second pass with min_dense_override = 0) */
    char note[96];                /* the bracketed note of hprlp_solver_describe for `why` ("" or " [...]") */
} hprlp_form_decision;
/* host only: the decisions for a facts record (hooks NULL: none set).  -1 + hprlp_last_error() when a rule asks for a fact that
 * the record marks as not measured. */
int hprlp_form_select(const hprlp_form_facts *facts, const hprlp_form_hooks *hooks, hprlp_form_decision *out);
/* The facts A (which = 0) or A^T (1) of a solver was decided on: out[0] the pass with the dense-tile requirement (on the final
 * numbering, behind a locality ordering), out[1] the all-remainder pass where one followed.  Returns the number of passes. */
int hprlp_solver_form_facts(hprlp_solver *s, int which, hprlp_form_facts out[2]);

#ifdef __cplusplus
}
#endif
#endif /* HPRLP_AMD_H */
