// kernels.h -- device data views and launch wrappers of the hand-written gfx950 kernels.
// Everything here is private to the library; the C ABI is in include/*.h.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "tiled.h"

namespace hprlp {

constexpr int kWave = 64;         // CDNA wavefront
constexpr int kWavesPerBlock = 4; // 256-thread workgroups, one row block per wave
constexpr int kThreads = kWave * kWavesPerBlock;
constexpr int kStreamW = 512;     // max nonzeros staged through LDS by one wave (4 KiB per vector)
constexpr int kStreamRows = 64;   // max rows per stream block: one lane per row
constexpr int kLongRow = 64;      // rows longer than this get a whole wave (vector mode: lanes stride the row, then a wave sum).  256 until late in
                                  // round 2: one lane adding a 205-entry row in CSR order is a chain of 205 dependent additions -- 1.5 us of the
                                  // config-3 x-half launch (10.9 -> 9.4 us per iteration).  Rows up to 64 entries keep the plain CSR-order sum
                                  // (bit-identical to the oracle and to the single-workgroup kernel); longer ones agree to rounding.
constexpr int kSplitRow = 4096;   // rows longer than this are cut into chunks of this many nonzeros
constexpr int kNumScalars = 32;   // device scalar slots (see enum Slot)

// Scalar slots filled by the reduction epilogues.  0-9 follow the reference's 10-slot buffer
// (reference include/structs.h:196-206); the rest are ours.
enum Slot : int {
    S_CX = 0,      // c . x_bar
    S_YOBJ_Y = 1,  // y_obj . y_bar
    S_XZ = 2,      // x_bar . z_bar
    S_RD2 = 3,     // |Rd|^2
    S_RP2 = 4,     // |Rp|^2
    S_ADX_DY = 5,  // <A x_temp, y_temp>
    S_DY2 = 6,     // |y_temp|^2
    S_DX2 = 7,     // |x_temp|^2
    S_MOVE_X2 = 8, // |x_bar - last_x|^2
    S_MOVE_Y2 = 9, // |y_bar - last_y|^2
    S_LU2 = 10,    // iteration-0 bound violation
    S_PW_ZZ = 11,  // power iteration z.z
    S_PW_QZ = 12,  // power iteration q.z
    S_PW_ERR2 = 13,
    S_NB2 = 14,    // |conceptual b|^2
    S_NC2 = 15,    // |c|^2
    S_TMP0 = 16,
    S_TMP1 = 17,
    S_SMALL_PW_LAMBDA = 18,  // single-launch power iteration (small.hip): lambda ...
    S_SMALL_PW_ITERS = 19,   // ... and the iteration it stopped at (0: the kernel did not run)
    // infeasibility detection (Solver::ray_test), original units: k_ray_form's six, then the two ray SpMVs'
    S_RAY_DY = 20,  // D: bound terms of the rows
    S_RAY_CD = 21,  // c'd
    S_RAY_VY = 22,  // V: rows (max)
    S_RAY_WD = 23,  // W: columns (max)
    S_RAY_YN = 24,  // |y|_inf
    S_RAY_DN = 25,  // |d|_inf
    S_RAY_DZ = 26,  // D: bound terms of the columns (z = -A^T y)
    S_RAY_VZ = 27,  // V: columns (max)
    S_RAY_WQ = 28,  // W: rows (q = A d, max)
    // Solver::set_data (between two solves, when no ray test is in flight: the six slots of k_ray_form serve again)
    S_DATA_B_ORG = 20,  // |b|^2 of the caller's AL / AU
    S_DATA_C_ORG = 21,  // |c|^2 of the caller's c
    S_DATA_B_PRE = 22,  // |b|^2 after row_norm, before the b scaling (b_scale = 1 + its root; k_data_bc reads it on the device)
    S_DATA_C_PRE = 23,  // |c|^2 after col_norm, before the c scaling
    S_DATA_NB = 24,     // norm_b^2 of the final vectors
    S_DATA_NC = 25,     // norm_c^2
};

// Row-block descriptor: one per wave.  {first row, number of rows, first nonzero, nonzero count}.
// rows==1 && nz>kLongRow: vector mode (lanes stride the row); otherwise stream mode (nz<=kStreamW,
// rows<=kStreamRows): products staged in LDS in CSR order, lane t sums row t sequentially.
struct CsrDev {
    int rows = 0, cols = 0;
    int nnz = 0;
    int nt = 1;  // stream the matrix with nontemporal loads (large matrices); 0: keep it in L2 between launches
    const int *rowptr = nullptr;
    const int *col = nullptr;
    double *val = nullptr;
    const int4 *blk = nullptr;
    int nblk = 0;
    TiledDev tiled;  // optional column-tiled copy (tiled.h); when valid every fused launch uses it
    // rows longer than kSplitRow: {row, first chunk slot, one past last slot, 0}; chunk sums land in
    // long_partial[2*slot + v] and k_long_finish completes the row
    const int4 *longrows = nullptr;
    int nlong = 0;
    double *long_partial = nullptr;
    int csr_grid() const { return (nblk + kWavesPerBlock - 1) / kWavesPerBlock; }
    int finish_grid() const { return (nlong + kThreads - 1) / kThreads; }
    // workgroups of a fused launch on this matrix = number of reduction partials it writes
    int tiled_finish_grid() const { return (rows + kThreads - 1) / kThreads; }
    int grid() const { return tiled.valid ? (tiled.n_pieces > 0 ? tiled_finish_grid() : tiled.grid) : csr_grid() + finish_grid(); }
};

// Device-resident iteration scalars (reference Halpern_params[4] + halpern_inner,
// include/structs.h:153-168).  kx is read by the x-half, ky by the y-half; each half writes the
// other's counter, so no kernel reads a word that is written during the same launch.
struct Ctrl {
    double sigma, lam_sigma, inv_lam_sigma, inv_sigma;
    int kx, ky;
    int pad0, pad1;
};

// Hand-off of the remainder products between the two kernels of an iteration (tiled.h, propagation blocking): the
// half-step that PRODUCES a gathered vector (x_hat or y) holds a super-block's fresh values in LDS at its epilogue and
// writes the products a * v[col] of the OTHER matrix' remainder entries whose source group is that super-block straight
// into the other matrix' P -- the consumer then skips its pre-pass (k_far_products).  gptr == nullptr: no hand-off.
struct FarPush {
    const int *gptr = nullptr;       // n_groups + 1 of the consumer matrix (group g = rows of the producer's super-block g)
    const double *val = nullptr;
    const int *pos = nullptr;
    const uint16_t *lcol = nullptr;
    double *P = nullptr;
    // run tables of the consumer's source side (tiled.h: f_rptr / f_rk / f_rp); null: positions come from `pos`
    const int *rptr = nullptr, *rk = nullptr, *rp = nullptr;
};

struct XHalfArgs {
    const double *y_full;  // gather source (all rows of y)
    double *x, *x_hat;     // local slices (x_hat points into the gathered x_hat buffer)
    const double *l, *u, *c, *last_x;
    double *x_bar, *z_bar, *x_temp;  // check variant only
    Ctrl *ctrl;
    double *partials;  // check variant: 3 x stride
    int stride;
    FarPush push;            // x_hat's products into the remainder buffer of A (consumed by the y-half)
    bool far_ready = false;  // A^T's remainder buffer already holds the products of y_full (pushed by the y-half before)
    // one byte per column saying which of l[j], u[j] the update has to READ (launch_bound_codes): the common bounds -- lower
    // bound 0 or -inf, upper bound +inf -- are constants of the code and cost no 8-byte load (LPs have l = 0, u = +inf on
    // most columns: 16 of the x-half's 56 bytes per column).  nullptr: always load both.
    const unsigned char *lu_code = nullptr;
    // Normal x-halves of a matrix with a tiled copy, inside a run of normal iterations (Solver::run_normal): x is
    // f2' * x_hat + f1' * last_x of values the previous x-half stored and this one reads anyway, so it need not travel through
    // memory between them.  kXRebuild: this launch forms its x from x_hat and last_x with the previous iteration's Halpern
    // factors (bit for bit the value the previous launch would have stored); kXNoStore: this launch does not store x (the next
    // one rebuilds it).  The first launch of a run reads x, the last one stores it: everybody else finds x in memory.
    int x_mode = 0;
};
constexpr int kXRebuild = 1, kXNoStore = 2;
// bit 0: l[j] must be loaded (neither -inf nor +0.0); bit 1: u[j] must be loaded (not +inf); bit 2: l[j] is +0.0
constexpr unsigned kLoadL = 1u, kLoadU = 2u, kZeroL = 4u;
void launch_bound_codes(int n, const double *l, const double *u, unsigned char *code, hipStream_t s);

struct YHalfArgs {
    const double *xhat_full;
    double *y;  // local slice inside the gathered y buffer
    const double *AL, *AU, *last_y;
    double *y_bar, *y_obj, *y_temp;
    Ctrl *ctrl;
    double *partials;  // check variant: 2 x stride
    int stride;
    FarPush push;            // y's products into the remainder buffer of A^T (consumed by the next x-half)
    bool far_ready = false;  // A's remainder buffer already holds the products of xhat_full
    // one byte per row saying which of AL[i], AU[i] the update has to READ (launch_row_codes), as lu_code for the x-half: an
    // infinite side is a constant of the code, an equality row (AL == AU) reads one value for both.  nullptr: load both.
    const unsigned char *row_code = nullptr;
};
// bit 0: AL[i] must be loaded (finite, differs from AU[i]); bit 1: AU[i] must be loaded (finite); bit 2: AL[i] == AU[i] (finite)
constexpr unsigned kLoadLo = 1u, kLoadHi = 2u, kRowEq = 4u;
void launch_row_codes(int m, const double *AL, const double *AU, unsigned char *code, hipStream_t s);

struct FinalizeItem {
    const double *partials;
    int count;
    int slot;
    int max = 0;  // 1: the partials are nonnegative maxima (their maximum, not their sum)
};
struct FinalizeArgs {
    FinalizeItem item[8];
    int n;
};

// return true if the launch filled the `push` buffer (the fused tiled kernel ran and a hand-off was requested)
bool launch_x_half(const CsrDev &AT, const XHalfArgs &a, bool check, hipStream_t s);
bool launch_y_half(const CsrDev &A, const YHalfArgs &a, bool check, hipStream_t s);
// the hand-off lists of a tiled matrix as a consumer (empty if it has no remainder lists)
FarPush far_push_of(const CsrDev &consumer);
// normal half-steps over the remote-column part of a split matrix; base = row sums of the local-column part
void launch_x_half_base(const CsrDev &AT_remote, const XHalfArgs &a, const double *base, hipStream_t s);
void launch_y_half_base(const CsrDev &A_remote, const YHalfArgs &a, const double *base, hipStream_t s);

// |(c - AT y_bar - z_bar) .* col_norm|^2 partials (reference residual_compute_Rd, main_iterate.cu:217-226)
void launch_resid_d(const CsrDev &AT, const double *ybar_full, const double *c, const double *z_bar,
                    const double *col_norm, double *partials, hipStream_t s);
// |max(min(AU - A x_bar,0), AL - A x_bar) .* row_norm|^2 partials, optionally <A x_temp, y_temp> in the same pass
void launch_resid_p(const CsrDev &A, const double *xbar_full, const double *xtemp_full, const double *AL,
                    const double *AU, const double *row_norm, const double *y_temp, bool with_gap,
                    double *partials, int stride, hipStream_t s);
// <A x_temp, y_temp> partials only (reference compute_weighted_norm, main_iterate.cu:486-515)
void launch_gap(const CsrDev &A, const double *xtemp_full, const double *y_temp, double *partials, hipStream_t s);
// out = M v ; optionally partials of out.out and out.q  (power iteration)
// plain product whose epilogue hands the remainder products of the OTHER matrix over (returns true if it did)
bool launch_spmv_push(const CsrDev &M, const double *v_full, double *out, const FarPush &push, hipStream_t s);
void launch_spmv_plain(const CsrDev &M, const double *v_full, double *out, const double *q, bool with_dots,
                       double *partials, int stride, hipStream_t s, bool far_ready = false);

void launch_finalize(const FinalizeArgs &f, double *scalars, hipStream_t s);

// ---- infeasibility detection (Solver::ray_test): the candidate rays and the Farkas ratio test in original units -------------
// k_ray_form: ds = x_bar - prev_x, ys = y_bar - prev_y, prev_* <- *_bar, and the elementwise terms; partials (kRayFormAccs x
// nblocks): D of the rows, c'd (sums), V of the rows, W of the columns, |y|_inf, |d|_inf (maxima)
constexpr int kRayFormAccs = 6;
struct RayFormArgs {
    int n, m;
    const double *x_bar, *y_bar;
    double *prev_x, *prev_y, *ds, *ys;
    const double *l, *u, *c, *col_norm, *AL, *AU, *row_norm;
    double b_scale, c_scale;
};
void launch_ray_form(const RayFormArgs &a, double *partials, int nblocks, hipStream_t s);
// z = -A^T y on the scaled ray (A^T, gathered ys): partials (2 x AT.grid()) of D of the columns (sum) and V of the columns (max)
void launch_ray_col(const CsrDev &AT, const double *ys_full, const double *l, const double *u, const double *col_norm, double b_scale,
                    double c_scale, double *partials, hipStream_t s);
// q = A d on the scaled ray (A, gathered ds): partials (A.grid()) of W of the rows (max)
void launch_ray_row(const CsrDev &A, const double *ds_full, const double *AL, const double *AU, const double *row_norm, double b_scale,
                    double *partials, hipStream_t s);

// ---- warm start (Solver::set_start, DESIGN.md "Warm start"): the caller's point into the iteration state ---------------------
// k_start_in: x_s = clamp(x0[pc[j]] * col_norm[j] / b_scale, l_j, u_j) into x, last_x, x_hat, x_bar and y_s = y0[pr[i]] *
// row_norm[i] / c_scale, projected onto the sign cone of row i's sides, into y, last_y, y_bar.  x0 / y0 null: zeros; pc / pr
// null: no locality ordering (device index = caller's index).
struct StartInArgs {
    int n, m;
    const double *x0, *y0;  // device copies of the caller's vectors (caller's numbering)
    const int *pc, *pr;     // device index -> caller's index, or null
    const double *l, *u, *col_norm, *AL, *AU, *row_norm;
    double b_scale, c_scale;
    double *x, *last_x, *x_hat, *x_bar, *y, *last_y, *y_bar;
};
void launch_start_in(const StartInArgs &a, hipStream_t s);
// z_bar = dual completion of w = c - A^T y_bar (A^T, gathered y_bar); partials (2 x AT.grid()) of c.x_bar and of the bound terms
// l.z+ + u.z- (what x_bar.z_bar is at a check)
void launch_start_col(const CsrDev &AT, const double *ybar_full, const double *c, const double *l, const double *u,
                      const double *x_bar, double *z_bar, double *partials, hipStream_t s);
// y_obj = AL / AU / clamp(A x_bar) by the sign of y_bar (A, gathered x_bar); partials (A.grid()) of y_obj.y_bar
void launch_start_row(const CsrDev &A, const double *xbar_full, const double *AL, const double *AU, const double *y_bar,
                      double *y_obj, double *partials, hipStream_t s);

// x_temp = x_bar - last_x, y_temp = y_bar - last_y, squared norms -> partials (2 x stride);
// then last_x = x = x_bar, last_y = y = y_bar and the Halpern counter is reset
// (reference update_sigma movement + do_restart, main_iterate.cu:312-322,369-375)
void launch_movement(int n, int m, const double *x_bar, const double *last_x, double *x_temp, const double *y_bar,
                     const double *last_y, double *y_temp, double *partials, int stride, int nblocks, hipStream_t s);
void launch_restart_copy(int n, int m, const double *x_bar, double *x, double *last_x, const double *y_bar,
                         double *y, double *last_y, Ctrl *ctrl, hipStream_t s);
// iteration-0 bound violation (reference residual_compute_lu_kernel)
void launch_lu(int n, const double *x_bar, const double *l, const double *u, const double *col_norm, double *x_temp,
               double *partials, int nblocks, hipStream_t s);
void launch_set_ctrl(Ctrl *ctrl, double sigma, double lambda_max, int reset_k, hipStream_t s);

// scaling (reference src/scaling.cu)
// tval_log / fval_log: the log values of M's tiled copy (launch_tiled_refresh_log) -- the pass then runs through the tiled
// kernel if cr_runs_tiled(M); null: stream kernel
void launch_cr_log_update(const CsrDev &M, const double *other_full, double *result, hipStream_t s, const double *tval_log = nullptr,
                          const double *fval_log = nullptr);
bool cr_runs_tiled(const CsrDev &M);
void launch_exp_clamp(double *v, int n, hipStream_t s);
void launch_row_norm(const CsrDev &M, double *result, int norm, hipStream_t s);
double launch_line_density(const int *rowptr, const int *col, int rows, hipStream_t s);  // distinct 64-byte lines gathered per entry, sampled (synchronises)
// max_i rowptr[i+1] - rowptr[i] (synchronises the stream); entries_in_long (optional): the entries in rows of more than `limit` entries
int launch_longest_row(const int *rowptr, int rows, hipStream_t s, int limit = 0, long *entries_in_long = nullptr);
// the most entries any block of `height` consecutive rows holds (synchronises the stream)
int launch_heaviest_block(const int *rowptr, int rows, int height, hipStream_t s);
// val = op(op(val, first), second) where first/second are the row vector or the gathered column vector
void launch_scale_matrix(const CsrDev &M, const double *rowvec, const double *colvec_full, bool row_first,
                         bool divide, hipStream_t s, double *next_max_norm = nullptr);
void launch_vec_scale(double *x, const double *s, int n, bool divide, hipStream_t s_);
void launch_vec_scal(double *x, double a, int n, hipStream_t s);
void launch_fill(double *x, double a, int n, hipStream_t s);
void launch_bnorm2(const double *AL, const double *AU, int m, double *partials, int nblocks, hipStream_t s);
void launch_norm2(const double *x, int n, double *partials, int nblocks, hipStream_t s);

// power iteration helpers
void launch_check_columns(long nnz, int cols, const int *col, int *bad, hipStream_t s);
void launch_pw_start(int m, unsigned long long seed, long long offset, double *z, hipStream_t s);  // power_start_vector on the device
void launch_pw_normalize(const double *z, double *q, int m, const double *scalars, hipStream_t s);
void launch_pw_err(const double *z, const double *q, int m, const double *scalars, double *partials, int nblocks,
                   hipStream_t s);

// ---- re-solve (Solver::set_data, DESIGN.md "Re-solve"): new data of the caller into the resident model's scaled vectors --------
// k_data_in: AL, AU = in[pr[i]] / row_norm[i]; c = in[pc[j]] / col_norm[j]; l, u = in[pc[j]] * col_norm[j]; partials (4 x stride)
// of |b|^2, |c|^2 of the caller's data and of the scaled data.  m / nc / nb = 0: that part was not given.  pc / pr null: no
// locality ordering.  Grid kReduceBlocks, the reduction of k_bnorm2 / k_norm2.
struct DataInArgs {
    int m, nc, nb;
    const double *AL_in, *AU_in, *c_in, *l_in, *u_in;  // device copies of the caller's vectors (caller's numbering)
    const int *pc, *pr;
    const double *row_norm, *col_norm;
    double *AL, *AU, *c, *l, *u;
    double *partials;
    int stride;
};
void launch_data_in(const DataInArgs &a, hipStream_t s);
// k_data_bc: AL, AU, l, u *= 1 / (1 + sqrt(scalars[S_DATA_B_PRE])), c *= 1 / (1 + sqrt(scalars[S_DATA_C_PRE])) (use_bc; else as they
// are), row_code / lu_code of the results (null: not kept), partials (2 x stride) of norm_b^2, norm_c^2
struct DataBcArgs {
    int m, nc, nb;
    int use_bc;
    const double *scalars;
    double *AL, *AU, *c, *l, *u;
    unsigned char *row_code, *lu_code;
    double *partials;
    int stride;
};
void launch_data_bc(const DataBcArgs &a, hipStream_t s);

// x = b_scale * x_bar / col_norm etc. (reference collect_solution, utils.cu:143-200)
void launch_unscale(int n, int m, const double *x_bar, const double *y_bar, const double *z_bar,
                    const double *col_norm, const double *row_norm, double b_scale, double c_scale, double *xo,
                    double *yo, double *zo, hipStream_t s);

// ---- device-resident re-solve (DESIGN.md "Device-resident re-solve"): the caller's device buffers in, the caller's buffers out ----
// k_unscale_out: k_unscale's three operations in its order, on its grid and element-to-thread map, stored into the caller's
// buffers in the caller's numbering: xo[pc[j]], zo[pc[j]], yo[pr[i]] (pc / pr: device index -> caller's index, null: no locality
// ordering).  A null output is skipped.
void launch_unscale_out(int n, int m, const double *x_bar, const double *y_bar, const double *z_bar, const double *col_norm,
                        const double *row_norm, double b_scale, double c_scale, const int *pc, const int *pr, double *xo, double *yo,
                        double *zo, hipStream_t s);
// k_data_check: one grid-stride pass over up to kDataCheckVecs caller vectors (null / length 0: skipped).  *first_bad, which the
// caller sets to kDataCheckClean before the launch, receives the smallest (vector << kDataCheckShift) | index whose entry is NaN
// (non_finite = 0) or not finite (non_finite = 1: the warm start's rule).
constexpr int kDataCheckVecs = 5;
constexpr int kDataCheckShift = 56;
constexpr unsigned long long kDataCheckClean = ~0ULL;
struct DataCheckArgs {
    const double *v[kDataCheckVecs];
    int len[kDataCheckVecs];
    int non_finite;
};
void launch_data_check(const DataCheckArgs &a, unsigned long long *first_bad, hipStream_t s);

// ---- small-LP path (small.hip): `count` normal iterations in one single-workgroup launch -----------
constexpr int kSmallMaxK = 12;     // matrix entries per thread (1024 threads) -> nnz <= 12288
constexpr int kSmallMaxR = 2;      // rows per thread -> m, n <= 2048
constexpr int kSmallMaxRow = 256;  // longest row / column (its owner thread sums it sequentially)
struct SmallArgs {
    int m, n, nnz;
    const int *A_rowptr, *AT_rowptr;
    const double *AT_val;          // the matrix is read once, in A^T order
    const int *ent_ij;             // per A^T entry: row i of A | column j << 16
    const int *ent_posA;           // per A^T entry: position of the same entry in the CSR order of A
    const int *order_x, *order_y;  // rows of A^T / of A sorted by length, longest first (n / m entries)
    double *x, *x_hat, *y;
    const double *l, *u, *c, *last_x, *AL, *AU, *last_y;
    Ctrl *ctrl;
};
bool small_path_fits(int m, int n, long nnz, int max_row_A, int max_row_AT);
void launch_small_iterations(const SmallArgs &a, int count, hipStream_t s);
// the whole power iteration of a small LP in one launch (small.hip): z0 = start vector (m), out = {lambda, iterations done}
void launch_small_power(const SmallArgs &a, const double *z0, int max_iter, double tol, double *out, hipStream_t s);

// ---- many small LPs at once (small.hip, DESIGN.md "Many small LPs"): grid = number of tasks, workgroup b runs task b exactly as
// the single-LP kernel runs its arguments.  K is filled in by the launch wrappers.
struct SmallIterTask {
    SmallArgs a;
    int K, count;  // count <= 0: the workgroup (if one is launched at all) returns at once
};
struct SmallPowerTask {
    SmallArgs a;
    const double *z0;  // start vector (m)
    double *out;       // {lambda, iterations done}
    double tol;
    int K, max_iter;
};
// Where the task lists travel: a pinned staging block and its device copy, both grown on demand.  One list is in flight per
// stream; the staging block is rewritten only after the previous copy out of it has completed.
struct SmallTaskBuf {
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t copied = nullptr;
    SmallTaskBuf() = default;
    SmallTaskBuf(const SmallTaskBuf &) = delete;
    SmallTaskBuf &operator=(const SmallTaskBuf &) = delete;
    ~SmallTaskBuf();
    void *stage(size_t bytes);  // room for `bytes` in the staging block, free to be written
    void send(size_t bytes, hipStream_t s);
};
// One launch per <KMAX, R> class present among the tasks (the classes of launch_small_iterations / launch_small_power); tasks
// with count <= 0 are left out.  Returns the number of launches.
int launch_small_iterations_many(const SmallIterTask *tasks, int ntasks, SmallTaskBuf &buf, hipStream_t s);
int launch_small_power_many(const SmallPowerTask *tasks, int ntasks, SmallTaskBuf &buf, hipStream_t s);

// ---- group forms of the regular kernels (kernels.hip, DESIGN.md "Many small LPs"): check step, evaluation and restart of every
// member of a group in one launch per kernel.  A workgroup runs the single kernel's body as workgroup lb of lg of its member, so a
// member's partials and scalars are the bits of its own launches.
// What the stream kernel reads of a matrix that has neither a tiled copy nor split rows.
struct CsrStream {
    int nblk, nt;
    const int *rowptr, *col;
    const double *val;
    const int4 *blk;
    double *long_partial;  // (null, never reached: no block of such a matrix is a chunk of a split row)
    __host__ __device__ int csr_grid() const { return (nblk + kWavesPerBlock - 1) / kWavesPerBlock; }
};
bool group_form_fits(const CsrDev &M);  // every fused launch on M is one k_spmv_fused launch: no tiled copy, no split rows
// The calls mirror the single launch_* wrappers and only record; run() sends the tables of all records in one copy and issues ONE
// launch per kind present and stage, the kinds in one fixed order (kernels.hip: GroupKinds -- the order of a member's own calls
// wherever two kinds of a stage touch the same memory; the table part is host only: group_table.h); fetch() packs the scalar
// blocks recorded by pack() and enqueues one copy to the host; deliver(), after the caller's wait, hands each member its
// kNumScalars doubles.  Whatever a member enqueues itself between run() and fetch() rides on that copy.  The loop, the re-solve
// and the data passes record with own_launches: a kind that holds ONE task is issued as that member's own launch (arguments in the
// launch, no table), a stage's finalize items that are one member's and at most 8 go through launch_finalize, and one member's
// scalars come by its own copy -- a group of one issues what the member issues alone.  scale_many records without it: every kind
// present gets its table.  One run's tables are in flight at a time: the caller waits for the stream between two runs of one
// object (the staging block is rewritten only after the copy out of it has completed, as for SmallTaskBuf).
struct VectorsInArgs;  // values.h
class GroupLaunches {
  public:
    explicit GroupLaunches(bool own_launches = true);
    ~GroupLaunches();
    GroupLaunches(const GroupLaunches &) = delete;
    void x_half_check(const CsrDev &AT, const XHalfArgs &a);
    void y_half_check(const CsrDev &A, const YHalfArgs &a);
    // Wide members (DESIGN.md "Many small LPs", wide members).  The normal half-steps as launch_x_half / launch_y_half issue them on
    // a matrix without a tiled copy (a.x_mode 0, no hand-off; anything else is refused): the caller closes the stage after each,
    // the y-half gathers what the x-half stores.  The regular-kernel power iteration: launch_pw_normalize, launch_spmv_push with an
    // empty hand-off, launch_spmv_plain with the two dots, launch_pw_err on kReduceBlocks workgroups -- a stage each.
    void x_half(const CsrDev &AT, const XHalfArgs &a);
    void y_half(const CsrDev &A, const YHalfArgs &a);
    void pw_normalize(const double *z, double *q, int m, const double *scalars);
    void pw_err(const double *z, const double *q, int m, const double *scalars, double *partials);  // kReduceBlocks partials
    void spmv_push(const CsrDev &M, const double *v_full, double *out);
    void spmv_dots(const CsrDev &M, const double *v_full, double *out, const double *q, double *partials, int stride);
    void resid_d(const CsrDev &AT, const double *ybar_full, const double *c, const double *z_bar, const double *col_norm, double *partials);
    void resid_p(const CsrDev &A, const double *xbar_full, const double *xtemp_full, const double *AL, const double *AU, const double *row_norm,
                 const double *y_temp, bool with_gap, double *partials, int stride);
    void gap(const CsrDev &A, const double *xtemp_full, const double *y_temp, double *partials);
    void finalize(const FinalizeArgs &f, double *scalars);
    void movement(int n, int m, const double *x_bar, const double *last_x, double *x_temp, const double *y_bar, const double *last_y, double *y_temp,
                  double *partials, int stride);
    void restart_copy(int n, int m, const double *x_bar, double *x, double *last_x, const double *y_bar, double *y, double *last_y, Ctrl *ctrl);
    void set_ctrl(Ctrl *ctrl, double sigma, double lambda_max, int reset_k);
    void pack(const double *scalars, double *host);  // a member's device scalars and the host block they go to
    // The kernels on either side of the loop (DESIGN.md "Many small LPs", group re-solve; many.cpp: set_data_many, resolve_many).
    // fill(x, +0.0, n) leaves the bits of a memset.
    void fill(double *x, double a, int n);
    void bound_codes(int n, const double *l, const double *u, unsigned char *code);
    void row_codes(int m, const double *AL, const double *AU, unsigned char *code);
    void start_in(const StartInArgs &a);
    void start_col(const CsrDev &AT, const double *ybar_full, const double *c, const double *l, const double *u, const double *x_bar, double *z_bar,
                   double *partials);
    void start_row(const CsrDev &A, const double *xbar_full, const double *AL, const double *AU, const double *y_bar, double *y_obj, double *partials);
    void lu(int n, const double *x_bar, const double *l, const double *u, const double *col_norm, double *x_temp, double *partials);  // kReduceBlocks partials
    void data_in(const DataInArgs &a);  // stride kReduceBlocks, as the member's own launch
    void data_bc(const DataBcArgs &a);
    void unscale(int n, int m, const double *x_bar, const double *y_bar, const double *z_bar, const double *col_norm, const double *row_norm,
                 double b_scale, double c_scale, double *xo, double *yo, double *zo);
    // The scaling kernels (DESIGN.md "Many small LPs", group scaling; the pieces of Solver::scale()).  fill, the two vector scalings
    // and exp / clamp share one launch; a matrix scaling is one launch per <ROW_FIRST, DIVIDE, NEXT> instance present.
    void vec_scale(double *x, const double *s, int n, bool divide);
    void vec_scal(double *x, double a, int n);
    void exp_clamp(double *v, int n);
    void bnorm2(const double *AL, const double *AU, int m, double *partials);  // kReduceBlocks partials
    void norm2(const double *x, int n, double *partials);
    void row_norm(const CsrDev &M, double *result, int norm);  // 99 or 1
    void scale_matrix(const CsrDev &M, const double *rowvec, const double *colvec_full, bool row_first, bool divide, double *next_max_norm);
    void cr_log_update(const CsrDev &M, const double *other_full, double *result);
    // New matrix values (DESIGN.md "Many small LPs", group matrix values; values.h has the single launches): the check of one
    // member's staged values into its own flag word, the scatter through the value maps, the gather of the five vectors.
    void values_check(const double *v, long n, unsigned long long *first_bad);
    void values_in(long nnz, const double *stage, const int *mapA, const int *mapAT, double *A_val, double *AT_val);
    // The group's device entries (DESIGN.md "Many small LPs", group device re-solve): k_data_check on one member's caller vectors
    // into its own flag word, which the caller has set to kDataCheckClean.  Nothing is recorded where no vector is given.
    void data_check(const DataCheckArgs &a, unsigned long long *first_bad);
    void vectors_in(const VectorsInArgs &a);
    // Infeasibility detection (DESIGN.md "Many small LPs", group detection): the ray test's three kernels, mirroring launch_ray_*
    // (the form on its kReduceBlocks workgroups), and a verdict's raw arrays into the group's certificate block -- elementwise
    // copies and the plain product M v (launch_spmv_plain without dots) writing straight into it.
    void ray_form(const RayFormArgs &a, double *partials);
    void ray_col(const CsrDev &AT, const double *ys_full, const double *l, const double *u, const double *col_norm, double b_scale, double c_scale,
                 double *partials);
    void ray_row(const CsrDev &A, const double *ds_full, const double *AL, const double *AU, const double *row_norm, double b_scale, double *partials);
    void copy(double *dst, const double *src, int n);
    void spmv_plain(const CsrDev &M, const double *v_full, double *out);
    long tables_sent() const;  // host-to-device copies of the tables so far (one per run() that had a table to send)
    int recorded_launches() const;  // what run() would issue for the records held now
    // What is recorded from here on runs after everything recorded so far, finalize included (one run, one copy of the tables
    // all the same; nothing happens while the open stage holds no record).  Needed where a later kernel overwrites partials an
    // earlier finalize reads: an evaluation's Rd writes part_x, where the check step before it left the partials of c.x -- alone,
    // the member finalises the check step in between.
    void next_stage();
    // The last n closed stages are issued `times` times in a row (the twenty Curtis-Reid sweeps share two tables).
    void repeat_last(int nstages, int times);
    int run(hipStream_t s);    // returns the number of launches
    int fetch(hipStream_t s);  // returns the number of copies to the host (0: nothing was recorded by pack())
    void deliver();
  private:
    struct Impl;
    std::unique_ptr<Impl> impl;
};
long &scaling_launch_count();  // kernel launches of the scaling wrappers above on the calling thread (callers take differences)

// device CSR -> device CSR of the transpose, stable in row order (transpose.hip); all pointers are device memory,
// trp has cols+1 entries, tci / tv nnz
void device_transpose(int rows, int cols, long nnz, const int *rowptr, const int *col, const double *val, int *trp,
                      int *tci, double *tv, hipStream_t s);

// column split of a device CSR matrix into the entries with lo <= column < hi and the rest (transpose.hip)
void device_split_columns(int rows, long nnz, const int *rowptr, const int *col, const double *val, int lo, int hi, DBuf<int> &rp_loc,
                          DBuf<int> &col_loc, DBuf<double> &val_loc, DBuf<int> &rp_rem, DBuf<int> &col_rem, DBuf<double> &val_rem,
                          hipStream_t s);

// multi-GPU neighbour exchange: dst[k] = src[idx[k]] before the sends, dst[idx[k]] = src[k] after the receives
void launch_pack(const double *src, const int *idx, double *dst, int n, hipStream_t s);
void launch_scatter(double *dst, const int *idx, const double *src, int n, hipStream_t s);

constexpr int kReduceBlocks = 512;  // grid of the plain vector reductions

}  // namespace hprlp
