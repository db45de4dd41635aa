// solver.h -- device-resident single-LP HPR solver state (private).
// Replaces the reference's HPRLP_workspace_gpu / LP_info_gpu / Scaling_info / HPRLP_restart
// (reference include/structs.h:127-277) without vendor-library handles.
#pragma once

#include <string>
#include <vector>

#include <functional>
#include <future>
#include <map>
#include <memory>

#include "common.h"
#include "env.h"
#include "dist.h"
#include "kernels.h"
#include "hpr_rules.h"
#include "form_select.h"

namespace hprlp {

struct TraceRow {  // same layout as hprlp_trace_row in include/hprlp_amd.h
    int iter, restart_flag;
    double err_Rp, err_Rd, primal_obj, dual_obj, gap, kkt, sigma, current_gap, lambda_max;
};

// One row-partitioned CSR matrix resident on the device together with its row-block descriptors.
struct DeviceMatrix {
    DBuf<int> rowptr, col;
    DBuf<double> val;
    DBuf<int4> blk, longrows;
    DBuf<double> long_partial;
    DeviceTiled tiled;  // optional column-tiled copy for large matrices with column locality (tiled.h)
    // shape of the tiled copy, set by the solver before upload() / describe(): rows per super-block (tiled.h: 8192 unless
    // lowered for a mid-size matrix) and columns per source group of the remainder lists (= sb_rows of the OTHER matrix)
    int sb_rows = kTileRows, far_group = kTileRows;
    int rem_cap = kTileRemCap;  // entries per remainder step (tiled.h: kPbRemCap for the all-remainder form)
    int tile_cols = kTileCols;  // columns per tile of the copy (tiled.h: kTileCols, or kTileColsNarrow for narrow bands)
    CsrDev view;
    // The tiled copy is built on the host (about a second per 2e8 nonzeros) by a background job started in
    // upload(); until finish_tiling() has run every launch on this matrix uses the stream kernel.  `keep` is held
    // by the job (the A^T arrays, which nobody else owns); rp / ci must stay valid until finish_tiling().
    std::future<std::shared_ptr<TiledHost>> tiling;
    int planned_grid = 0;  // grid of the tiled kernel if the build succeeds (sizes the reduction partials)
    void upload(int rows, int cols, const int *rp, const int *ci, const double *v, std::shared_ptr<void> keep = nullptr);
    // after the arrays are on the device.  min_dense >= 0 overrides the share of the entries the tiled build wants in
    // staged tiles (0: accept any pattern -- everything outside dense tiles goes through the propagation-blocking remainder)
    void describe(int rows, int cols, const int *rp, const int *ci, std::shared_ptr<void> keep, double min_dense_override = -1.0);
    // the same with the host row pointers delivered later and the values possibly still being uploaded (solver.cpp)
    void describe_when(int rows, int cols, long nnz, std::shared_future<const int *> rp_ready, const int *ci, std::shared_ptr<void> keep,
                       double min_dense_override, std::future<void> *values_ready);
    void build_tiled_copy(int rows, int cols, int nnz, double long_row_share, const std::function<const int *()> &host_rp, const int *ci,
                          std::shared_ptr<void> keep, double min_dense_override, const std::function<void()> &join_values, struct PhaseTimer &pt);
    int longest_row = 0;  // entries of the longest row (set by describe)
    // Why the last describe() left no tiled copy (form_select.h; hprlp_solver_describe prints its note).  Every pass starts it
    // afresh -- except under HPRLP_NO_TILED=1, which leaves the matrix as it is.
    FormOutcome outcome;
    // What the rules were asked about: the last pass with the dense-tile requirement and the all-remainder pass (passes == 2)
    FormFacts facts = blank_form_facts(), facts_pb = blank_form_facts();
    int passes = 0;
    double xcd_gather_bytes = 0.0; // estimate by Solver::choose_sb_rows: bytes of the gathered vector an XCD's eighth of the rows reads (0: unknown)
    void finish_tiling(hipStream_t s);  // wait for the job, upload the copy, fill its values from the CSR values
    void refresh_tiled(hipStream_t s);  // re-gather the tiled values from the CSR values (after scaling)
};

std::vector<int4> build_row_blocks(int rows, const int *rowptr, std::vector<int4> *longrows);
// host only: the stream kernel's block list of a pattern, built and checked as describe_when() does (solver.cpp)
void row_block_plan_host(int rows, int cols, const int *rp, const int *ci, bool with_cuts, long out[6]);

// How one kind of gathered vector (length-m: read through the columns of the A^T shard; length-n:
// through the columns of the A shard) reaches this rank after a half-step.  Dense coupling: one
// in-place all-gather.  Sparse coupling (the shards name less than half of the remote entries, e.g.
// banded or block-angular LPs): every rank packs exactly the entries each peer's column indices
// name, one grouped send/recv moves them, a scatter kernel drops them into the full-length vector.
// The choice is made from the all-gathered request counts, so every rank takes the same branch.
struct HaloPlan {
    bool sparse = false;
    int nsend = 0, nrecv = 0;
    long total_requests = 0;  // over all ranks (info)
    DBuf<int> send_idx, recv_idx;  // positions in the gathered vector, grouped by peer, ascending
    DBuf<double> sendbuf, recvbuf;
    std::vector<P2P> ops;
    void build(Comm *comm, const int *cols, long nnz, int total, int chunk, hipStream_t s);
};

// What Solver::solve_loop keeps between two events (an event: evaluation, decision, restart).  The loop is
//   loop_begin; while (loop_event) loop_advance; loop_finish
// and a group of solvers advanced in lock-step (many.cpp) runs the same pieces member by member around shared launches and waits.
struct LoopState {
    int iter = 0;
    Residuals r;
    RestartState rs;
    bool first4 = true, first6 = true, first8 = true;
    std::string status = "CONTINUE";
    int pending = -1;        // normal iterations before the next check step (loop_advance); < 0: no check step either
    bool restarted = false;  // the last event restarted (its check step and weighted norm have run)
    bool periodic = false, at_limit = false, ray = false;  // of the evaluation in flight
    int verdict = 0, verdict_iter = 0;  // loop_status: the verdict that ended the loop (0: none), for loop_certificate
    int check_iter = 1, max_iter = 0;
    double t_before = 0.0;   // what the reported times start from
    clock_type::time_point t_loop;
    HPRLP_results *out = nullptr;
};

struct GroupBlocks;  // many.cpp

struct Solver {
    HPRLP_parameters prm;
    int m = 0, n = 0;          // global sizes
    int m_loc = 0, n_loc = 0;  // rows of A / rows of A^T owned by this rank
    int row_off = 0, col_off = 0;
    int m_pad = 0, n_pad = 0;  // gathered-vector lengths (multiple of the chunk size)
    double obj_constant = 0.0;
    bool verbose = true;
    hipStream_t stream = nullptr;
    // Created inside an ArenaScope (common.h; abi.cpp: hprlp_solver_create_many): the small device buffers and the pinned scalar
    // block of setup() are pieces of the group's arena, `stream` is the group's and goes with the arena, not with this solver.
    Arena *arena = nullptr;
    // setup() inside an ArenaScope is sound only where it allocates, zeroes and uploads and launches nothing (the uploads reach
    // the device at arena_flush): a model within the small path's sizes that no hook sends through a device transpose or a tiled
    // build.  Host-only test.
    static bool group_setup_fits(const LP_info_cpu *model);
    Comm *comm = nullptr;
    // Second communicator (its own unique id) for the exchanges enqueued on comm_stream beside the local part of a
    // half-step: a communicator is only ever driven from ONE stream.  Null: the in-process group (host-blocking, no
    // concurrency) or a launcher that handed over a single id -- then comm serves both streams as in rounds 1-2.
    Comm *xcomm = nullptr;

    DeviceMatrix A, AT;  // A: m_loc x n (global columns); AT: n_loc x m (global columns)
    // Set-up time locality ordering (reorder.cpp): when set, the device holds P A Q and all per-row / per-column vectors
    // in the permuted numbering; perm_r[i] / perm_c[j] = the caller's index of permuted row i / column j.  The C ABI
    // (get / set_vector, collect_solution) speaks the caller's numbering.
    std::vector<int> perm_r, perm_c;
    double reorder_time = 0.0, reorder_before = 0.0, reorder_after = 0.0;
    // Callers that read A / AT / row_norm / col_norm directly in the caller's numbering (solve_batched) switch the
    // ordering off before setup(): they would otherwise pair permuted scale vectors with unpermuted panels.
    bool allow_reorder = true;
    bool try_reorder(const LP_info_cpu *model);
    void choose_sb_rows(const LP_info_cpu *model);  // super-block heights of this LP's tiled copies (tiled.h), before the matrices are described
    void choose_pb_rows(DeviceMatrix &M, DeviceMatrix &other, int rows, int other_rows);  // ... of a matrix without column locality (all-remainder form, tiled.h)
    // (other_rowptr: the device row pointers of M's transpose, other_rows + 1 of them -- its view need not be described yet)
    bool pb_fallback_wanted(DeviceMatrix &M, const int *other_rowptr, int other_rows);  // unstructured large matrix: tiled form without dense-tile requirement
    // Hand-off of the remainder products between the two kernels of an iteration (kernels.h: FarPush).  far_A_ready: A's
    // remainder buffer holds the products of the current x_hat (written by the x-half's epilogue); far_AT_ready likewise
    // for y.  Every other launch on a tiled matrix refills its buffer for another vector: invalidate_far().
    bool far_A_ready = false, far_AT_ready = false;
    bool graph_end_A = false, graph_end_AT = false;  // what a replayed iteration graph leaves behind
    void invalidate_far() { far_A_ready = far_AT_ready = false; }
    FarPush push_into(const DeviceMatrix &consumer, const DeviceMatrix &producer) const;  // called by setup() for a large matrix that failed the tiling test
    HaloPlan halo_m, halo_n;  // exchange of length-m / length-n gathered vectors (multi-GPU only)
    DBuf<double> AL, AU, l, u, c, row_norm, col_norm;
    DBuf<unsigned char> row_code;  // per row: which of AL, AU the y-half reads (kernels.h); follows AL / AU (refresh_bound_codes)
    DBuf<unsigned char> lu_code;  // per column: which of l, u the x-half reads (kernels.h); follows l / u (refresh_bound_codes)
    void refresh_bound_codes(GroupLaunches *g = nullptr);
    // local work vectors
    DBuf<double> x, last_x, z_bar, last_y, y_obj, y_temp;
    // gathered vectors (length *_pad); the local slice starts at *_off
    DBuf<double> gy, gxh, gxb, gyb, gxt, gsn, gsm;
    double *y = nullptr, *x_hat = nullptr, *x_bar = nullptr, *y_bar = nullptr, *x_temp = nullptr;
    DBuf<double> sm1, sn1;  // local scratch
    DBuf<Ctrl> ctrl;
    DBuf<double> scal;
    HBuf<double> scal_h;
    DBuf<double> part_x, part_y, part_r, part_v;
    int stride_x = 0, stride_y = 0;

    double b_scale = 1, c_scale = 1, norm_b = 0, norm_c = 0, norm_b_org = 1, norm_c_org = 1;
    double sigma = 1.0, lambda_max = 1.0;
    double setup_time = 0, scaling_time = 0, power_time = 0;
    double fetch_enqueue_s = 0, fetch_wait_s = 0;  // HPRLP_TIMING: host time in fetch_scalars (enqueue of the copy / wait for the stream)
    long fetches = 0;
    int power_iters = 0;
    bool use_graph = true;
    bool use_small = false;  // Netlib-scale LP on one GPU: normal iterations run in the single-workgroup kernel (small.hip)
    // hprlp_solver_set_group_wide: off the small path this solver asks for the group launches of the *_many entries all the same
    // (joins_group; DESIGN.md "Many small LPs", wide members).  Nothing outside those entries reads it.
    bool group_wide = false;
    int max_row_A = 0, max_row_AT = 0;
    DBuf<int> small_order_x, small_order_y;  // rows of A^T / A sorted by length (row ownership in small.hip)
    DBuf<int> small_ij, small_posA;          // per A^T entry: i | j << 16, position in the CSR order of A

    // Infeasibility detection: at every periodic evaluation the rays d = x_bar - x_bar(previous evaluation), y = y_bar - y_bar(...)
    // pass the ratio tests or not (ray_test enqueues, ray_scalars().verdict() judges after the evaluation's scalar fetch).  The
    // buffers exist only while detection is on; nothing the iteration reads is touched, so the iterates are the same bits either way.
    Detection detect;
    DBuf<double> ray_prev_x, ray_prev_y, ray_d, ray_y, ray_part;
    bool ray_have_prev = false;
    Certificate cert;  // of the last solve_loop (kind 0: no verdict)
    // solve_loop: buffers allocated (first time) and the previous iterate forgotten.  g: the first-time zeroing is recorded as
    // fills of +0.0 (the bits of the memset) instead of four synchronous memsets
    void ray_begin(GroupLaunches *g = nullptr);
    // enqueue the rays' kernels and reductions; false at the first evaluation (no previous iterate yet).  g: the form, the two
    // SpMVs and the nine finalize items recorded (a first test records the form only)
    bool ray_test(GroupLaunches *g = nullptr);
    RayScalars ray_scalars();      // after fetch_scalars: the ratio tests' sums of the last ray_test
    void collect_certificate(int kind, int iter);
    // collect_certificate in the pieces a group call walks (many.cpp: loop_many): the raw arrays recorded into the member's ranges
    // of the group's block (kind 1: row_norm, col_norm, ray_y and A^T y_s by the plain product; kind 2: col_norm, ray_d; the
    // pointers a kind does not use are null), then, once the block is on the host, finish_certificate and the un-permutation
    void certificate_launch(int kind, double *rn, double *cn, double *ray, double *aty, GroupLaunches *g);
    void certificate_consume(int kind, int iter, const double *rn, const double *cn, const double *ray, const double *aty);

    // Warm start (DESIGN.md "Warm start"): after init_iteration_state(), before solve_loop().  x0 (n) / y0 (m): the caller's point
    // in the caller's units and numbering (host memory, either may be null: zeros), every entry finite.  Projects it, writes it
    // into every vector the first iteration reads and evaluates it for iteration 0 (z_bar, y_obj, S_CX, S_XZ, S_YOBJ_Y).  Single
    // GPU only.  start_time: seconds of the last call (upload, kernels, reductions).
    void set_start(const double *x0, const double *y0);
    double start_time = 0.0;

    // Re-solve (DESIGN.md "Re-solve"): new data for the LP this solver holds, caller's units and numbering, host memory.  Objective
    // group: c_ (n) and / or obj_constant_; bounds group: AL_, AU_ (m), l_, u_ (n), all four or none.  A null group keeps its
    // vectors, scales, norms and bound codes bit for bit.  After scale(); single GPU only.  Throws before anything is written
    // (a NaN, an incomplete bounds group).  Two kernels (k_data_in, k_data_bc), two finalizes, one scalar fetch.
    void set_data(const double *c_, const double *obj_constant_, const double *AL_, const double *AU_, const double *l_, const double *u_);
    // A further solve on this solver: iterates to zero, sigma from the current norm_b / norm_c (sigma_ > 0 overrides), lambda_max as
    // it stands, optional start, loop, solution.  out->time = set_data seconds since the previous loop + this loop.
    void resolve(double sigma_, const double *x0, const double *y0, HPRLP_results *out);
    double data_time[3] = {0.0, 0.0, 0.0};  // the last set_data: upload, kernels + fetch, total
    double data_since_run = 0.0;            // set_data seconds since the last solve_loop
    double time_base = -1.0;                // solve_loop: what the reported time starts from (< 0: power_time, as the reference)
    bool scaled = false;                    // scale() has run: row_norm / col_norm are the model's
    DBuf<double> data_stage, data_part;     // set_data: the uploaded vectors (kept between calls while small), 4 x kReduceBlocks partials
    DBuf<int> perm_r_dev, perm_c_dev;       // set_data: the locality ordering's permutations on the device (first use)
    std::vector<double> data_pack;          // set_data: small vectors travel in one copy
    // set_data_many / resolve_many with this solver as member 0 (the owner of the group's stream): the group's staging, partials
    // and result blocks, grown on demand and kept between calls (many.cpp)
    std::shared_ptr<GroupBlocks> group_blocks;

    // Matrix values (DESIGN.md "Matrix values"): new values on the resident pattern.  val: the nnz values of the model's CSR in the
    // caller's order; the five vectors and obj_constant_ (null: kept) in the caller's units and numbering, host memory.  Afterwards
    // the solver is bit for bit a fresh setup() on the changed model followed by scale(): values scattered through the value maps,
    // vectors written unscaled in the solver's numbering, iterates zeroed, scale() as it is.  The power iteration is the caller's
    // next step.  After scale(); single GPU only.  Throws before anything the solver reads is written (a NaN in a vector, a
    // non-finite value -- found on the device in the staging block).
    void set_matrix_values(const double *val, long nnz, const double *c_, const double *obj_constant_, const double *AL_, const double *AU_,
                           const double *l_, const double *u_);
    // The value maps, built at the first use and kept (4 bytes per entry each): map_A[e] / map_AT[k] = the caller's CSR position of
    // entry e of A / k of A^T as the device holds them.  map_A stays empty where it is the identity (no locality ordering).
    void build_value_maps();
    DBuf<int> map_A, map_AT;
    bool have_maps = false;
    bool device_transposed = false;      // setup() built A^T with device_transpose (else csr_transpose_host)
    DBuf<int> src_rowptr, src_col;       // locality ordering in place: the caller's pattern on the device, until the maps are built
    DBuf<double> matrix_stage;           // [val | AL | AU | l | u | c], kept between calls while small (as data_stage)
    DBuf<unsigned long long> values_flag;
    double matrix_time[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // the last call: maps (first call only), upload, kernels, scale(), total
    long matrix_calls = 0;

    // Device-resident re-solve (DESIGN.md "Device-resident re-solve"): set_data, resolve and set_matrix_values with the caller's
    // vectors in DEVICE memory (caller's units and numbering) and the solution written into the caller's device buffers.  The
    // kernels of the host entries read the caller's pointers in the staging block's place, so the bits are the host entries'.
    // Every device pointer passes check_device_pointer before anything is launched; `caller` is the stream the inputs were
    // produced on (the solver's stream waits for an event recorded on it), and the solver's stream has drained on return.  A NaN
    // (a non-finite entry of a start) is found by k_data_check before anything the solver reads is written.
    void set_data_device(const double *dc, const double *obj_constant_, const double *dAL, const double *dAU, const double *dl,
                         const double *du, hipStream_t caller);
    // dx0 / dy0 null: cold; dx, dz (n) / dy (m) null: not wanted; dx may be dx0 and dy may be dy0.  out->x / y / z stay null.
    void resolve_device(double sigma_, const double *dx0, const double *dy0, hipStream_t caller, double *dx, double *dy, double *dz,
                        HPRLP_results *out);
    void set_matrix_values_device(const double *dval, long nnz, const double *dc, const double *obj_constant_, const double *dAL,
                                  const double *dAU, const double *dl, const double *du, hipStream_t caller);
    // The last successful set_data* / set_matrix_values* / resolve*: bytes of model data and solution host -> device, device ->
    // host, 1 for a device entry, device-entry calls so far.
    long transfer[4] = {0, 0, 0, 0};
    hipEvent_t inputs_ready = nullptr;       // recorded on the caller's stream, waited for by `stream`
    DBuf<unsigned long long> check_flags;    // k_data_check's word and k_values_check's, fetched together

    std::map<int, hipGraphExec_t> graphs;
    TraceRow *trace = nullptr;
    int trace_cap = 0, trace_n = 0;

    Solver() = default;
    ~Solver();
    Solver(const Solver &) = delete;

    // reference copy_lpinfo_to_device + allocate_memory (src/preprocess.cu:66-256)
    void setup(const LP_info_cpu *model, const HPRLP_parameters *param);
    // distributed variant: the caller supplies this rank's rows of A and rows of A^T
    void setup_shard(int m_glob, int n_glob, int row_off_, int m_loc_, int col_off_, int n_loc_, const int *Arp,
                     const int *Aci, const double *Av, const int *ATrp, const int *ATci, const double *ATv,
                     const double *AL_, const double *AU_, const double *l_, const double *u_, const double *c_,
                     double obj_constant_, const HPRLP_parameters *param, Comm *comm_);
    void scale();                                                   // src/scaling.cu:88-216
    // scale() in pieces (many.cpp: scale_many walks them for a group, with a stage change or a host round trip between two).  g:
    // record instead of issuing; then a zeroing is a fill of +0.0, the second pair of gathered vectors and the two slots for the
    // pair of sums (w->sums) are the caller's, and nothing is fetched: the caller brings the sums to the host.
    struct ScaleWalk {
        double *gm = nullptr, *gn = nullptr;            // the gathered scale vectors of this pass ...
        double *gm_next = nullptr, *gn_next = nullptr;  // ... and where a scaling pass leaves the next pass's row norms (fuse)
        bool fuse = false, have_norms = false;          // have_norms: gm_next / gn_next hold the next pass's row norms
        int passes = 0;                                 // Ruiz (ten) + Pock-Chambolle (one)
        double *sums = nullptr;                         // g: |b|^2 and |c|^2 are finalised into sums[0], sums[1]
        DBuf<double> gsm2, gsn2;                        // alone: the second pair
        DBuf<double> logA_tile, logA_far, logAT_tile, logAT_far;  // alone: -log|a| of the tiled copies, for the Curtis-Reid sweeps
    };
    void scale_begin(ScaleWalk *w, GroupLaunches *g = nullptr);          // fills, norms of the unscaled b and c, Curtis-Reid set-up
    void scale_sums(ScaleWalk *w, GroupLaunches *g, double out[2], bool also_tmp0 = false);  // |b|^2, |c|^2 (alone: fetched into out)
    void scale_norms_org(const double sums[2]);                          // ... of the unscaled problem: norm_b_org, norm_c_org
    void scale_cr_sweep(ScaleWalk *w, bool transposed, GroupLaunches *g = nullptr);  // one Curtis-Reid update on A or on A^T
    void scale_cr_exp(ScaleWalk *w, GroupLaunches *g = nullptr);         // after the sweeps: exp / clamp ...
    void scale_cr_apply(ScaleWalk *w, GroupLaunches *g = nullptr);       // ... and the Curtis-Reid scaling pass (reads what exp / clamp wrote)
    void scale_pass(ScaleWalk *w, int it, GroupLaunches *g = nullptr);   // Ruiz / Pock-Chambolle pass `it` (nothing past w->passes)
    void scale_bc_apply(const double sums[2], GroupLaunches *g = nullptr);  // b_scale, c_scale and their passes (1 without b / c scaling)
    void scale_finish(ScaleWalk *w, GroupLaunches *g, double out[2]);    // norms of the scaled b and c, tiled copies, bound codes
    void scale_norms(const double sums[2]);                              // ... norm_b, norm_c
    void scale_end(GroupLaunches *g = nullptr);                          // the gathered vectors back to zero
    double power_iteration(int max_iter, double tol, int *iters);   // src/power_iteration.cu:20-119
    void init_iteration_state(GroupLaunches *g = nullptr, double sigma_ = -1.0);  // src/HPRLP.cu:154-167 (sigma_ > 0 with g: the override)
    // (g, here and below: record the launch for a group run instead of issuing it -- kernels.h: GroupLaunches, many.cpp)
    void set_sigma_lambda(double sigma_, double lambda_, bool reset_k, GroupLaunches *g = nullptr);
    void reset_iterates(GroupLaunches *g = nullptr);                // all iterates back to zero (as after create + scale + power iteration)
    void step(bool check, GroupLaunches *g = nullptr);              // one HPR iteration
    void run_normal(int count);                                     // count normal iterations (graph replay)
    void run_normal_then_check(int count);                          // count normal iterations, then one check-variant iteration
    void fetch_scalars();                                           // fetch_enqueue + fetch_wait
    void fetch_enqueue();                                           // the asynchronous copy of the scalars, no wait
    void fetch_wait();                                              // the wait for the stream
    // main_iterate.cu:229-309; ray: also the infeasibility detection's ray test (detect.on only), read by ray_verdict()
    void compute_residuals(int iter, bool compute_gap, Residuals *r, RestartState *rs, bool *ray = nullptr);
    // its two halves: everything up to and including the asynchronous copy of the scalars / what follows the wait for the stream
    void residuals_enqueue(int iter, bool compute_gap, bool *ray);
    void residuals_launch(int iter, bool compute_gap, GroupLaunches *g);  // its kernels and finalize: no ray test, no copy (g: iter > 0 only)
    void residuals_consume(int iter, bool compute_gap, Residuals *r, RestartState *rs);
    double weighted_norm_after_restart();                           // main_iterate.cu:486-515: gap_launch, fetch, weighted_norm_consume
    void gap_launch(GroupLaunches *g);
    double weighted_norm_consume();                                 // (the rare lambda bump inside is always the solver's own launch)
    // main_iterate.cu:312-322,367-404: movement_launch, fetch, restart_launch
    void update_sigma_and_restart(RestartState *rs, const Residuals &r);
    void movement_launch(GroupLaunches *g);                         // the movement and its two norms, not fetched
    void restart_launch(RestartState *rs, const Residuals &r, GroupLaunches *g);  // movement fetched: the sigma rule, restart copy, ctrl
    // Check step, evaluation and restart run in the group launches (many.cpp): small path or group_wide, one GPU, and both matrices
    // run the stream kernel alone (no tiled copy, no split rows).  Adopts a pending tiled copy first.
    bool joins_group();
    // the arguments of one normal iteration's half-steps, as launch_normal_pair issues them without an exchange in flight
    XHalfArgs normal_x_args(int x_mode);
    YHalfArgs normal_y_args();
    // One normal half-step of a wide member recorded (y_half: the second one); the caller closes the stage behind it.
    void normal_half(bool y_half, GroupLaunches &g);
    // The pieces of power_iteration's regular path (g: recorded; the caller closes the stage behind each piece):
    //   power_norm   |z|^2 of the start vector and its finalize
    //   power_piece  0: q = z / |z|;  1: A^T q (true: it handed A's remainder products over -- never with g);  2: z = A (A^T q)
    //                with the two dots and their finalize (handed: what piece 1 returned)
    //   power_err    |z - lambda q|^2 and its finalize
    void power_norm(GroupLaunches *g = nullptr);
    bool power_piece(int piece, GroupLaunches *g = nullptr, bool handed = false);
    void power_err(GroupLaunches *g = nullptr);
    void solve_loop(HPRLP_results *out);                            // src/HPRLP.cu:154-310
    // the pieces of solve_loop (LoopState)
    void loop_begin(LoopState *ls, HPRLP_results *out, GroupLaunches *g = nullptr);  // (g: ray_begin's zeroing recorded)
    // first half of an event: the evaluation of the current iterate, not waited for.  g: kernels and finalize recorded, nothing
    // else; fetch = false: without the copy of the scalars (a group's copy carries them)
    void loop_enqueue_evaluation(LoopState *ls, GroupLaunches *g = nullptr, bool fetch = true);
    // the ray test of that evaluation where detection asks for one (true: enqueued, or recorded into g)
    bool loop_enqueue_ray(LoopState *ls, GroupLaunches *g = nullptr);
    // second half, after the wait, in pieces that end where the host has to wait for scalars:
    //   loop_status    status, marks, restart decision.  false: finished (ls->status says how; a verdict is noted in
    //                  ls->verdict and collected by loop_certificate); true: ls->restarted says whether the two pieces below run
    //   loop_certificate  a noted verdict's certificate: collect_certificate (its copies and its wait)
    //   loop_movement  the movement and its norms enqueued                                  [wait]
    //   loop_restart   the sigma rule, restart copy, ctrl, check step, gap enqueued         [wait]
    //   loop_plan      a restart's weighted norm consumed; ls->pending and ls->iter say what runs next
    bool loop_status(LoopState *ls);
    void loop_certificate(LoopState *ls);
    void loop_movement(LoopState *ls, GroupLaunches *g = nullptr);
    void loop_restart(LoopState *ls, GroupLaunches *g = nullptr);
    void loop_plan(LoopState *ls);
    bool loop_event(LoopState *ls);               // loop_enqueue_evaluation, wait, the four pieces with their waits
    // what run_normal_then_check does for ls->pending; normal_done: the normal iterations have been run by a group launch
    void loop_advance(LoopState *ls, bool normal_done = false, GroupLaunches *g = nullptr);
    void loop_finish(LoopState *ls);              // the results' scalars
    SmallArgs small_args() const;                 // the single-workgroup kernels' view of this LP (use_small)
    bool small_power_wanted() const;              // the power iteration runs in the single-workgroup kernel
    void power_start(double *z);                  // the power iteration's start vector (m_loc), in place on return
    void collect_solution(HPRLP_results *out);                      // src/utils.cu:143-200
    double reduce_sum_sq(const double *v, int n_local);             // allreduced ||v||^2
    void verify_exchange();                                         // set-up self-test of the exchange (multi-GPU only)
    void gather(double *gbuf, bool is_m) { gather_on(gbuf, is_m, stream); }  // all-gather a length-m or length-n vector
    void gather_on(double *gbuf, bool is_m, hipStream_t s);

    // Multi-GPU overlap of the exchange with the local part of the next half-step: both shards are split
    // by columns into the part that reads this rank's own slice of the gathered vector and the part that reads remote
    // entries.  While the exchange runs on comm_stream, the local part's row sums go to `part`; the remote part's
    // kernel adds them and runs the epilogue.  Built after scaling (the copies carry the scaled values).
    struct SplitShard {
        DeviceMatrix loc, rem;
        DBuf<double> part;
    };
    std::unique_ptr<SplitShard> ovA, ovAT;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_done_x = nullptr, ev_done_y = nullptr;
    // the environment switches in effect when this solver was set up (env.h), and the test hooks found set but ignored
    std::string env_at_setup, env_ignored_at_setup;
    bool hook_no_far_push = false, hook_no_bound_codes = false, hook_store_x = false;  // test hooks read once per solver (read_hooks), used every iteration
    void read_hooks();
    bool overlap_enabled = false, overlap_ready = false, y_exchange_pending = false;
    bool overlap_spmv_first = false;  // launch order of the local SpMV and the exchange (launch_normal_pair)
    void prepare_overlap();
    void ensure_comm_stream();
    void allreduce_scalars();
    void finish_tiling();  // adopt tiled copies whose background build is still pending (no-op otherwise)

    // One normal iteration.  ev (optional, 3 events): recorded before the x-half, between the halves, after the y-half.
    // more_follow (multi-GPU overlap only): the caller launches another normal pair next, so the exchange of y may stay
    // in flight behind the local part of that pair's x-half; otherwise the gathered y is complete on return.
    void launch_normal_pair(bool more_follow = false, hipEvent_t *ev = nullptr, int x_mode = 0);
    // kernels.h XHalfArgs::x_mode of iteration `i` of a run of `count` normal iterations enqueued back to back (0 where the
    // x-half's epilogue has no such mode: no tiled copy, split shards)
    int x_mode_of(int i, int count) const;

    // The pieces of set_data / resolve that a group call records instead of launching (DESIGN.md "Many small LPs", group re-solve;
    // many.cpp: set_data_many, resolve_many).  Each ends where the host must wait; the single entries call them with g = nullptr
    // and issue today's launches in today's order.
    void data_first_pass(const double *dAL, const double *dAU, const double *dl, const double *du, const double *dc, bool bounds, double *part,
                         GroupLaunches *g);                                      // k_data_in, finalize
    void data_second_pass(bool bounds, bool c_, double *part, GroupLaunches *g);  // k_data_bc, finalize
    void data_consume(bool bounds, bool c_);                                      // the host formulas, scalars fetched
    void start_launch(const double *dx, const double *dy, const int *dpc, const int *dpr, GroupLaunches *g);  // start_apply without its wait
    void solution_launch(double *xo, double *yo, double *zo, GroupLaunches *g);   // k_unscale
    bool bound_codes_in_place() const;  // row_code / lu_code need no allocation (or the hook keeps them out)
    // joins_group(), and nothing of this member's set_data / resolve needs a launch or an allocation of its own: no locality
    // ordering, code arrays in place (allocating them drops the captured graphs)
    bool joins_group_resolve();
    void set_transfer(size_t h2d_words, size_t d2h_words, bool device_entry);

   private:
    // What the host and the device entries share: everything after the caller's vectors are readable on the device.
    void data_apply(const double *dAL, const double *dAU, const double *dl, const double *du, const double *dc, bool bounds,
                    clock_type::time_point t0);
    void start_apply(const double *dx, const double *dy, const int *dpc, const int *dpr);
    void values_apply(const double *dval, long nnz, const double *dAL, const double *dAU, const double *dl, const double *du,
                      const double *dc, const double *obj_constant_, clock_type::time_point t0, double times[5]);
    void perms_to_device();                                                   // perm_r_dev / perm_c_dev, first use
    void wait_for_caller(hipStream_t caller);                                 // event on `caller`, `stream` waits for it
    unsigned long long *cleared_check_flags();                                // two words of all ones
    void alloc_work();
    hipGraphExec_t graph_for(int len);
};

}  // namespace hprlp
