// batched.h -- solve_batched as the C boundary (abi.cpp) calls it; batched.hip.
#pragma once

#include <vector>

#include "hpr_rules.h"
#include "structs.h"

namespace hprlp {

// batched.hip: solve_batched with the infeasibility detection, member by member (DESIGN.md "Batched detection").  det null or
// off: exactly solve_batched.  certs (may be null) receives one Certificate per member, kind 0 where no verdict was reached.
// X0 (n x B) / Y0 (m x B), column-major, caller's units: warm start per member (DESIGN.md "Warm start"); both null: cold.
HPRLP_batched_results solve_batched_impl(const LP_info_cpu *model, int batch_size, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL,
                                         const HPRLP_FLOAT *AU, const HPRLP_FLOAT *l, const HPRLP_FLOAT *u,
                                         const HPRLP_FLOAT *obj_constants, const HPRLP_parameters *param, const Detection *det,
                                         std::vector<Certificate> *certs, const HPRLP_FLOAT *X0 = nullptr,
                                         const HPRLP_FLOAT *Y0 = nullptr);

// The resident solver behind hprlp_batched_solver_* (DESIGN.md "Resident batches"): the scaled shared matrix, the workspace of
// the last batch geometry and its captured graphs stay on the device from one batch to the next.  Every function throws on
// failure; a solve that refuses its arguments leaves the handle as it was.  param of a solve (null: the create's) supplies
// max_iter, stop_tol, time_limit, check_iter and use_bc_scaling only.  carry: start every member from the previous batch's
// solution of the same member, taken from the panels on the device (kb_carry_start).
struct BatchedSolver;
BatchedSolver *batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param);
void batched_solver_destroy(BatchedSolver *h);
void batched_solver_solve(BatchedSolver *h, int batch_size, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL, const HPRLP_FLOAT *AU,
                          const HPRLP_FLOAT *l, const HPRLP_FLOAT *u, const HPRLP_FLOAT *obj_constants, const HPRLP_parameters *param,
                          const HPRLP_FLOAT *X0, const HPRLP_FLOAT *Y0, bool carry, const Detection *det,
                          std::vector<Certificate> *certs, HPRLP_batched_results *out);
// Streamed batches (DESIGN.md "Streamed batches"; hprlp_batched_solver_solve_stream): count problems through min(width, count) slots, a
// finished member's slot taking the next queued problem at the same evaluation.  Host arrays, column-major rows x count.
void batched_solver_solve_stream(BatchedSolver *h, int count, int width, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL, const HPRLP_FLOAT *AU,
                                 const HPRLP_FLOAT *l, const HPRLP_FLOAT *u, const HPRLP_FLOAT *obj_constants, const HPRLP_parameters *param,
                                 const HPRLP_FLOAT *X0, const HPRLP_FLOAT *Y0, const Detection *det, std::vector<Certificate> *certs,
                                 HPRLP_batched_results *out);
int batched_solver_stream_record(const BatchedSolver *h, int *slot, int *event_in, int *event_out);  // returns count
void batched_solver_stream_info(const BatchedSolver *h, long out[8], double seconds[2]);              // either may be what is wanted (seconds null: not)
void batched_solver_lambda(const BatchedSolver *h, double out[2]);                                    // hprlp_batched_solver_lambda
// The device entry (DESIGN.md "Device-resident batches"): C .. Y0 are DEVICE arrays, column-major like the host entry's, ordered on
// `stream` (a hipStream_t); x / y / z are device buffers of n x B / m x B / n x B doubles that receive the solution in the
// caller's units; the members' scalars go to the host arrays below (B each, status 64 bytes per member; null: not wanted).
// Every pointer is checked against the runtime's records before anything is launched.
struct DeviceBatch {
    void *stream = nullptr;
    double *x = nullptr, *y = nullptr, *z = nullptr;
    double *primal_obj = nullptr, *residuals = nullptr, *gap = nullptr;
    int *iter = nullptr;
    char *status = nullptr;
    double time = 0.0, setup_time = 0.0, solve_time = 0.0, power_time = 0.0;
};
void batched_solver_solve_device(BatchedSolver *h, int batch_size, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL, const HPRLP_FLOAT *AU,
                                 const HPRLP_FLOAT *l, const HPRLP_FLOAT *u, const HPRLP_FLOAT *obj_constants /* host */,
                                 const HPRLP_parameters *param, const HPRLP_FLOAT *X0, const HPRLP_FLOAT *Y0, bool carry,
                                 const Detection *det, std::vector<Certificate> *certs, DeviceBatch *dev);
// The stream's device entry (DESIGN.md "Device-resident streams"; hprlp_batched_solver_solve_stream_device): the queue C .. Y0 as
// DEVICE arrays, column-major rows x count, ordered on dev->stream; dev's x / y / z take rows x count doubles, its host arrays count
// entries.  The queue is not staged: its scalars are taken where it lies, and a problem is scaled on its way into a slot.
void batched_solver_solve_stream_device(BatchedSolver *h, int count, int width, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL,
                                        const HPRLP_FLOAT *AU, const HPRLP_FLOAT *l, const HPRLP_FLOAT *u,
                                        const HPRLP_FLOAT *obj_constants /* host */, const HPRLP_parameters *param, const HPRLP_FLOAT *X0,
                                        const HPRLP_FLOAT *Y0, const Detection *det, std::vector<Certificate> *certs, DeviceBatch *dev);
void batched_solver_stream_memory(const BatchedSolver *h, long out[4]);  // hprlp_batched_solver_stream_memory
// A stream whose queued problems start from earlier ones' solutions (DESIGN.md "Streamed batches", "Parents";
// hprlp_batched_solver_solve_stream_parents and its device twin): parent is a HOST array of count entries in both.  dev null: the
// host entry (host arrays, the results into `out`); dev set: the device entry (device arrays, `out` unused).
void batched_solver_solve_stream_parents(BatchedSolver *h, int count, int width, const HPRLP_FLOAT *C, const HPRLP_FLOAT *AL,
                                         const HPRLP_FLOAT *AU, const HPRLP_FLOAT *l, const HPRLP_FLOAT *u, const HPRLP_FLOAT *obj_constants,
                                         const HPRLP_parameters *param, const HPRLP_FLOAT *X0, const HPRLP_FLOAT *Y0, const int *parent,
                                         const Detection *det, std::vector<Certificate> *certs, HPRLP_batched_results *out,
                                         DeviceBatch *dev);
// {roots, cold members, children started, slot-events a slot stood empty while problems waited} of the last stream call, a parents call
void batched_solver_stream_parents_info(const BatchedSolver *h, long out[4]);
// New values on the shared matrix' pattern (DESIGN.md "Matrix values"): val = the nnz values of the model's CSR in the caller's order.
// The shared solver takes them with zero vectors and is scaled again, the host's row / column norms and the created lambda_max
// follow; panels, staging blocks, order tables and workspace stay.  carry is refused until the next successful solve.
void batched_solver_set_matrix_values(BatchedSolver *h, const double *val, long nnz);
void batched_solver_set_norms(BatchedSolver *h, int rule);           // the HOST entry's norm rule (batch_prep.h): 0 reference, 1 tree
int batched_solver_scalars(const BatchedSolver *h, double *out);     // 7 x B of the last successful call; returns B
void batched_solver_transfer(const BatchedSolver *h, long out[4]);   // hprlp_batched_solver_transfer
void batched_solver_info(const BatchedSolver *h, long out[8]);       // hprlp_batched_solver_info
void batched_solver_seconds(const BatchedSolver *h, double out[6]);  // hprlp_batched_solver_seconds
// One ray test of the detection outside the loop, on the panels of the last successful solve (hprlp_batched_solver_ray_step):
// active (B ints), out (9 x B slots, slot-major), tested (B); 1 after a test, 0 where the iterate was only stored (restart).
int batched_solver_ray_step(BatchedSolver *h, const int *active, bool restart, double *out, int *tested);
// A panel of the last successful solve by name, column-major rows x B (hprlp_batched_solver_get_panel / _set_panel); X_bar and
// Y_bar alone can be written.
long batched_solver_get_panel(BatchedSolver *h, const char *name, double *out, long len);
void batched_solver_set_panel(BatchedSolver *h, const char *name, const double *in, long len);

}  // namespace hprlp
