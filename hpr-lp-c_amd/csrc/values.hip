// values.hip -- new matrix values for a resident solver (DESIGN.md "Matrix values", Solver::set_matrix_values): the check of the
// staged values, their scatter into A and A^T through the value maps, the gather of the five model vectors into the solver's
// numbering, and the two conversions of the map construction.  The first three are wrappers of the bodies in values_body.h, which
// the group launches run as well (kernels.hip).  A translation unit of its own: the code objects of the iteration
// kernels do not change with it.
#include "values.h"

#include "common.h"
#include "kernels.h"
#include "values_body.h"

namespace hprlp {

namespace {

__global__ void __launch_bounds__(kThreads) k_values_check(const double *__restrict__ v, long n, unsigned long long *__restrict__ first_bad) {
    values_check_body(v, n, first_bad, blockIdx.x, gridDim.x);
}

__global__ void __launch_bounds__(kThreads) k_values_in(long nnz, const double *__restrict__ stage, const int *__restrict__ mapA,
                                                       const int *__restrict__ mapAT, double *__restrict__ A_val,
                                                       double *__restrict__ AT_val) {
    values_in_body(nnz, stage, mapA, mapAT, A_val, AT_val, blockIdx.x, gridDim.x);
}

__global__ void __launch_bounds__(kThreads) k_vectors_in(VectorsInArgs a) { vectors_in_body(a, blockIdx.x); }

__global__ void __launch_bounds__(kThreads) k_positions(double *__restrict__ out, long n) {
    const long stride = static_cast<long>(gridDim.x) * kThreads;
    for (long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) out[i] = static_cast<double>(i);
}

__global__ void __launch_bounds__(kThreads) k_positions_to_int(const double *__restrict__ in, long n, int *__restrict__ out,
                                                              int *__restrict__ bad) {
    const long stride = static_cast<long>(gridDim.x) * kThreads;
    for (long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const double p = in[i];
        const bool ok = p >= 0.0 && p < static_cast<double>(n);
        if (!ok) atomicOr(bad, 1);
        out[i] = ok ? static_cast<int>(p) : 0;
    }
}

}  // namespace

void launch_values_check(const double *v, long n, unsigned long long *first_bad, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_values_check, dim3(grid_stride_blocks(n)), dim3(kThreads), 0, s, v, n, first_bad);
}

void launch_values_in(long nnz, const double *stage, const int *mapA, const int *mapAT, double *A_val, double *AT_val, hipStream_t s) {
    if (nnz <= 0) return;
    hipLaunchKernelGGL(k_values_in, dim3(grid_stride_blocks((nnz + 1) / 2)), dim3(kThreads), 0, s, nnz, stage, mapA, mapAT, A_val, AT_val);
}

void launch_vectors_in(const VectorsInArgs &a, hipStream_t s) {
    const int len = std::max(a.m, a.n);
    if (len <= 0) return;
    hipLaunchKernelGGL(k_vectors_in, dim3((len + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
}

void launch_positions(double *out, long n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_positions, dim3(grid_stride_blocks(n)), dim3(kThreads), 0, s, out, n);
}

void launch_positions_to_int(const double *in, long n, int *out, int *bad, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_positions_to_int, dim3(grid_stride_blocks(n)), dim3(kThreads), 0, s, in, n, out, bad);
}

}  // namespace hprlp
