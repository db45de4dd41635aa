// values.hip -- new matrix values for a resident solver (DESIGN.md "Matrix values", Solver::set_matrix_values): the check of the
// staged values, their scatter into A and A^T through the value maps, the gather of the five model vectors into the solver's
// numbering, and the two conversions of the map construction.  A translation unit of its own: the code objects of the iteration
// kernels do not change with it.
#include "values.h"

#include "common.h"
#include "kernels.h"

namespace hprlp {

namespace {

constexpr int kValuesMaxGrid = 4096;  // grid-stride passes: 16 workgroups per CU of 256, every lane a few entries at 1e8 nonzeros

inline unsigned grid_stride_blocks(long items) {
    const long g = (items + kThreads - 1) / kThreads;
    return static_cast<unsigned>(std::max<long>(1, std::min<long>(g, kValuesMaxGrid)));
}

// One pass over the staged values: the smallest position of a NaN or an infinity (atomicMin on a word that starts at ~0).
__global__ void __launch_bounds__(kThreads) k_values_check(const double *__restrict__ v, long n, unsigned long long *__restrict__ first_bad) {
    const long stride = static_cast<long>(gridDim.x) * kThreads;
    long mine = -1;
    for (long i = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const double a = v[i];
        if (!isfinite(a)) {
            mine = i;
            break;  // (a lane's positions ascend)
        }
    }
    if (mine >= 0) atomicMin(first_bad, static_cast<unsigned long long>(mine));
}

// Lane = two consecutive entries of each array: one 16-byte store per array (the value arrays come from hipMalloc, so entry 2 t
// is 16-byte aligned), an 8-byte load of the two map words, two scalar gathers from the staged values.  An odd last entry goes alone.
__global__ void __launch_bounds__(kThreads) k_values_in(long nnz, const double *__restrict__ stage, const int *__restrict__ mapA,
                                                       const int *__restrict__ mapAT, double *__restrict__ A_val,
                                                       double *__restrict__ AT_val) {
    const long pairs = (nnz + 1) >> 1;
    const long stride = static_cast<long>(gridDim.x) * kThreads;
    for (long t = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; t < pairs; t += stride) {
        const long e = 2 * t;
        if (e + 1 < nnz) {
            double2 a, b;
            if (mapA) {
                const int2 ma = *reinterpret_cast<const int2 *>(mapA + e);
                a.x = stage[ma.x];
                a.y = stage[ma.y];
            } else {
                a = *reinterpret_cast<const double2 *>(stage + e);
            }
            const int2 mt = *reinterpret_cast<const int2 *>(mapAT + e);
            b.x = stage[mt.x];
            b.y = stage[mt.y];
            *reinterpret_cast<double2 *>(A_val + e) = a;
            *reinterpret_cast<double2 *>(AT_val + e) = b;
        } else {
            A_val[e] = stage[mapA ? mapA[e] : e];
            AT_val[e] = stage[mapAT[e]];
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_vectors_in(VectorsInArgs a) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < a.m) {
        const int r = a.perm_r ? a.perm_r[i] : i;
        a.AL[i] = a.sAL[r];
        a.AU[i] = a.sAU[r];
    }
    if (i < a.n) {
        const int j = a.perm_c ? a.perm_c[i] : i;
        a.l[i] = a.sl[j];
        a.u[i] = a.su[j];
        a.c[i] = a.sc[j];
    }
}

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
