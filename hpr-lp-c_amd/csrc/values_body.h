// values_body.h -- the bodies of the three kernels that bring new matrix values in (values.hip: k_values_check, k_values_in,
// k_vectors_in), where both values.hip and the group launches of kernels.hip see them.  A body runs as workgroup `bid` of a grid
// of `grid` workgroups: the single kernels pass blockIdx.x / gridDim.x, a group launch the member's own numbers (kernels.hip:
// ValuesCheckTask, ValuesInTask, VectorsInTask).  Device code: included by the two translation units only.
#pragma once

#include <algorithm>

#include "common.h"
#include "values.h"

namespace hprlp {

constexpr int kValuesMaxGrid = 4096;  // grid-stride passes: 16 workgroups per CU of 256, every lane a few entries at 1e8 nonzeros

inline unsigned grid_stride_blocks(long items) {
    const long g = (items + kThreads - 1) / kThreads;
    return static_cast<unsigned>(std::max<long>(1, std::min<long>(g, kValuesMaxGrid)));
}

// One pass over the staged values: the smallest position of a NaN or an infinity (atomicMin on a word that starts at ~0; a
// minimum does not depend on the order in which the lanes arrive).
__device__ __forceinline__ void values_check_body(const double *__restrict__ v, long n, unsigned long long *__restrict__ first_bad, unsigned bid,
                                                  unsigned grid) {
    const long stride = static_cast<long>(grid) * kThreads;
    long mine = -1;
    for (long i = static_cast<long>(bid) * kThreads + threadIdx.x; i < n; i += stride) {
        const double a = v[i];
        if (!isfinite(a)) {
            mine = i;
            break;  // (a lane's positions ascend)
        }
    }
    if (mine >= 0) atomicMin(first_bad, static_cast<unsigned long long>(mine));
}

// Lane = two consecutive entries of each array: one 16-byte store per array (the value arrays come from hipMalloc or from a
// group's arena, 256-byte aligned both, so entry 2 t is 16-byte aligned), an 8-byte load of the two map words, two scalar gathers
// from the staged values.  An odd last entry goes alone.
__device__ __forceinline__ void values_in_body(long nnz, const double *__restrict__ stage, const int *__restrict__ mapA,
                                               const int *__restrict__ mapAT, double *__restrict__ A_val, double *__restrict__ AT_val, unsigned bid,
                                               unsigned grid) {
    const long pairs = (nnz + 1) >> 1;
    const long stride = static_cast<long>(grid) * kThreads;
    for (long t = static_cast<long>(bid) * kThreads + threadIdx.x; t < pairs; t += stride) {
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

__device__ __forceinline__ void vectors_in_body(const VectorsInArgs &a, unsigned bid) {
    const int i = bid * kThreads + threadIdx.x;
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

}  // namespace hprlp
