// values.h -- new matrix values for a resident solver (DESIGN.md "Matrix values"): the kernels of values.hip and the host-only
// restatement of the value maps (values_host.cpp).  Private to the library; the C ABI is in include/hprlp_amd.h.
#pragma once

#include <hip/hip_runtime.h>

namespace hprlp {

// First non-finite entry of v[0 .. n): *first_bad receives its position, or is left at kValuesAllFinite (which the caller
// writes before the launch).
constexpr unsigned long long kValuesAllFinite = ~0ULL;
void launch_values_check(const double *v, long n, unsigned long long *first_bad, hipStream_t s);

// A_val[e] = stage[mapA[e]] and AT_val[k] = stage[mapAT[k]], e, k in [0, nnz); mapA null: the identity.
void launch_values_in(long nnz, const double *stage, const int *mapA, const int *mapAT, double *A_val, double *AT_val, hipStream_t s);

// The five model vectors in the solver's numbering: dst[i] = src[perm[i]] (perm null: dst[i] = src[i]).  perm_r serves AL, AU
// (m entries), perm_c serves l, u, c (n entries).
struct VectorsInArgs {
    int m, n;
    const double *sAL, *sAU, *sl, *su, *sc;  // staged, caller's numbering
    const int *perm_r, *perm_c;
    double *AL, *AU, *l, *u, *c;
};
void launch_vectors_in(const VectorsInArgs &a, hipStream_t s);

// Map construction: out[i] = i as a double (exact below 2^53), and the way back, out[i] = int(in[i]); an entry outside [0, n)
// raises *bad and is written as 0.
void launch_positions(double *out, long n, hipStream_t s);
void launch_positions_to_int(const double *in, long n, int *out, int *bad, hipStream_t s);

// Host only.  The value maps of a CSR pattern under a locality ordering (row_new2old / col_new2old, both null: none):
// mapA[e] = the caller's CSR position of entry e of P A Q with the columns of every row ascending (ties in the caller's order),
// mapAT[k] = the same for entry k of its row-stable transpose.  Throws on a malformed pattern or permutation.
void value_maps_host(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old, int *mapA,
                     int *mapAT);

}  // namespace hprlp
