// small.hip -- the HPR normal iterations of a SMALL LP (Netlib scale: nnz < 12288, m, n <= 2048,
// rows and columns of at most 256 nonzeros) as ONE persistent 1024-thread workgroup that runs `count`
// whole iterations per launch with everything on the chip.
//
// Why: on such an LP the regular path (k_spmv_fused, one launch per half-step) spends ~4 us per launch
// on the kernel boundary and three dependent trips to memory (tools/latency_probe.py: 8 us per
// iteration on config 2 whatever the block shape) for ~25 waves of work.  Here
//   * the matrix lives in REGISTERS, once: thread t owns entries [t*K, (t+1)*K) of A^T in CSR order as
//     {value, row i, column j, position of the same entry in the CSR order of A};
//   * y, x_hat and the products of the current half-step live in LDS;
//   * a row's data (x, c, l, u, last_x / y, AL, AU, last_y) lives in the registers of its owner thread;
//     rows are dealt to threads sorted by length, so the 64 lanes of a wave sum rows of similar length.
// A half-step is: every thread writes its products into LDS at their CSR position (of A^T for the
// x-half, of A for the y-half) -> LDS barrier -> every row owner adds its row's products in CSR order
// and applies the update -> LDS barrier.  No global memory is touched between the first and the last
// iteration of a launch.  Per row the arithmetic is the stream mode's (products summed sequentially in
// CSR order from 0; same update formulas as XEpi<false>/YEpi<false>::apply in kernels.hip), so the
// iterates are bit-identical to the regular kernels' (tests/test_gpu_small.py).
// Replaces, for this problem class, reference update_zx_normal_gpu / update_y_normal_gpu +
// advance_halpern_factors (src/main_iterate.cu:434-481,68-70) and the graph replay around them
// (src/HPRLP.cu:99-114,290-303).
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace hprlp {

namespace {

constexpr int NT = 1024;

// Product q lives at prod[pad(q)]: one spare slot per 32 keeps the lanes' stride-K writes (K = 8: 64-byte
// stride, 16 lanes on one bank pair) and the row owners' reads off the same LDS banks.
__device__ __forceinline__ int pad(int q) { return q + (q >> 5); }

// Sum of products [q0, q0+np) in index order.  The LDS reads are issued four at a time so that a long row
// costs one LDS latency per four entries instead of one per entry; the additions stay sequential.
__device__ __forceinline__ double seq_sum(const double *prod, int q0, int np) {
    double s = 0.0;
    int p = q0;
    const int end = q0 + np;
    for (; p + 4 <= end; p += 4) {
        const double a0 = prod[pad(p)], a1 = prod[pad(p + 1)], a2 = prod[pad(p + 2)], a3 = prod[pad(p + 3)];
        s += a0; s += a1; s += a2; s += a3;
    }
    if (p + 2 <= end) {
        const double a0 = prod[pad(p)], a1 = prod[pad(p + 1)];
        s += a0; s += a1;
        p += 2;
    }
    if (p < end) s += prod[pad(p)];
    return s;
}

// Returns w unchanged but opaque to the optimiser: LDS addresses derived from the packed per-entry words must be
// recomputed in every iteration (2 ALU ops) instead of being hoisted out of the iteration loop into 4 more
// registers per matrix entry -- that hoisting is what made the 12-entries-per-thread variant spill.
__device__ __forceinline__ unsigned int fresh(unsigned int w) {
    asm volatile("" : "+v"(w));
    return w;
}

__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The body of k_small_iterations and of k_small_iterations_many: one workgroup, `count` iterations of the LP `a` names.
// (Args: SmallArgs, or the same with its pointers typed as global memory -- see SmallArgsGlobal)
template <int KMAX, int R, class Args>
__device__ __forceinline__ void small_iterations_body(const Args &a, int K, int count) {
    static_assert(KMAX % 2 == 0, "positions are packed in pairs");
    __shared__ double prod[NT * KMAX + NT * KMAX / 32 + 1];
    __shared__ double ys[NT * R];
    __shared__ double xh[NT * R];
    const int t = threadIdx.x;

    // ---- this thread's matrix entries (A^T order): value, i | j << 16, position in A order (packed in pairs)
    double v[KMAX];
    unsigned int ij[KMAX], pa[KMAX / 2];
    const int e0 = t * K;
#pragma unroll
    for (int k = 0; k < KMAX; k += 2) {
        const int q0 = e0 + k, q1 = q0 + 1;
        const bool on0 = k < K && q0 < a.nnz, on1 = k + 1 < K && q1 < a.nnz;
        v[k] = on0 ? a.AT_val[q0] : 0.0;
        v[k + 1] = on1 ? a.AT_val[q1] : 0.0;
        ij[k] = on0 ? static_cast<unsigned int>(a.ent_ij[q0]) : 0u;
        ij[k + 1] = on1 ? static_cast<unsigned int>(a.ent_ij[q1]) : 0u;
        // entries beyond the end park their products in the last slot of prod, which no row reads (nnz < NT*KMAX)
        const unsigned int park = static_cast<unsigned int>(NT * KMAX - 1);
        const unsigned int p0 = on0 ? static_cast<unsigned int>(a.ent_posA[q0]) : park;
        const unsigned int p1 = on1 ? static_cast<unsigned int>(a.ent_posA[q1]) : park;
        pa[k >> 1] = p0 | (p1 << 16);
    }

    // ---- rows owned by this thread: slots t + NT*q of the rows sorted by length
    double xi[R], ci[R], li[R], ui[R], lx[R], yi[R], lo[R], hi[R], ly[R];
    unsigned int xseg[R], yseg[R];  // first product | count << 16 (first < 12288, count <= 256)
    unsigned int own[R];            // row j of A^T | row i of A << 16 (0xffff: none)
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int slot = t + NT * q;
        const bool on = slot < a.n, oni = slot < a.m;
        const int j = on ? a.order_x[slot] : 0, i = oni ? a.order_y[slot] : 0;
        own[q] = static_cast<unsigned int>(on ? j : 0xffff) | (static_cast<unsigned int>(oni ? i : 0xffff) << 16);
        xi[q] = on ? a.x[j] : 0.0;
        ci[q] = on ? a.c[j] : 0.0;
        li[q] = on ? a.l[j] : 0.0;
        ui[q] = on ? a.u[j] : 0.0;
        lx[q] = on ? a.last_x[j] : 0.0;
        const int xs = on ? a.AT_rowptr[j] : 0, xe = on ? a.AT_rowptr[j + 1] : 0;
        xseg[q] = static_cast<unsigned int>(xs) | (static_cast<unsigned int>(xe - xs) << 16);
        yi[q] = oni ? a.y[i] : 0.0;
        lo[q] = oni ? a.AL[i] : 0.0;
        hi[q] = oni ? a.AU[i] : 0.0;
        ly[q] = oni ? a.last_y[i] : 0.0;
        const int ysb = oni ? a.A_rowptr[i] : 0, ye = oni ? a.A_rowptr[i + 1] : 0;
        yseg[q] = static_cast<unsigned int>(ysb) | (static_cast<unsigned int>(ye - ysb) << 16);
        if (oni) ys[i] = yi[q];
        if (on) xh[j] = 0.0;
    }
    const double sigma = a.ctrl->sigma, fact1 = a.ctrl->lam_sigma, fact2 = a.ctrl->inv_lam_sigma;
    const int k0 = a.ctrl->kx;
    __syncthreads();

    for (int it = 0; it < count; ++it) {
        const double f1 = 1.0 / (static_cast<double>(k0 + it) + 2.0), f2 = 1.0 - f1;
        // ---- x-half: products of A^T y in A^T order (this thread's own consecutive slots)
#pragma unroll
        for (int k = 0; k < KMAX; k += 2) {
            const double g0 = ys[fresh(ij[k]) & 0xffffu], g1 = ys[fresh(ij[k + 1]) & 0xffffu];
            const int qq = static_cast<int>(fresh(static_cast<unsigned int>(e0))) + k;
            if (k < K) prod[pad(qq)] = v[k] * g0;
            if (k + 1 < K) prod[pad(qq + 1)] = v[k + 1] * g1;
        }
        lds_sync();
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const double s = seq_sum(prod, static_cast<int>(xseg[q] & 0xffffu), static_cast<int>(xseg[q] >> 16));
            // same operations as XEpi<false>::apply
            const double gc = s - ci[q];
            const double zt = xi[q] + sigma * gc;
            const double xb = fmin(ui[q], fmax(li[q], zt));
            const double h = 2.0 * xb - xi[q];
            xi[q] = f2 * h + f1 * lx[q];
            if ((own[q] & 0xffffu) != 0xffffu) xh[own[q] & 0xffffu] = h;
        }
        lds_sync();
        // ---- y-half: products of A x_hat, scattered to their position in the CSR order of A
        // (the y-half of iteration k uses the same Halpern factors)
#pragma unroll
        for (int k = 0; k < KMAX; k += 2) {
            const double g0 = xh[fresh(ij[k]) >> 16], g1 = xh[fresh(ij[k + 1]) >> 16];
            const unsigned int pp = fresh(pa[k >> 1]);
            prod[pad(static_cast<int>(pp & 0xffffu))] = v[k] * g0;
            prod[pad(static_cast<int>(pp >> 16))] = v[k + 1] * g1;
        }
        lds_sync();
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const double s = seq_sum(prod, static_cast<int>(yseg[q] & 0xffffu), static_cast<int>(yseg[q] >> 16));
            // same operations as YEpi<false>::apply
            const double w = s - fact1 * yi[q];
            const double d = fmax(lo[q] - w, fmin(hi[q] - w, 0.0));
            const double yb = fact2 * d;
            const double yh = 2.0 * yb - yi[q];
            yi[q] = f2 * yh + f1 * ly[q];
            if ((own[q] >> 16) != 0xffffu) ys[own[q] >> 16] = yi[q];
        }
        lds_sync();
    }

#pragma unroll
    for (int q = 0; q < R; ++q) {
        const unsigned int j = own[q] & 0xffffu, i = own[q] >> 16;
        if (j != 0xffffu) {
            a.x[j] = xi[q];
            a.x_hat[j] = xh[j];
        }
        if (i != 0xffffu) a.y[i] = yi[q];
    }
    if (t == 0 && count > 0) {
        a.ctrl->kx = k0 + count;
        a.ctrl->ky = k0 + count - 1;
    }
}

template <int KMAX, int R>
__global__ void __launch_bounds__(NT) k_small_iterations(SmallArgs a, int K, int count) {
    small_iterations_body<KMAX, R>(a, K, count);
}

// A pointer read from a task list is a generic one to the compiler (a kernel argument it knows to be global memory): every access
// through it would be a flat one with a 64-bit address register pair, and the <12, 2> instance would spill.  The group kernels
// therefore hand the body the same arguments typed as global memory.
#define HPRLP_GLOBAL __attribute__((address_space(1)))
struct SmallArgsGlobal {
    int m, n, nnz;
    const HPRLP_GLOBAL int *A_rowptr, *AT_rowptr;
    const HPRLP_GLOBAL double *AT_val;
    const HPRLP_GLOBAL int *ent_ij, *ent_posA, *order_x, *order_y;
    HPRLP_GLOBAL double *x, *x_hat, *y;
    const HPRLP_GLOBAL double *l, *u, *c, *last_x, *AL, *AU, *last_y;
    HPRLP_GLOBAL Ctrl *ctrl;
};
template <class T>
__device__ __forceinline__ HPRLP_GLOBAL T *as_global(T *p) {
    return (HPRLP_GLOBAL T *)p;
}
__device__ __forceinline__ SmallArgsGlobal global_args(const SmallArgs &a) {
    return SmallArgsGlobal{a.m, a.n, a.nnz, as_global(a.A_rowptr), as_global(a.AT_rowptr), as_global(a.AT_val), as_global(a.ent_ij),
                           as_global(a.ent_posA), as_global(a.order_x), as_global(a.order_y), as_global(a.x), as_global(a.x_hat),
                           as_global(a.y), as_global(a.l), as_global(a.u), as_global(a.c), as_global(a.last_x), as_global(a.AL),
                           as_global(a.AU), as_global(a.last_y), as_global(a.ctrl)};
}

// Many small LPs at once (DESIGN.md "Many small LPs"): workgroup b runs task b exactly as k_small_iterations would -- the same body
// on the same arguments, so a member's iterates are the single launch's bits.  The task is uniform in the workgroup and is read
// before anything is stored (scalar loads into a private copy).  No workgroup reads what another writes; a task without
// iterations touches nothing.
template <int KMAX, int R>
__global__ void __launch_bounds__(NT) k_small_iterations_many(const SmallIterTask *__restrict__ tasks) {
    const SmallIterTask task = tasks[blockIdx.x];
    if (task.count <= 0) return;
    small_iterations_body<KMAX, R>(global_args(task.a), task.K, task.count);
}

// ------------------------------------------------------------------------------------------------
// The power iteration of a small LP (reference power_method_cusparse, src/power_iteration.cu:20-119) in ONE launch of the
// same single workgroup: q = z / sqrt(z.z + eps), z = A (A^T q), every 10th iteration lambda = q.z and the stopping test
// |z - lambda q| < tol -- decided on the device, so the host neither launches 6 kernels per iteration nor waits for the
// stream every 10th (config 2: 600 iterations, 10 ms -> 2 ms).  Same row sums as the regular kernels (products added in
// CSR order); the three dot products are added in a fixed tree order (thread, wave shuffle, 16 wave sums), i.e. they
// agree with the oracle's sequential sums to rounding.  out = {lambda, iterations done}.
// ------------------------------------------------------------------------------------------------
template <int KMAX, int R, bool TIGHT, class Args, class In, class Out>
__device__ __forceinline__ void small_power_body(const Args &a, int K, In z0, int max_iter, double tol, Out out) {
    auto fr = [](unsigned int w) { return TIGHT ? fresh(w) : w; };
    __shared__ double prod[NT * KMAX + NT * KMAX / 32 + 1];
    __shared__ double qs[NT * R];   // q (length m), gathered by the products of A^T q
    __shared__ double gs[NT * R];   // A^T q (length n), gathered by the products of A (A^T q)
    __shared__ double red[2][3][NT / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double v[KMAX];
    unsigned int ij[KMAX], pa[KMAX / 2];
    const int e0 = t * K;
#pragma unroll
    for (int k = 0; k < KMAX; k += 2) {
        const int q0 = e0 + k, q1 = q0 + 1;
        const bool on0 = k < K && q0 < a.nnz, on1 = k + 1 < K && q1 < a.nnz;
        v[k] = on0 ? a.AT_val[q0] : 0.0;
        v[k + 1] = on1 ? a.AT_val[q1] : 0.0;
        ij[k] = on0 ? static_cast<unsigned int>(a.ent_ij[q0]) : 0u;
        ij[k + 1] = on1 ? static_cast<unsigned int>(a.ent_ij[q1]) : 0u;
        const unsigned int park = static_cast<unsigned int>(NT * KMAX - 1);
        const unsigned int p0 = on0 ? static_cast<unsigned int>(a.ent_posA[q0]) : park;
        const unsigned int p1 = on1 ? static_cast<unsigned int>(a.ent_posA[q1]) : park;
        pa[k >> 1] = p0 | (p1 << 16);
    }
    double z[R];
    unsigned int xseg[R], yseg[R], own[R];
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int slot = t + NT * q;
        const bool on = slot < a.n, oni = slot < a.m;
        const int j = on ? a.order_x[slot] : 0, i = oni ? a.order_y[slot] : 0;
        own[q] = static_cast<unsigned int>(on ? j : 0xffff) | (static_cast<unsigned int>(oni ? i : 0xffff) << 16);
        const int xs = on ? a.AT_rowptr[j] : 0, xe = on ? a.AT_rowptr[j + 1] : 0;
        xseg[q] = static_cast<unsigned int>(xs) | (static_cast<unsigned int>(xe - xs) << 16);
        const int ysb = oni ? a.A_rowptr[i] : 0, ye = oni ? a.A_rowptr[i + 1] : 0;
        yseg[q] = static_cast<unsigned int>(ysb) | (static_cast<unsigned int>(ye - ysb) << 16);
        z[q] = oni ? z0[i] : 0.0;
        part += z[q] * z[q];
    }
    // block sums of up to three values, identical in every thread: thread partial -> wave shuffle -> the 16 wave sums in order
    int flip = 0;
    auto block_sum3 = [&](double &s0, double &s1, double &s2) {
        const double w0 = wave_sum64(s0), w1 = wave_sum64(s1), w2 = wave_sum64(s2);
        if (lane == 0) {
            red[flip][0][wave] = w0;
            red[flip][1][wave] = w1;
            red[flip][2][wave] = w2;
        }
        lds_sync();
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            r0 += red[flip][0][w];
            r1 += red[flip][1][w];
            r2 += red[flip][2][w];
        }
        flip ^= 1;  // the next sum writes the other buffer: no barrier needed before it
        s0 = r0; s1 = r1; s2 = r2;
    };
    double zz = part, d1 = 0.0, d2 = 0.0;
    block_sum3(zz, d1, d2);
    double lambda = 1.0;
    int done = max_iter;
    for (int it = 1; it <= max_iter; ++it) {
        const double invn = 1.0 / sqrt(zz + 2.220446049250313e-16);
        double qv[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            qv[q] = invn * z[q];
            if ((own[q] >> 16) != 0xffffu) qs[own[q] >> 16] = qv[q];
        }
        lds_sync();
        // A^T q: products in A^T order, row sums in CSR order
#pragma unroll
        for (int k = 0; k < KMAX; k += 2) {
            const double g0 = qs[fresh(ij[k]) & 0xffffu], g1 = qs[fresh(ij[k + 1]) & 0xffffu];
            const int qq = static_cast<int>(fresh(static_cast<unsigned int>(e0))) + k;
            if (k < K) prod[pad(qq)] = v[k] * g0;
            if (k + 1 < K) prod[pad(qq + 1)] = v[k + 1] * g1;
        }
        lds_sync();
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const double sx = seq_sum(prod, static_cast<int>(fr(xseg[q]) & 0xffffu), static_cast<int>(fr(xseg[q]) >> 16));
            if ((own[q] & 0xffffu) != 0xffffu) gs[own[q] & 0xffffu] = sx;
        }
        lds_sync();
        // A (A^T q): products scattered to their position in the CSR order of A
#pragma unroll
        for (int k = 0; k < KMAX; k += 2) {
            const double g0 = gs[fresh(ij[k]) >> 16], g1 = gs[fresh(ij[k + 1]) >> 16];
            const unsigned int pp = fresh(pa[k >> 1]);
            prod[pad(static_cast<int>(pp & 0xffffu))] = v[k] * g0;
            prod[pad(static_cast<int>(pp >> 16))] = v[k + 1] * g1;
        }
        lds_sync();
        double pzz = 0.0, pqz = 0.0;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const double sy = seq_sum(prod, static_cast<int>(fr(yseg[q]) & 0xffffu), static_cast<int>(fr(yseg[q]) >> 16));
            z[q] = (own[q] >> 16) != 0xffffu ? sy : 0.0;
            pzz += z[q] * z[q];
            pqz += z[q] * qv[q];
        }
        double dummy = 0.0;
        block_sum3(pzz, pqz, dummy);
        zz = pzz;
        if (it % 10 == 0) {
            lambda = pqz;
            double pe = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const double d = -lambda * qv[q] + 1.0 * z[q];
                pe += d * d;
            }
            block_sum3(pe, u1, u2);
            if (sqrt(pe) < tol) {  // (the same value in every thread: a uniform exit)
                done = it;
                break;
            }
        }
    }
    if (t == 0) {
        out[0] = lambda;
        out[1] = static_cast<double>(done);
    }
}

template <int KMAX, int R>
__global__ void __launch_bounds__(NT) k_small_power(SmallArgs a, int K, const double *__restrict__ z0, int max_iter, double tol,
                                                   double *__restrict__ out) {
    small_power_body<KMAX, R, false>(a, K, z0, max_iter, tol, out);
}

// workgroup b runs the power iteration of task b (its own start vector, limit, tolerance and output) as k_small_power would
template <int KMAX, int R>
__global__ void __launch_bounds__(NT) k_small_power_many(const SmallPowerTask *__restrict__ tasks) {
    const SmallPowerTask task = tasks[blockIdx.x];
    small_power_body<KMAX, R, true>(global_args(task.a), task.K, as_global(task.z0), task.max_iter, task.tol, as_global(task.out));
}

template <int KMAX, int R>
void launch_power_kr(const SmallArgs &a, const double *z0, int max_iter, double tol, double *out, hipStream_t s) {
    const int K = (a.nnz + NT - 1) / NT;
    hipLaunchKernelGGL((k_small_power<KMAX, R>), dim3(1), dim3(NT), 0, s, a, K, z0, max_iter, tol, out);
    HIP_CHECK(hipGetLastError());  // (the <12, 2> instance holds about 135 KB of static LDS: a refused launch must not pass silently)
}

template <int KMAX, int R>
void launch_kr(const SmallArgs &a, int count, hipStream_t s) {
    const int K = (a.nnz + NT - 1) / NT;
    hipLaunchKernelGGL((k_small_iterations<KMAX, R>), dim3(1), dim3(NT), 0, s, a, K, count);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

bool small_path_fits(int m, int n, long nnz, int max_row_A, int max_row_AT) {
    return m >= 1 && n >= 1 && m <= NT * kSmallMaxR && n <= NT * kSmallMaxR && nnz >= 1 &&
           nnz < static_cast<long>(NT) * kSmallMaxK && max_row_A <= kSmallMaxRow && max_row_AT <= kSmallMaxRow;
}

void launch_small_power(const SmallArgs &a, const double *z0, int max_iter, double tol, double *out, hipStream_t s) {
    const int K = (a.nnz + NT - 1) / NT;
    const int R = (std::max(a.m, a.n) + NT - 1) / NT;
    if (K <= 4 && R <= 1) launch_power_kr<4, 1>(a, z0, max_iter, tol, out, s);
    else if (K <= 4) launch_power_kr<4, 2>(a, z0, max_iter, tol, out, s);
    else if (K <= 8 && R <= 1) launch_power_kr<8, 1>(a, z0, max_iter, tol, out, s);
    else if (K <= 8) launch_power_kr<8, 2>(a, z0, max_iter, tol, out, s);
    else if (R <= 1) launch_power_kr<12, 1>(a, z0, max_iter, tol, out, s);
    else launch_power_kr<12, 2>(a, z0, max_iter, tol, out, s);
}

void launch_small_iterations(const SmallArgs &a, int count, hipStream_t s) {
    if (count <= 0) return;
    // instantiated by entries / rows per thread so that small problems do not carry the registers of big ones
    const int K = (a.nnz + NT - 1) / NT;
    const int R = (std::max(a.m, a.n) + NT - 1) / NT;
    if (K <= 4 && R <= 1) launch_kr<4, 1>(a, count, s);
    else if (K <= 4) launch_kr<4, 2>(a, count, s);
    else if (K <= 8 && R <= 1) launch_kr<8, 1>(a, count, s);
    else if (K <= 8) launch_kr<8, 2>(a, count, s);
    else if (R <= 1) launch_kr<12, 1>(a, count, s);
    else launch_kr<12, 2>(a, count, s);
}

// ---- task lists of the group launches ------------------------------------------------------------------------------------
SmallTaskBuf::~SmallTaskBuf() {
    if (copied) (void)hipEventDestroy(copied);
    if (host) (void)hipHostFree(host);
    if (dev) (void)hipFree(dev);
}

void *SmallTaskBuf::stage(size_t bytes) {
    if (!copied) HIP_CHECK(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    else HIP_CHECK(hipEventSynchronize(copied));  // the previous list has left the staging block (long ago, as a rule)
    if (bytes > cap) {
        // (the device copy may still be read by the previous launch: hipFree waits for the device)
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        host = dev = nullptr;
        cap = 0;
        const size_t want = std::max(bytes, static_cast<size_t>(1) << 14);
        HIP_CHECK(hipHostMalloc(&host, want, hipHostMallocDefault));
        HIP_CHECK(hipMalloc(&dev, want));
        cap = want;
    }
    return host;
}

void SmallTaskBuf::send(size_t bytes, hipStream_t s) {
    HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(copied, s));
}

namespace {

// the <KMAX, R> class of an LP, in the order of the if-chains of launch_small_iterations / launch_small_power
int small_class(const SmallArgs &a) {
    const int K = (a.nnz + NT - 1) / NT;
    const int R = (std::max(a.m, a.n) + NT - 1) / NT;
    if (K <= 4 && R <= 1) return 0;
    if (K <= 4) return 1;
    if (K <= 8 && R <= 1) return 2;
    if (K <= 8) return 3;
    if (R <= 1) return 4;
    return 5;
}

void check_small_task(const SmallArgs &a) {
    // the kernels index LDS by these: a task outside the small path's limits must never reach them
    if (a.m < 1 || a.n < 1 || a.m > NT * kSmallMaxR || a.n > NT * kSmallMaxR || a.nnz < 1 || a.nnz >= NT * kSmallMaxK)
        throw std::runtime_error("a task of a group launch is outside the small path's limits");
}

// tasks -> staging block, grouped by class (stable), K filled in; first[c] .. first[c + 1] is class c's range
template <class Task, class Keep>
int stage_tasks(const Task *tasks, int ntasks, SmallTaskBuf &buf, int first[7], Keep keep) {
    int per[6] = {0, 0, 0, 0, 0, 0}, total = 0;
    for (int k = 0; k < ntasks; ++k)
        if (keep(tasks[k])) {
            check_small_task(tasks[k].a);
            ++per[small_class(tasks[k].a)];
            ++total;
        }
    first[0] = 0;
    for (int c = 0; c < 6; ++c) first[c + 1] = first[c] + per[c];
    if (total == 0) return 0;
    Task *st = static_cast<Task *>(buf.stage(sizeof(Task) * static_cast<size_t>(total)));
    int at[6];
    for (int c = 0; c < 6; ++c) at[c] = first[c];
    for (int k = 0; k < ntasks; ++k)
        if (keep(tasks[k])) {
            Task t = tasks[k];
            t.K = (t.a.nnz + NT - 1) / NT;
            st[at[small_class(t.a)]++] = t;
        }
    return total;
}

template <int KMAX, int R>
int launch_iterations_many_kr(const SmallIterTask *dev, int first, int count, hipStream_t s) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL((k_small_iterations_many<KMAX, R>), dim3(count), dim3(NT), 0, s, dev + first);
    HIP_CHECK(hipGetLastError());  // (as launch_kr: a refused launch must not pass silently)
    return 1;
}

template <int KMAX, int R>
int launch_power_many_kr(const SmallPowerTask *dev, int first, int count, hipStream_t s) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL((k_small_power_many<KMAX, R>), dim3(count), dim3(NT), 0, s, dev + first);
    HIP_CHECK(hipGetLastError());
    return 1;
}

}  // namespace

int launch_small_iterations_many(const SmallIterTask *tasks, int ntasks, SmallTaskBuf &buf, hipStream_t s) {
    int first[7];
    const int total = stage_tasks(tasks, ntasks, buf, first, [](const SmallIterTask &t) { return t.count > 0; });
    if (total == 0) return 0;
    buf.send(sizeof(SmallIterTask) * static_cast<size_t>(total), s);
    const SmallIterTask *d = static_cast<const SmallIterTask *>(buf.dev);
    return launch_iterations_many_kr<4, 1>(d, first[0], first[1] - first[0], s) + launch_iterations_many_kr<4, 2>(d, first[1], first[2] - first[1], s) +
           launch_iterations_many_kr<8, 1>(d, first[2], first[3] - first[2], s) + launch_iterations_many_kr<8, 2>(d, first[3], first[4] - first[3], s) +
           launch_iterations_many_kr<12, 1>(d, first[4], first[5] - first[4], s) + launch_iterations_many_kr<12, 2>(d, first[5], first[6] - first[5], s);
}

int launch_small_power_many(const SmallPowerTask *tasks, int ntasks, SmallTaskBuf &buf, hipStream_t s) {
    int first[7];
    const int total = stage_tasks(tasks, ntasks, buf, first, [](const SmallPowerTask &) { return true; });
    if (total == 0) return 0;
    buf.send(sizeof(SmallPowerTask) * static_cast<size_t>(total), s);
    const SmallPowerTask *d = static_cast<const SmallPowerTask *>(buf.dev);
    return launch_power_many_kr<4, 1>(d, first[0], first[1] - first[0], s) + launch_power_many_kr<4, 2>(d, first[1], first[2] - first[1], s) +
           launch_power_many_kr<8, 1>(d, first[2], first[3] - first[2], s) + launch_power_many_kr<8, 2>(d, first[3], first[4] - first[3], s) +
           launch_power_many_kr<12, 1>(d, first[4], first[5] - first[4], s) + launch_power_many_kr<12, 2>(d, first[5], first[6] - first[5], s);
}

// warm-up (abi.cpp: hprlp_warmup): an attribute query makes the runtime load this translation unit's code object now instead
// of at the first launch of one of its kernels
void warm_small_tu() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>((&k_small_iterations<4, 1>)));
}

}  // namespace hprlp
