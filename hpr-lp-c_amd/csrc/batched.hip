// batched.hip -- solve_batched: B linear programs that share the sparse matrix A, solved together on
// one MI355X.  Replaces reference src/batched_solver.cu (kernels :122-323, SpMM wrappers :428-477,
// loop :1017-1084, host restart/sigma logic :667-762, set-up :792-885, results :887-935).
//
// Layout: the batch (padded to Bp = a power of two <= 64, or a multiple of 64) is cut into chunks of Bc problems
// (Bc = Bp below 64, else 8..64: choose_chunk); a panel of `rows` rows is stored chunk after chunk, each chunk
// ROW-major in the batch index: element (row j, problem k) lives at P[((k / Bc) * rows + j) * Bc + k % Bc].
// A gathered row of a chunk is one contiguous Bc*8-byte run: the SpMM is a CSR row loop in which a lane follows
// one problem, 64 / Bc rows per wave.  A workgroup works on ONE chunk, chunk = blockIdx.x % (number of chunks):
// workgroups go round-robin to the 8 XCDs, so with 8 chunks every XCD gathers from the same eighth of the
// gathered panel (config 4: 2.2 MB of Y instead of 17 MB -- it stays in the XCD's 4 MiB L2).  Each problem's row sums are accumulated sequentially in CSR order, exactly like
// the single-LP stream kernel, so the result is bit-identical to the oracle's batched restatement (held to it iterate by
// iterate up to the first restart, and within the oracle's own sensitivity after, by tests/test_gpu_batched_kernels.py).
// The half-step update (projection, reflection, Halpern average, per-problem sigma / inner counter /
// active mask) is fused into the SpMM epilogue: one launch per half-step, no per-iteration host sync
// (the reference synchronises the stream and uploads 2B doubles every iteration, :1070-1073).
// The MFMA f64 tile (v_mfma_f64_16x16x4) is not used: with ~2-7 nonzeros per row there is no dense
// A-tile to feed it and the kernel is bound by panel traffic, not by FMA rate.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <type_traits>
#include <utility>

#include "HPRLP.h"
#include "batch_prep.h"
#include "batched.h"
#include "env.h"
#include "solver.h"
#include "stream_schedule.h"

namespace hprlp {
namespace {

enum BSlot : int {  // per-problem scalar slots, SC[slot*Bp + k]
    B_CX = 0, B_YOBJ_Y, B_XZ, B_RD2, B_RP2, B_ADX_DY, B_DY2, B_DX2, B_MOVE_X2, B_MOVE_Y2, B_LU2, B_NSLOT
};
enum BRaySlot : int {  // infeasibility detection only, after the slots above: kb_ray_form's six, kb_ray_col's two, kb_ray_row's one
    B_RAY_DY = B_NSLOT, B_RAY_CD, B_RAY_VY, B_RAY_WD, B_RAY_YN, B_RAY_DN, B_RAY_DZ, B_RAY_VZ, B_RAY_WQ, B_NSLOT_DETECT
};

struct BatchCtl {  // per-problem device scalars
    double *sigma;
    int *active;
    int *kx, *ky;
    int *restart_flag;
};

// which chunk / which block of rows a workgroup works on (1-D grids of nchunk * row blocks, chunk fastest)
struct Blk {
    int chunk, rb, nrb;
};
__device__ __forceinline__ Blk decode_block(const Geo &g) {
    Blk b;
    b.chunk = blockIdx.x % g.nchunk;
    b.rb = blockIdx.x / g.nchunk;
    b.nrb = gridDim.x / g.nchunk;
    return b;
}
// element (row r, local problem kl) of a chunk of a panel with `rows` rows
__device__ __forceinline__ size_t pidx(const Geo &g, int chunk, int rows, int r, int kl) {
    return (static_cast<size_t>(chunk) * rows + r) * g.Bw + kl;
}

// Sum `NACC` per-thread accumulators over all threads of the block that share a problem index and
// store them to partials[(rb * NACC + i) * Bp + k] (rb: the workgroup's row block).  The last NMAX accumulators are
// nonnegative maxima (the infeasibility detection's violations) and combine with fmax.  Fixed order => deterministic.
template <int NACC, int NMAX = 0>
__device__ __forceinline__ void block_store_per_problem(double (&acc)[NACC], const Geo &g, int rb, int k, bool kvalid,
                                                        double *partials) {
    __shared__ double red[4][NACC][64];
    constexpr int kSums = NACC - NMAX;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
        double v = acc[i];
        for (int off = 32; off >= g.Bw; off >>= 1) {  // combine sub-rows of the wave
            const double o = __shfl_xor(v, off, 64);
            v = i < kSums ? v + o : fmax(v, o);
        }
        red[wave][i][lane] = v;
    }
    __syncthreads();
    if (wave == 0 && lane < g.Bw && kvalid) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const double v = i < kSums ? ((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane]
                                       : fmax(fmax(fmax(red[0][i][lane], red[1][i][lane]), red[2][i][lane]), red[3][i][lane]);
            partials[(static_cast<size_t>(rb) * NACC + i) * g.Bp + k] = v;
        }
    }
}

// ---- fused SpMM + half-step ---------------------------------------------------------------------
// XHALF: M = A^T (n rows), V = Y.  reference update_x_z_{check,normal}_batched_kernel :122-178
// else : M = A   (m rows), V = X_hat.  reference update_y_{check,normal}_batched_kernel :180-236
// cache policy of the panel streams (measured on config 4, profiles/r02_pmc_summary.md)
#ifndef HPRLP_BATCH_NT
#define HPRLP_BATCH_NT 1  // 1: nontemporal loads of the panel streams (6390 -> 6800 batch-it/s on config 4); 2: also store X nontemporal (no difference)
#endif
constexpr bool kNtPanels = HPRLP_BATCH_NT != 0;
constexpr bool kNtStoreX = HPRLP_BATCH_NT >= 2;

struct HalfArgs {
    const double *V;                   // gathered panel
    int vrows;                         // its rows (= columns of the matrix)
    double *P, *P_hat;                 // X / X_hat  or  Y / (unused)
    const double *lo, *hi, *cost;      // L,U,C  or  AL,AU,(unused)
    const double *last;
    double *bar, *aux, *delta;         // X_bar, Z_bar, DX  or  Y_bar, Y_obj, DY  (check only)
    BatchCtl ctl;
    double lambda_max;
    double *partials;
    const int *order;                  // kb_half64: row group handled at position g of the launch (null: g itself)
};

// the half-step update of one (row, problem) element given the SpMM row sum s
template <bool XHALF, bool CHECK, int NACC>
__device__ __forceinline__ void half_update(const HalfArgs &a, size_t t, double s, double p_i, double p_lo, double p_hi,
                                            double p_last, double p_cost, double sig, double fact1, double f1,
                                            double f2, double (&acc)[NACC]) {
    if (XHALF) {
        const double xi = p_i;
        const double zt = xi + sig * (s - p_cost);
        const double xb = fmin(fmax(zt, p_lo), p_hi);
        const double xh = 2.0 * xb - xi;
        a.P_hat[t] = xh;  // gathered by the y-half that follows: default policy
        if (kNtStoreX) __builtin_nontemporal_store(f2 * xh + f1 * p_last, a.P + t);  // next read: the next iteration's x-half
        else a.P[t] = f2 * xh + f1 * p_last;
        if (CHECK) {
            const double zb = (xb - zt) / sig, dx = xb - xh;
            a.delta[t] = dx;
            a.aux[t] = zb;
            a.bar[t] = xb;
            acc[0] += p_cost * xb;
            acc[1 % NACC] += xb * zb;
            acc[2 % NACC] += dx * dx;
        }
    } else {
        const double yi = p_i;
        const double v = s - fact1 * yi;
        const double d = fmax(p_lo - v, fmin(p_hi - v, 0.0));
        const double yb = d / fact1;
        const double yh = 2.0 * yb - yi;
        a.P[t] = f2 * yh + f1 * p_last;
        if (CHECK) {
            const double dy = yb - yh, yo = v + d;
            a.delta[t] = dy;
            a.bar[t] = yb;
            a.aux[t] = yo;
            acc[0] += yo * yb;
            acc[1 % NACC] += dy * dy;
        }
    }
}

template <bool XHALF, bool CHECK>
__global__ void __launch_bounds__(256) kb_half(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                               const double *__restrict__ val, Geo g, HalfArgs a) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    constexpr int NACC = CHECK ? (XHALF ? 3 : 2) : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

    const bool act = a.ctl.active[k] != 0;
    const int kk = XHALF ? a.ctl.kx[k] : a.ctl.ky[k];
    const double sig = a.ctl.sigma[k];
    const double f1 = 1.0 / (static_cast<double>(kk) + 2.0), f2 = 1.0 - f1;
    const double fact1 = a.lambda_max * sig;
    // counter hand-off (see Ctrl in kernels.h): the x-half publishes ky, the y-half advances kx
    if (blk.rb == 0 && wave == 0 && sub == 0) {
        if (XHALF) a.ctl.ky[k] = kk;
        else if (act) a.ctl.kx[k] = kk + 1;
    }
    const double *__restrict__ V = a.V + pidx(g, blk.chunk, a.vrows, 0, kl);
    for (int r = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub; r < rows; r += blk.nrb * g.rows_per_block) {
        if (!act) continue;
        // the panel operands do not depend on the row sum: issue their loads first so that they
        // overlap the gather chain of the SpMM loop
        const size_t t = pidx(g, blk.chunk, rows, r, kl);
        const double p_i = a.P[t], p_lo = a.lo[t], p_hi = a.hi[t], p_last = a.last[t];
        const double p_cost = XHALF ? a.cost[t] : 0.0;
        double s = 0.0;
        const int e = rowptr[r + 1];
        for (int p = rowptr[r]; p < e; p += 4) {  // four gathers in flight, summed in CSR order
            double av[4], gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(p + u, e - 1);
                av[u] = val[q];
                gv[u] = V[static_cast<size_t>(col[q]) * g.Bw];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (p + u < e) s += av[u] * gv[u];
        }
        half_update<XHALF, CHECK, NACC>(a, t, s, p_i, p_lo, p_hi, p_last, p_cost, sig, fact1, f1, f2, acc);
    }
    if (CHECK) block_store_per_problem<NACC>(acc, g, blk.rb, k, true, a.partials);
}

// Chunks of 64 problems (a wave = 64 problems of ONE row): the row index is wave-uniform, so row pointers, column
// indices and values come through the scalar cache, and a wave works on kRowsPerWave consecutive rows
// at once -- their nonzeros are one contiguous CSR range -- with all panel loads and up to 8 gathers
// in flight before the first use.  Each row is still summed in CSR order.
constexpr int kRowsPerWave = 4;

template <bool XHALF, bool CHECK>
__global__ void __launch_bounds__(256) kb_half64(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                 const double *__restrict__ val, Geo g, HalfArgs a) {
    constexpr int RW = kRowsPerWave, G = 8;
    static_assert(RW == 4, "the row select below is written for 4 rows");
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blk.chunk * 64 + lane;
    constexpr int NACC = CHECK ? (XHALF ? 3 : 2) : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

    const bool act = a.ctl.active[k] != 0;
    const int kk = XHALF ? a.ctl.kx[k] : a.ctl.ky[k];
    const double sig = a.ctl.sigma[k];
    const double f1 = 1.0 / (static_cast<double>(kk) + 2.0), f2 = 1.0 - f1;
    const double fact1 = a.lambda_max * sig;
    if (blk.rb == 0 && wave == 0) {
        if (XHALF) a.ctl.ky[k] = kk;
        else if (act) a.ctl.kx[k] = kk + 1;
    }
    const double *__restrict__ V = a.V + pidx(g, blk.chunk, a.vrows, 0, lane);
    // Row groups in launch order: the few groups with long rows first (BatchWS::order_*).  A 200-entry row is 26 dependent
    // trips to memory for its wave (about 50 us): dispatched wherever it falls in the row order it ends up as the launch's
    // tail (config 4: 53 such rows of A^T, x-half 101 -> 71 us without them); dispatched first it runs beside everything else.
    const int ngroups = (rows + RW - 1) / RW;
    for (int gi = __builtin_amdgcn_readfirstlane(blk.rb * 4 + wave); gi < ngroups; gi += blk.nrb * 4) {
        const int rb = (a.order ? a.order[gi] : gi) * RW;
        int pb[RW + 1];
#pragma unroll
        for (int i = 0; i <= RW; ++i) pb[i] = rowptr[min(rb + i, rows)];
        double p_i[RW], p_lo[RW], p_hi[RW], p_last[RW], p_cost[RW], s[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const size_t t = pidx(g, blk.chunk, rows, min(rb + i, rows - 1), lane);
            if (kNtPanels) {  // the panel streams are read once per half-step: keep them out of the gathered panel's way in the caches
                p_i[i] = __builtin_nontemporal_load(a.P + t), p_lo[i] = __builtin_nontemporal_load(a.lo + t);
                p_hi[i] = __builtin_nontemporal_load(a.hi + t), p_last[i] = __builtin_nontemporal_load(a.last + t);
                p_cost[i] = XHALF ? __builtin_nontemporal_load(a.cost + t) : 0.0;
            } else {
                p_i[i] = a.P[t], p_lo[i] = a.lo[t], p_hi[i] = a.hi[t], p_last[i] = a.last[t];
                p_cost[i] = XHALF ? a.cost[t] : 0.0;
            }
            s[i] = 0.0;
        }
        const int pend = pb[RW];
        for (int p = pb[0]; p < pend; p += G) {
            double gv[G], av[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int q = min(p + u, pend - 1);
                av[u] = val[q];
                gv[u] = V[static_cast<size_t>(col[q]) * 64];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int q = p + u;
                if (q < pend) {
                    const double prod = av[u] * gv[u];
                    if (q < pb[1]) s[0] += prod;
                    else if (q < pb[2]) s[1] += prod;
                    else if (q < pb[3]) s[2] += prod;
                    else s[3] += prod;
                }
            }
        }
        if (act) {
#pragma unroll
            for (int i = 0; i < RW; ++i)
                if (rb + i < rows)
                    half_update<XHALF, CHECK, NACC>(a, pidx(g, blk.chunk, rows, rb + i, lane), s[i], p_i[i], p_lo[i], p_hi[i],
                                                    p_last[i], p_cost[i], sig, fact1, f1, f2, acc);
        }
    }
    if (CHECK) block_store_per_problem<NACC>(acc, g, blk.rb, k, true, a.partials);
}

// Chunks of BW = 8 / 16 / 32 problems: a wave is SUBS = 64 / BW lane groups; lane group `sub` of a wave that works on the
// 4 * SUBS consecutive rows from r0 takes rows r0 + i * SUBS + sub, i = 0..3, so that every panel load of the wave (fixed i)
// reads SUBS consecutive rows = one contiguous 512-byte run.  Same structure as kb_half64 otherwise -- all panel loads and up
// to 8 gathers in flight per lane before the first use, every row summed in CSR order -- but the CSR arrays come through
// vector loads (the rows are uniform per lane group, not per wave) and a lane group's entries are four separate CSR ranges,
// walked as one concatenated range.
template <bool XHALF, bool CHECK, int BW>
__global__ void __launch_bounds__(256) kb_halfN(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                const double *__restrict__ val, Geo g, HalfArgs a) {
    constexpr int RW = kRowsPerWave, G = 8, SUBS = 64 / BW;
    static_assert(RW == 4, "the row select below is written for 4 rows");
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % BW, sub = lane / BW, k = blk.chunk * BW + kl;
    constexpr int NACC = CHECK ? (XHALF ? 3 : 2) : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

    const bool act = a.ctl.active[k] != 0;
    const int kk = XHALF ? a.ctl.kx[k] : a.ctl.ky[k];
    const double sig = a.ctl.sigma[k];
    const double f1 = 1.0 / (static_cast<double>(kk) + 2.0), f2 = 1.0 - f1;
    const double fact1 = a.lambda_max * sig;
    if (blk.rb == 0 && wave == 0 && sub == 0) {
        if (XHALF) a.ctl.ky[k] = kk;
        else if (act) a.ctl.kx[k] = kk + 1;
    }
    const double *__restrict__ V = a.V + pidx(g, blk.chunk, a.vrows, 0, kl);
    const int ngroups = (rows + RW * SUBS - 1) / (RW * SUBS);
    for (int gi = blk.rb * 4 + wave; gi < ngroups; gi += blk.nrb * 4) {
        const int r0 = (a.order ? a.order[gi] : gi) * (RW * SUBS) + sub;
        int pb[RW], pe[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const int r = min(r0 + i * SUBS, rows);
            pb[i] = rowptr[r];
            pe[i] = rowptr[min(r + 1, rows)];
        }
        double p_i[RW], p_lo[RW], p_hi[RW], p_last[RW], p_cost[RW], s[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const size_t t = pidx(g, blk.chunk, rows, min(r0 + i * SUBS, rows - 1), kl);
            if (kNtPanels) {
                p_i[i] = __builtin_nontemporal_load(a.P + t), p_lo[i] = __builtin_nontemporal_load(a.lo + t);
                p_hi[i] = __builtin_nontemporal_load(a.hi + t), p_last[i] = __builtin_nontemporal_load(a.last + t);
                p_cost[i] = XHALF ? __builtin_nontemporal_load(a.cost + t) : 0.0;
            } else {
                p_i[i] = a.P[t], p_lo[i] = a.lo[t], p_hi[i] = a.hi[t], p_last[i] = a.last[t];
                p_cost[i] = XHALF ? a.cost[t] : 0.0;
            }
            s[i] = 0.0;
        }
        // position e of the concatenated range -> CSR position e + (offset of the row e falls in)
        const int c1 = pe[0] - pb[0], c2 = c1 + (pe[1] - pb[1]), c3 = c2 + (pe[2] - pb[2]), total = c3 + (pe[3] - pb[3]);
        const int d0 = pb[0], d1 = pb[1] - c1, d2 = pb[2] - c2, d3 = pb[3] - c3;
        for (int p = 0; p < total; p += G) {
            double gv[G], av[G];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int e = min(p + u, total - 1);
                const int q = e + (e < c1 ? d0 : e < c2 ? d1 : e < c3 ? d2 : d3);
                av[u] = val[q];
                gv[u] = V[static_cast<size_t>(col[q]) * BW];
            }
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int e = p + u;
                if (e < total) {
                    const double prod = av[u] * gv[u];
                    if (e < c1) s[0] += prod;
                    else if (e < c2) s[1] += prod;
                    else if (e < c3) s[2] += prod;
                    else s[3] += prod;
                }
            }
        }
        if (act) {
#pragma unroll
            for (int i = 0; i < RW; ++i)
                if (r0 + i * SUBS < rows)
                    half_update<XHALF, CHECK, NACC>(a, pidx(g, blk.chunk, rows, r0 + i * SUBS, kl), s[i], p_i[i], p_lo[i], p_hi[i],
                                                    p_last[i], p_cost[i], sig, fact1, f1, f2, acc);
        }
    }
    if (CHECK) block_store_per_problem<NACC>(acc, g, blk.rb, k, true, a.partials);
}

// ---- residual SpMMs (reference compute_batched_Rd/Rp_kernel :238-263 + SpMM) ---------------------
// WHICH 0: |(C - A^T Ybar - Zbar) .* col_norm|^2 ; 1: |Rp|^2 ; 2: |Rp|^2 and <A DX, DY> ; 3: <A DX, DY>
template <int WHICH>
__global__ void __launch_bounds__(256) kb_resid(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                const double *__restrict__ val, Geo g, int vrows, const double *V,
                                                const double *V2, const double *p0, const double *p1,
                                                const double *norm, const double *dvec, double *partials) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    const size_t vbase = pidx(g, blk.chunk, vrows, 0, kl);
    constexpr int NACC = (WHICH == 2) ? 2 : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    for (int r = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub; r < rows; r += blk.nrb * g.rows_per_block) {
        double s = 0.0, s2 = 0.0;
        const int e = rowptr[r + 1];
        for (int p = rowptr[r]; p < e; p += 4) {  // four entries in flight (a dependent trip per entry made long rows a 300 us tail); summed in CSR order
            double av[4], g1[4], g2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(p + u, e - 1);
                const size_t gi = vbase + static_cast<size_t>(col[q]) * g.Bw;
                av[u] = val[q];
                g1[u] = WHICH != 3 ? V[gi] : 0.0;
                g2[u] = WHICH >= 2 ? V2[gi] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (p + u < e) {
                    if (WHICH != 3) s += av[u] * g1[u];
                    if (WHICH >= 2) s2 += av[u] * g2[u];
                }
        }
        const size_t t = pidx(g, blk.chunk, rows, r, kl);
        if (WHICH == 0) {
            const double rd = (p0[t] - s - p1[t]) * norm[r];
            acc[0] += rd * rd;
        } else if (WHICH == 1 || WHICH == 2) {
            const double rp = norm[r] * fmax(fmin(p1[t] - s, 0.0), p0[t] - s);
            acc[0] += rp * rp;
            if (WHICH == 2) acc[1 % NACC] += s2 * dvec[t];
        } else {
            acc[0] += s2 * dvec[t];
        }
    }
    block_store_per_problem<NACC>(acc, g, blk.rb, k, true, partials);
}

// iteration-0 bound violation (reference compute_batched_lu_violation_kernel :265-278)
__global__ void __launch_bounds__(256) kb_lu(int n, Geo g, const double *Xb, const double *L, const double *U,
                                             const double *col_norm, double *DX, double *partials) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    double acc[1] = {0.0};
    for (int r = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub; r < n; r += blk.nrb * g.rows_per_block) {
        const size_t t = pidx(g, blk.chunk, n, r, kl);
        const double x = Xb[t];
        const double viol = x < L[t] ? L[t] - x : (x > U[t] ? x - U[t] : 0.0);
        const double v = viol / col_norm[r];
        DX[t] = v;
        acc[0] += v * v;
    }
    block_store_per_problem<1>(acc, g, blk.rb, k, true, partials);
}

// DX = Xbar - lastX, DY = Ybar - lastY for ALL problems, with their squared norms
// (reference batched_restart_movement_kernel :280-294 + the per-problem nrm2 calls :662-663)
__global__ void __launch_bounds__(256) kb_movement(int n, int m, Geo g, const double *Xb, const double *lastX,
                                                   double *DX, const double *Yb, const double *lastY, double *DY,
                                                   double *partials) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    double acc[2] = {0.0, 0.0};
    const int r0 = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub, rs = blk.nrb * g.rows_per_block;
    for (int r = r0; r < n; r += rs) {
        const size_t t = pidx(g, blk.chunk, n, r, kl);
        const double d = Xb[t] - lastX[t];
        DX[t] = d;
        acc[0] += d * d;
    }
    for (int r = r0; r < m; r += rs) {
        const size_t t = pidx(g, blk.chunk, m, r, kl);
        const double d = Yb[t] - lastY[t];
        DY[t] = d;
        acc[1] += d * d;
    }
    block_store_per_problem<2>(acc, g, blk.rb, k, true, partials);
}

// where restart_flag[k]: X = lastX = Xbar, Y = lastY = Ybar, inner counter reset
// (reference do_batched_restart_kernel :296-323)
__global__ void __launch_bounds__(256) kb_restart(int n, int m, Geo g, double *X, double *lastX, const double *Xb,
                                                  double *Y, double *lastY, const double *Yb, BatchCtl ctl) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    if (!ctl.restart_flag[k]) return;
    const int r0 = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub, rs = blk.nrb * g.rows_per_block;
    for (int r = r0; r < n; r += rs) {
        const size_t t = pidx(g, blk.chunk, n, r, kl);
        const double v = Xb[t];
        X[t] = v;
        lastX[t] = v;
    }
    for (int r = r0; r < m; r += rs) {
        const size_t t = pidx(g, blk.chunk, m, r, kl);
        const double v = Yb[t];
        Y[t] = v;
        lastY[t] = v;
    }
    if (blk.rb == 0 && wave == 0 && sub == 0 && ctl.active[k]) {
        ctl.kx[k] = 0;
        ctl.ky[k] = 0;
    }
}

// ---- infeasibility detection (hprlp_solve_batched_detect; DESIGN.md "Batched detection") ------------------------------
// The Farkas ratio tests of Solver::ray_test, member by member in that member's units.  Scaled -> caller's units by the map of
// the results: x = X / col_norm * b_scale[k], y = Y / row_norm * c_scale[k], z = Z * col_norm * c_scale[k]; the bound panels
// hold AL / (row_norm b_scale[k]), l col_norm / b_scale[k] (positive factors: every bound stays on its side).
//
// A bound counts as finite iff its panel value is not +-kInfReplacement: the set-up writes that value where the caller passed
// +-inf.  A caller's own bound that is +-1e100 after scaling cannot be told apart and counts as infinite too, which is how the
// iteration already treats it (its projections see the same 1e100 either way).
__device__ __forceinline__ bool finite_bound(double v) { return v != kInfReplacement && v != -kInfReplacement; }

// kb_ray_form's accumulators are k_ray_form's (kernels.h kRayFormAccs): D of the rows, c'd (sums); V of the rows, W of the
// columns, |y|_inf, |d|_inf (maxima)
struct RayArgs {
    const double *Xb, *Yb;
    double *prevX, *prevY, *DS, *YS;  // previous evaluation's X_bar / Y_bar, and the rays (scaled units, gathered by kb_ray_col / kb_ray_row)
    const double *L, *U, *C, *AL, *AU;
    const double *col_norm, *row_norm;
    const double *b_scale, *c_scale;  // per member (Bp)
    const int *active;
};

// Active members only: DS = Xb - prevX, prevX <- Xb, YS = Yb - prevY, prevY <- Yb, and the elementwise terms of the tests in the
// caller's units -> partials (kRayFormAccs per row block).  A frozen member's columns are left as they are: a verdict's
// certificate is read from its DS / YS after the loop.
__global__ void __launch_bounds__(256) kb_ray_form(int n, int m, Geo g, RayArgs a, double *partials) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    double acc[kRayFormAccs] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.active[k]) {
        const double bs = a.b_scale[k], cs = a.c_scale[k];
        const int r0 = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub, rs = blk.nrb * g.rows_per_block;
        for (int r = r0; r < n; r += rs) {
            const size_t t = pidx(g, blk.chunk, n, r, kl);
            const double xb = a.Xb[t], ds = xb - a.prevX[t];
            a.prevX[t] = xb;
            a.DS[t] = ds;
            const double cn = a.col_norm[r];
            const double d = (ds / cn) * bs;
            acc[1] += ((a.C[t] * cn) * cs) * d;
            if (finite_bound(a.L[t])) acc[3] = fmax(acc[3], -d);
            if (finite_bound(a.U[t])) acc[3] = fmax(acc[3], d);
            acc[5] = fmax(acc[5], fabs(d));
        }
        for (int r = r0; r < m; r += rs) {
            const size_t t = pidx(g, blk.chunk, m, r, kl);
            const double yb = a.Yb[t], ys = yb - a.prevY[t];
            a.prevY[t] = yb;
            a.YS[t] = ys;
            const double rn = a.row_norm[r];
            const double y = (ys / rn) * cs;
            if (y > 0.0) {  // pairs with AL
                const double lo = a.AL[t];
                if (finite_bound(lo)) acc[0] += ((lo * rn) * bs) * y;
                else acc[2] = fmax(acc[2], y);
            } else if (y < 0.0) {  // pairs with AU
                const double hi = a.AU[t];
                if (finite_bound(hi)) acc[0] += ((hi * rn) * bs) * y;
                else acc[2] = fmax(acc[2], -y);
            }
            acc[4] = fmax(acc[4], fabs(y));
        }
    }
    block_store_per_problem<kRayFormAccs, 4>(acc, g, blk.rb, k, true, partials);
}

// The SpMMs of the ray test, with kb_resid's panel geometry (a lane follows one member, rows summed in CSR order, four entries
// in flight).  RAY_COL: rows of A^T gathering YS, z = -A^T y; D of the columns (z_j > 0 pairs with l_j, z_j < 0 with u_j; sum)
// and V of the columns (max) -> out = partials (2 per row block).  RAY_ROW: rows of A gathering DS, q = A d; W of the rows (max)
// -> partials.  RAY_PRODUCT: the plain product into the panel `out` for every member (the certificates' z, after the loop).
// The kernels: kb_ray_col, kb_ray_row, kb_ray_product below.
enum RaySpmm : int { RAY_COL = 0, RAY_ROW, RAY_PRODUCT };
template <int MODE>
__device__ __forceinline__ void ray_spmm(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                         const double *__restrict__ val, const Geo &g, int vrows, const double *V, const double *lo,
                                         const double *hi, const double *norm, const RayArgs &a, double *out) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    const size_t vbase = pidx(g, blk.chunk, vrows, 0, kl);
    constexpr int NACC = MODE == RAY_COL ? 2 : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    if (MODE == RAY_PRODUCT || a.active[k]) {
        const double bs = a.b_scale[k], cs = a.c_scale[k];
        for (int r = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub; r < rows; r += blk.nrb * g.rows_per_block) {
            double s = 0.0;
            const int e = rowptr[r + 1];
            for (int p = rowptr[r]; p < e; p += 4) {
                double av[4], gv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = min(p + u, e - 1);
                    av[u] = val[q];
                    gv[u] = V[vbase + static_cast<size_t>(col[q]) * g.Bw];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (p + u < e) s += av[u] * gv[u];
            }
            const size_t t = pidx(g, blk.chunk, rows, r, kl);
            if (MODE == RAY_PRODUCT) {
                out[t] = s;
            } else if (MODE == RAY_COL) {
                const double cn = norm[r], z = -((s * cn) * cs);
                if (z > 0.0) {
                    const double l = lo[t];
                    if (finite_bound(l)) acc[0] += ((l / cn) * bs) * z;
                    else acc[NACC - 1] = fmax(acc[NACC - 1], z);
                } else if (z < 0.0) {
                    const double u = hi[t];
                    if (finite_bound(u)) acc[0] += ((u / cn) * bs) * z;
                    else acc[NACC - 1] = fmax(acc[NACC - 1], -z);
                }
            } else {
                const double q = (s * norm[r]) * bs;
                if (finite_bound(lo[t])) acc[0] = fmax(acc[0], -q);
                if (finite_bound(hi[t])) acc[0] = fmax(acc[0], q);
            }
        }
    }
    if constexpr (MODE != RAY_PRODUCT) block_store_per_problem<NACC, 1>(acc, g, blk.rb, k, true, out);
}

#define HPRLP_RAY_SPMM_KERNEL(NAME, MODE)                                                                                        \
    __global__ void __launch_bounds__(256) NAME(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,        \
                                                const double *__restrict__ val, Geo g, int vrows, const double *V,            \
                                                const double *lo, const double *hi, const double *norm, RayArgs a, double *out) { \
        ray_spmm<MODE>(rows, rowptr, col, val, g, vrows, V, lo, hi, norm, a, out);                                              \
    }
HPRLP_RAY_SPMM_KERNEL(kb_ray_col, RAY_COL)
HPRLP_RAY_SPMM_KERNEL(kb_ray_row, RAY_ROW)
HPRLP_RAY_SPMM_KERNEL(kb_ray_product, RAY_PRODUCT)
#undef HPRLP_RAY_SPMM_KERNEL

// ---- warm start (hprlp_solve_batched_warm; DESIGN.md "Warm start") ------------------------------------------------------
// X and Y hold the members' starts, scaled on the host: project them (X into [L, U]; Y onto the sign cone of the row's sides --
// y > 0 means the row sits at AL) and seed every panel the first iteration reads: X, X_hat, X_bar, lastX (the Halpern anchor);
// Y, Y_bar, lastY.  mask null: every member, the padding included (its panels are zero and stay zero); else the members with
// mask[k] != 0 (a streamed batch's refill seeds the members that have just entered, and no other).
__global__ void __launch_bounds__(256) kb_start_seed(int n, int m, Geo g, double *X, double *Xh, double *Xb, double *lastX,
                                                     const double *L, const double *U, double *Y, double *Yb, double *lastY,
                                                     const double *AL, const double *AU, const int *mask) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw;
    const int sub = lane / g.Bw;
    if (mask && !mask[blk.chunk * g.Bw + kl]) return;
    const int r0 = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub, rs = blk.nrb * g.rows_per_block;
    for (int r = r0; r < n; r += rs) {
        const size_t t = pidx(g, blk.chunk, n, r, kl);
        const double v = fmin(fmax(X[t], L[t]), U[t]);
        X[t] = v;
        Xh[t] = v;
        Xb[t] = v;
        lastX[t] = v;
    }
    for (int r = r0; r < m; r += rs) {
        const size_t t = pidx(g, blk.chunk, m, r, kl);
        double v = Y[t];
        if (!finite_bound(AL[t])) v = fmin(v, 0.0);
        if (!finite_bound(AU[t])) v = fmax(v, 0.0);
        Y[t] = v;
        Yb[t] = v;
        lastY[t] = v;
    }
}

// The iteration-0 evaluation of the starts, with kb_resid's geometry.  START_COL: rows of A^T gathering Y_bar; w = C - A^T y and
// Z_bar = w where its sign has a finite bound to lean on (w > 0: L, w < 0: U), else 0 (the dual completion); partials of C.X_bar
// (B_CX) and of the bound terms L z (z > 0), U z (z < 0) (B_XZ: what X_bar.Z_bar is at a check, Solver::set_start).  START_ROW: rows of A gathering X_bar; Y_obj = AL where y > 0, AU where y < 0, the activity
// clamped into [AL, AU] where y = 0; partials of Y_obj.Y_bar (B_YOBJ_Y).  mask as kb_start_seed's: a member left out keeps its
// `out` column and contributes 0.0 partials.
template <bool COL>
__global__ void __launch_bounds__(256) kb_start_spmm(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                     const double *__restrict__ val, Geo g, int vrows, const double *V,
                                                     const double *p0, const double *lo, const double *hi, const double *bar,
                                                     double *out, double *partials, const int *mask) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    const size_t vbase = pidx(g, blk.chunk, vrows, 0, kl);
    constexpr int NACC = COL ? 2 : 1;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    const bool live = !mask || mask[k] != 0;
    for (int r = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub; live && r < rows; r += blk.nrb * g.rows_per_block) {
        double s = 0.0;
        const int e = rowptr[r + 1];
        for (int p = rowptr[r]; p < e; p += 4) {  // four entries in flight, summed in CSR order (kb_resid)
            double av[4], gv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(p + u, e - 1);
                av[u] = val[q];
                gv[u] = V[vbase + static_cast<size_t>(col[q]) * g.Bw];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (p + u < e) s += av[u] * gv[u];
        }
        const size_t t = pidx(g, blk.chunk, rows, r, kl);
        const double b = bar[t];
        if constexpr (COL) {
            const double c = p0[t], d = c - s;
            const double z = ((d > 0.0 && finite_bound(lo[t])) || (d < 0.0 && finite_bound(hi[t]))) ? d : 0.0;
            out[t] = z;
            acc[0] += c * b;
            acc[NACC - 1] += (z > 0.0 ? lo[t] : (z < 0.0 ? hi[t] : 0.0)) * z;
        } else {
            const double yo = b > 0.0 ? lo[t] : (b < 0.0 ? hi[t] : fmin(fmax(s, lo[t]), hi[t]));
            out[t] = yo;
            acc[0] += yo * b;
        }
    }
    block_store_per_problem<NACC>(acc, g, blk.rb, k, true, partials);
}

// SC[slot[i]*Bp + k] = sum over blocks of partials[(b*nacc + i)*Bp + k]; the maximum instead where bit i of max_mask is set
// (partials of nonnegative maxima: kb_ray_form, kb_ray_col / kb_ray_row)
struct BFin {
    int slot[6];
    int nacc;
    unsigned max_mask;
};
// grid (ceil(Bp/64), nacc): a block sums one accumulator for 64 problems; its 4 waves stride over the
// producer blocks (lane = problem: coalesced), then combine in a fixed order
__global__ void __launch_bounds__(1024) kb_finalize(const double *partials, int nblocks, int Bp, BFin f, double *SC) {
    // 16 waves, four independent load chains per wave; fixed combination order => deterministic
    __shared__ double red[16][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 64 + lane, i = blockIdx.y;
    const bool mx = (f.max_mask >> i) & 1u;  // (uniform per block)
    auto comb = [mx](double a, double b) { return mx ? fmax(a, b) : a + b; };
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (k < Bp) {
        const double *__restrict__ p = partials + static_cast<size_t>(i) * Bp + k;
        const size_t st = static_cast<size_t>(f.nacc) * Bp;
        int b = wave;
        for (; b + 48 < nblocks; b += 64) {
            v0 = comb(v0, p[b * st]);
            v1 = comb(v1, p[(b + 16) * st]);
            v2 = comb(v2, p[(b + 32) * st]);
            v3 = comb(v3, p[(b + 48) * st]);
        }
        for (; b < nblocks; b += 16) v0 = comb(v0, p[b * st]);
    }
    red[wave][lane] = comb(comb(v0, v1), comb(v2, v3));
    __syncthreads();
    if (wave == 0 && k < Bp) {
        double v = red[0][lane];
#pragma unroll
        for (int w = 1; w < 16; ++w) v = comb(v, red[w][lane]);
        SC[static_cast<size_t>(f.slot[i]) * Bp + k] = v;
    }
}

// ---- a batch's way in and out (DESIGN.md "Resident batches") --------------------------------------------------------------
// Column-major staging (rows x B: member k's vector at k * rows, as the ABI has it) <-> padded panels.  The staging side runs
// along the rows and the panel side along the members, so a 256-thread workgroup moves a tile of kPanelTile rows x kPanelTile
// members through LDS (one column of padding: the transposed access walks the banks) and both sides move whole lines: 256
// contiguous bytes per row of the tile on the staging side; on the panel side min(Bw, 32) members of a row are contiguous,
// and with Bw < 32 the rows of a chunk follow each other, so the tile's part of a chunk is one run.  Elementwise: the bits
// are the host path's (to_panel / from_panel, point_to_caller, reduced_cost_to_caller, start_to_scaled).
constexpr int kPanelTile = 32;
constexpr int kPanelVectors = 7;  // C, L, U, AL, AU and the starts X0, Y0

// (row, member) of the tile that thread `e` (of 1024 / 4 per thread) touches on the panel side: consecutive e = consecutive addresses
struct TileElem {
    int il, kl;  // row and member inside the tile
};
__device__ __forceinline__ TileElem panel_side(int e, int W) {
    const int sub = e / (kPanelTile * W), r = e % (kPanelTile * W);  // the tile's members lie in 32 / W chunks
    return TileElem{r / W, sub * W + r % W};
}

struct PanelIn {
    const double *src[kPanelVectors];  // column-major rows x B
    double *dst[kPanelVectors];        // padded panels
    int rows[kPanelVectors];
};
// grid (row tiles of the longest vector, member tiles of Bp, vectors): padding members and dead columns become 0.0
__global__ void __launch_bounds__(256) kb_panel_in(PanelIn a, int B, Geo g) {
    __shared__ double tile[kPanelTile][kPanelTile + 1];  // [member][row]
    const int v = blockIdx.z, rows = a.rows[v];
    const int i0 = blockIdx.x * kPanelTile, k0 = blockIdx.y * kPanelTile;
    if (i0 >= rows) return;  // (uniform per workgroup)
    const double *__restrict__ src = a.src[v];
    double *__restrict__ dst = a.dst[v];
    const int tx = threadIdx.x % kPanelTile, ty = threadIdx.x / kPanelTile;
#pragma unroll
    for (int j = 0; j < kPanelTile; j += 8) {
        const int k = k0 + ty + j, i = i0 + tx;
        tile[ty + j][tx] = (k < B && i < rows) ? src[static_cast<size_t>(k) * rows + i] : 0.0;
    }
    __syncthreads();
    const int W = min(g.Bw, kPanelTile);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const TileElem t = panel_side(threadIdx.x + 256 * j, W);
        const int k = k0 + t.kl, i = i0 + t.il;
        if (k < g.Bp && i < rows) dst[pidx(g, k / g.Bw, rows, i, k % g.Bw)] = tile[t.kl][t.il];
    }
}

struct PanelOut {
    const double *src[3];    // Xb, Yb, Zb
    double *dst[3];          // column-major rows x B
    const double *norm[3];   // cn, rn, cn
    const double *scale[3];  // b_scale, c_scale, c_scale (per member)
    int rows[3];
};
// The first B members of X_bar / Y_bar / Z_bar in the caller's units, column-major: x and y by point_to_caller, z by
// reduced_cost_to_caller (batch_units.h).
__global__ void __launch_bounds__(256) kb_panel_out(PanelOut a, int B, Geo g) {
    __shared__ double tile[kPanelTile][kPanelTile + 1];  // [member][row]
    const int v = blockIdx.z, rows = a.rows[v];
    const int i0 = blockIdx.x * kPanelTile, k0 = blockIdx.y * kPanelTile;
    if (i0 >= rows) return;
    const double *__restrict__ src = a.src[v];
    const double *__restrict__ norm = a.norm[v];
    const double *__restrict__ scale = a.scale[v];
    double *__restrict__ dst = a.dst[v];
    const int W = min(g.Bw, kPanelTile);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const TileElem t = panel_side(threadIdx.x + 256 * j, W);
        const int k = k0 + t.kl, i = i0 + t.il;
        double r = 0.0;
        if (k < B && i < rows) {
            const double p = src[pidx(g, k / g.Bw, rows, i, k % g.Bw)];
            r = v == 2 ? reduced_cost_to_caller(p, norm[i], scale[k]) : point_to_caller(p, norm[i], scale[k]);
        }
        tile[t.kl][t.il] = r;
    }
    __syncthreads();
    const int tx = threadIdx.x % kPanelTile, ty = threadIdx.x / kPanelTile;
#pragma unroll
    for (int j = 0; j < kPanelTile; j += 8) {
        const int k = k0 + ty + j, i = i0 + tx;
        if (k < B && i < rows) dst[static_cast<size_t>(k) * rows + i] = tile[ty + j][tx];
    }
}

// carry: every member starts from the previous batch's solution of the same member.  Per element the composition of
// point_to_caller with the previous batch's scales and start_to_scaled with this batch's (batch_units.h), each rounding kept: X with
// cn and the b scales, Y with rn and the c scales.  Reads X_bar / Y_bar in place (before they are zeroed), writes X / Y; padding
// members get 0.0.
__global__ void __launch_bounds__(256) kb_carry_start(int n, int m, int B, Geo g, const double *Xb, const double *Yb, double *X, double *Y,
                                                      const double *col_norm, const double *row_norm, const double *b_old,
                                                      const double *b_new, const double *c_old, const double *c_new) {
    const Blk blk = decode_block(g);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kl = lane % g.Bw, k = blk.chunk * g.Bw + kl;
    const int sub = lane / g.Bw;
    const bool live = k < B;
    const double bo = b_old[k], bn = b_new[k], co = c_old[k], cw = c_new[k];
    const int r0 = blk.rb * g.rows_per_block + wave * g.rows_per_wave + sub, rs = blk.nrb * g.rows_per_block;
    for (int r = r0; r < n; r += rs) {
        const size_t t = pidx(g, blk.chunk, n, r, kl);
        const double cn = col_norm[r];
        const double x = point_to_caller(Xb[t], cn, bo);
        X[t] = live ? start_to_scaled(x, cn, bn) : 0.0;
    }
    for (int r = r0; r < m; r += rs) {
        const size_t t = pidx(g, blk.chunk, m, r, kl);
        const double rn = row_norm[r];
        const double y = point_to_caller(Yb[t], rn, co);
        Y[t] = live ? start_to_scaled(y, rn, cw) : 0.0;
    }
}

// ---- one member into and out of a running workspace (DESIGN.md "Streamed batches") -------------------------------------------------
// A refill pass of a streamed batch is driven by one table of {slot, problem} pairs, ordered by slot.  One thread per element,
// element e = (row e / np, pair e % np): consecutive lanes take consecutive listed slots of ONE row before the next row.  On the
// panel side a row of a chunk is Bw consecutive doubles, so the slots of one chunk that refill together share its lines; the
// queue / result side is column-major per problem (problem p's vector at p * rows) and is strided by the vector's length.
// No thread writes an element another thread touches: no atomics.
struct SlotPair {
    int slot, problem;
};
__device__ __forceinline__ size_t slot_elem(const Geo &g, int rows, int i, int slot) {
    return pidx(g, slot / g.Bw, rows, i, slot % g.Bw);
}

constexpr int kSlotPanels = 8;  // most panels of one height a refill zeroes
struct SlotClear {
    double *pn[kSlotPanels], *pm[kSlotPanels];  // the n-row and the m-row panels whose listed columns become 0.0
    int npn, npm, n, m;
    double *SC;  // B_NSLOT_DETECT scalar slots per member
    BatchCtl ctl;
    double *bsc, *csc;
    const double *q_sigma, *q_bs, *q_cs;  // per problem of the staged queue
};
// What a fresh workspace holds for a member, for the listed slots: zero work panels (with detection: the four ray panels), zero
// counters, restart flag and scalar slots; sigma, b_scale, c_scale of the slot's problem and active = 1.
// grid (ceil(max(n, m) * np / 256), npn + npm + 1): y < npn + npm one panel each, the last y the control values.
__global__ void __launch_bounds__(256) kb_slot_clear(SlotClear a, const SlotPair *pairs, int np, Geo g) {
    const int v = blockIdx.y;
    const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    if (v == a.npn + a.npm) {
        if (e >= np) return;
        const SlotPair pr = pairs[e];
        const int k = pr.slot;
        for (int s = 0; s < B_NSLOT_DETECT; ++s) a.SC[static_cast<size_t>(s) * g.Bp + k] = 0.0;
        a.ctl.sigma[k] = a.q_sigma[pr.problem];
        a.bsc[k] = a.q_bs[pr.problem];
        a.csc[k] = a.q_cs[pr.problem];
        a.ctl.kx[k] = 0;
        a.ctl.ky[k] = 0;
        a.ctl.restart_flag[k] = 0;
        a.ctl.active[k] = 1;
        return;
    }
    const int rows = v < a.npn ? a.n : a.m;
    double *__restrict__ P = v < a.npn ? a.pn[v] : a.pm[v - a.npn];
    const long i = e / np;
    if (i >= rows) return;
    P[slot_elem(g, rows, static_cast<int>(i), pairs[e % np].slot)] = 0.0;
}

struct SlotIn {
    const double *src[kPanelVectors];  // the staged queue's regions, column-major rows x count
    double *dst[kPanelVectors];        // padded panels
    int rows[kPanelVectors];
};
// The listed problems' scaled vectors from the staged queue into their slots' columns: a copy, element for element what
// kb_panel_in writes for a member.  grid (ceil(max rows * np / 256), vectors).
__global__ void __launch_bounds__(256) kb_slot_in(SlotIn a, const SlotPair *pairs, int np, Geo g) {
    const int v = blockIdx.y, rows = a.rows[v];
    const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    const long i = e / np;
    if (i >= rows) return;
    const SlotPair pr = pairs[e % np];
    a.dst[v][slot_elem(g, rows, static_cast<int>(i), pr.slot)] = a.src[v][static_cast<size_t>(pr.problem) * rows + i];
}

constexpr int kSlotOutVectors = 6;  // x, y, z and, with detection, the rays d, y, A^T y, in that order ...
constexpr int kSlotOutPlain = 3, kSlotOutDual = 4;  // ... so that a pass copies as many as its verdicts need: none, a dual one, a primal one
enum SlotOutMap : int { SLOT_OUT_POINT = 0, SLOT_OUT_REDUCED_COST, SLOT_OUT_RAW };
struct SlotOut {
    const double *src[kSlotOutVectors];    // padded panels
    double *dst[kSlotOutVectors];          // the result block's regions, column-major rows x count
    const double *norm[kSlotOutVectors];   // cn / rn (unread for SLOT_OUT_RAW)
    const double *scale[kSlotOutVectors];  // per SLOT: b_scale / c_scale
    int rows[kSlotOutVectors], map[kSlotOutVectors];
};
// The listed slots' columns into column `problem` of the result block.  x, y, z in the caller's units by point_to_caller and
// reduced_cost_to_caller (batch_units.h), as kb_panel_out has them; the rays as they are (finish_certificate maps them on the host).
// grid (ceil(max rows * np / 256), vectors).
__global__ void __launch_bounds__(256) kb_slot_out(SlotOut a, const SlotPair *pairs, int np, Geo g) {
    const int v = blockIdx.y, rows = a.rows[v];
    const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    const long i = e / np;
    if (i >= rows) return;
    const SlotPair pr = pairs[e % np];
    const double p = a.src[v][slot_elem(g, rows, static_cast<int>(i), pr.slot)];
    double r = p;
    if (a.map[v] == SLOT_OUT_POINT) r = point_to_caller(p, a.norm[v][i], a.scale[v][pr.slot]);
    else if (a.map[v] == SLOT_OUT_REDUCED_COST) r = reduced_cost_to_caller(p, a.norm[v][i], a.scale[v][pr.slot]);
    a.dst[v][static_cast<size_t>(pr.problem) * rows + i] = r;
}

// ---- a batch from device memory (DESIGN.md "Device-resident batches") ------------------------------------------------------------
// prepare_batch (batch_prep.cpp) on the device: the same element and scalar functions (batch_units.h) in the same order, the norms
// by the tree rule of batch_prep.h.  The caller's vectors are column-major rows x B, so a segment of one member is one contiguous
// run: a 256-thread workgroup per (segment, member, vector group) reads it coalesced, thread j is lane j of the rule, and the
// workgroup leaves one partial per sum.  Group 0: the n-row vectors C, l, u; group 1: the m-row vectors AL, AU.  Partial (group g,
// sum a, member k, segment s) sits at part[((g * 2 + a) * B + k) * nseg + s], nseg = the segments of the longer vector.  The
// per-member scalars live in `scal`, 7 x B in BATCH_SCALARS' order (b_scale, c_scale, norm_b, norm_c, norm_b_org, norm_c_org,
// sigma), followed by two flag words.
// Both norm passes come in two forms.  A batch (DESIGN.md "Device-resident batches") is staged: the passes store what they compute
// into the staging block's regions.  A queue (DESIGN.md "Device-resident streams") is not: the same loads and operations, nothing
// stored beside the partials -- no scaled copy of the queue exists, a problem is scaled when it enters a slot (kb_slot_scale).
// grid (nseg, members of the slice, 2); k0: the slice's first member (a grid's y dimension holds 65535; a batch has one slice).
enum DataScalar : int { DS_B_SCALE = 0, DS_C_SCALE, DS_NORM_B, DS_NORM_C, DS_NORM_B_ORG, DS_NORM_C_ORG, DS_SIGMA, DS_COUNT };
enum DataFlag : int { DF_START = 0, DF_RESULT, DF_COUNT };  // a non-finite entry in X0 / Y0; in the x / y of the results

// The fold of the tree rule for NSUM sums at once: acc[i] of thread j is lane j's sum.  Strides 128 and 64 cross the waves
// through LDS; strides 32 .. 1 stay inside wave 0 (lane j takes lane j + stride's value: for j < stride that is a[j] += a[j + stride]).
// Thread 0 returns with the segment sums in acc.
template <int NSUM>
__device__ __forceinline__ void tree_fold(double (&acc)[NSUM]) {
    static_assert(kNormLanes == 256, "the fold below is written for 256 lanes = 4 waves");
    __shared__ double red[NSUM][kNormLanes];
    const int j = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NSUM; ++i) red[i][j] = acc[i];
    __syncthreads();
    if (j < 128) {
#pragma unroll
        for (int i = 0; i < NSUM; ++i) red[i][j] += red[i][j + 128];
    }
    __syncthreads();
    if (j < 64) {
#pragma unroll
        for (int i = 0; i < NSUM; ++i) {
            double v = red[i][j] + red[i][j + 64];
#pragma unroll
            for (int stride = 32; stride >= 1; stride >>= 1) v += __shfl_down(v, stride, 64);
            acc[i] = v;
        }
    }
}

struct DataIn {
    const double *C, *L, *U, *AL, *AU;  // the caller's, column-major (a queue: L, U unread)
    double *oC, *oL, *oU, *oAL, *oAU;   // the staging block's regions (a queue: none)
    const double *cn, *rn;
    double *part;
    int n, m, nseg;
};
// The first step by cn / rn.  sum 0: the caller's values' sum of squares, sum 1: the values' after the step.  STAGED: the values
// after the step go to the regions.
template <bool STAGED>
__global__ void __launch_bounds__(kNormLanes) kb_data_in(DataIn a, int B, int k0) {
    const int s = blockIdx.x, k = k0 + blockIdx.y, g = blockIdx.z;
    const int rows = g ? a.m : a.n;
    const int i0 = s * kNormSeg;
    if (i0 >= rows) return;  // (uniform per workgroup)
    const int end = min(rows, i0 + kNormSeg);
    const size_t base = static_cast<size_t>(k) * rows;
    double acc[2] = {0.0, 0.0};
    if (g == 0) {
        for (int i = i0 + threadIdx.x; i < end; i += kNormLanes) {
            const double nrm = a.cn[i];
            const double c = a.C[base + i];
            const double t0 = c * c;
            acc[0] += t0;
            const double cs = over_norm(c, nrm);
            const double t1 = cs * cs;
            acc[1] += t1;
            if (STAGED) {
                a.oC[base + i] = cs;
                a.oL[base + i] = times_norm(a.L[base + i], nrm);
                a.oU[base + i] = times_norm(a.U[base + i], nrm);
            }
        }
    } else {
        for (int i = i0 + threadIdx.x; i < end; i += kNormLanes) {
            const double nrm = a.rn[i];
            double lo = a.AL[base + i], hi = a.AU[base + i];
            const double v0 = bound_value(lo, hi);
            const double t0 = v0 * v0;
            acc[0] += t0;
            lo = over_norm(lo, nrm);
            hi = over_norm(hi, nrm);
            const double v1 = bound_value(lo, hi);
            const double t1 = v1 * v1;
            acc[1] += t1;
            if (STAGED) {
                a.oAL[base + i] = lo;
                a.oAU[base + i] = hi;
            }
        }
    }
    tree_fold<2>(acc);
    if (threadIdx.x == 0) {
        a.part[(static_cast<size_t>(g * 2 + 0) * B + k) * a.nseg + s] = acc[0];
        a.part[(static_cast<size_t>(g * 2 + 1) * B + k) * a.nseg + s] = acc[1];
    }
}

// the segment partials of (group g, sum a, member k), added in increasing s from 0.0
__device__ __forceinline__ double segment_total(const double *part, int g, int a, int B, int k, int nseg, int rows) {
    const double *p = part + (static_cast<size_t>(g * 2 + a) * B + k) * nseg;
    double total = 0.0;
    for (int s = 0; s < norm_segments(rows); ++s) total += p[s];
    return total;
}

// one thread per member: norm_b_org, norm_c_org of the caller's data; b_scale, c_scale (1.0 without use_bc_scaling)
__global__ void __launch_bounds__(256) kb_data_scales(const double *part, int B, int n, int m, int nseg, int use_bc, double *scal) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    scal[DS_NORM_C_ORG * B + k] = one_plus_norm(segment_total(part, 0, 0, B, k, nseg, n));
    scal[DS_NORM_B_ORG * B + k] = one_plus_norm(segment_total(part, 1, 0, B, k, nseg, m));
    scal[DS_C_SCALE * B + k] = use_bc ? one_plus_norm(segment_total(part, 0, 1, B, k, nseg, n)) : 1.0;
    scal[DS_B_SCALE * B + k] = use_bc ? one_plus_norm(segment_total(part, 1, 1, B, k, nseg, m)) : 1.0;
}

struct DataBc {
    const double *C, *L, *U, *AL, *AU;  // STAGED: the staging block's regions after the first pass; else the caller's (L, U unread)
    double *oC, *oL, *oU, *oAL, *oAU;   // STAGED: the same regions (the pass works in place); else none
    const double *X0, *Y0;              // the caller's starts (null: none) ...
    double *oX0, *oY0;                  // ... and, STAGED, their regions
    const double *cn, *rn;
    const double *scal;
    double *part;
    int *flags;
    int n, m, nseg;
};
// The second step by the scales kb_data_scales left (by 1.0 without use_bc_scaling: exact); sum 0: the final values' sum of
// squares, before any +-kInfReplacement.  A non-finite entry of the caller's starts raises flags[DF_START].  STAGED: reads the
// regions the first pass wrote and rewrites them, infinite sides and bounds replaced, and the starts go to their regions by
// start_to_scaled.  Not STAGED: reads the caller's arrays, applies the first step again and stores nothing.
template <bool STAGED>
__global__ void __launch_bounds__(kNormLanes) kb_data_bc(DataBc a, int B, int k0) {
    const int s = blockIdx.x, k = k0 + blockIdx.y, g = blockIdx.z;
    const int rows = g ? a.m : a.n;
    const int i0 = s * kNormSeg;
    if (i0 >= rows) return;
    const int end = min(rows, i0 + kNormSeg);
    const size_t base = static_cast<size_t>(k) * rows;
    const double bs = a.scal[DS_B_SCALE * B + k], cs = a.scal[DS_C_SCALE * B + k];
    double acc[1] = {0.0};
    bool bad = false;
    if (g == 0) {
        for (int i = i0 + threadIdx.x; i < end; i += kNormLanes) {
            const double c1 = STAGED ? a.C[base + i] : over_norm(a.C[base + i], a.cn[i]);
            const double c = by_scale(c1, cs);
            const double t = c * c;
            acc[0] += t;
            if (STAGED) {
                a.oC[base + i] = c;
                a.oL[base + i] = lower_replaced(by_scale(a.L[base + i], bs));
                a.oU[base + i] = upper_replaced(by_scale(a.U[base + i], bs));
            }
            if (a.X0) {
                const double x = a.X0[base + i];
                bad = bad || !isfinite(x);
                if (STAGED) a.oX0[base + i] = start_to_scaled(x, a.cn[i], bs);
            }
        }
    } else {
        for (int i = i0 + threadIdx.x; i < end; i += kNormLanes) {
            const double lo1 = STAGED ? a.AL[base + i] : over_norm(a.AL[base + i], a.rn[i]);
            const double hi1 = STAGED ? a.AU[base + i] : over_norm(a.AU[base + i], a.rn[i]);
            const double lo = by_scale(lo1, bs), hi = by_scale(hi1, bs);
            const double v = bound_value(lo, hi);
            const double t = v * v;
            acc[0] += t;
            if (STAGED) {
                a.oAL[base + i] = lower_replaced(lo);
                a.oAU[base + i] = upper_replaced(hi);
            }
            if (a.Y0) {
                const double y = a.Y0[base + i];
                bad = bad || !isfinite(y);
                if (STAGED) a.oY0[base + i] = start_to_scaled(y, a.rn[i], cs);
            }
        }
    }
    if (bad) a.flags[DF_START] = 1;  // (every writer writes the same word)
    tree_fold<1>(acc);
    if (threadIdx.x == 0) a.part[(static_cast<size_t>(g * 2) * B + k) * a.nseg + s] = acc[0];
}

// one thread per member of the PADDED batch: norm_b, norm_c of the final vectors (sum 0 of the second pass) and the first sigma
// into scal, and, where hdr is given, the header of the staging block as ws_fill reads it: sigma | b_scale | c_scale (padding
// members 1.0) | active (ints: 1 for a member, 0 for padding).  A queue has no header (its slots' is the host's) and no padding.
__global__ void __launch_bounds__(256) kb_data_header(const double *part, int B, int Bp, int n, int m, int nseg, double *scal, double *hdr) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Bp) return;
    double sigma = 1.0, bs = 1.0, cs = 1.0;
    if (k < B) {
        const double nc = sqrt(segment_total(part, 0, 0, B, k, nseg, n)), nb = sqrt(segment_total(part, 1, 0, B, k, nseg, m));
        sigma = first_sigma(nb, nc);
        scal[DS_NORM_B * B + k] = nb;
        scal[DS_NORM_C * B + k] = nc;
        scal[DS_SIGMA * B + k] = sigma;
        bs = scal[DS_B_SCALE * B + k];
        cs = scal[DS_C_SCALE * B + k];
    }
    if (!hdr) return;
    hdr[k] = sigma;
    hdr[Bp + k] = bs;
    hdr[2 * Bp + k] = cs;
    reinterpret_cast<int *>(hdr + 3 * static_cast<size_t>(Bp))[k] = k < B ? 1 : 0;
}

// raises *flag where one of the first `count` values of v is not finite (the x / y a device-entry call has just written)
__global__ void __launch_bounds__(256) kb_flag_nonfinite(const double *x, size_t nx, const double *y, size_t ny, int *flag) {
    bool bad = false;
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nx + ny; i += stride)
        bad = bad || !isfinite(i < nx ? x[i] : y[i - nx]);
    if (bad) *flag = 1;
}

// ---- a queue in device memory (DESIGN.md "Device-resident streams") ----------------------------------------------------------------
// The listed problems from the CALLER's arrays into their slots' columns in scaled units: kb_slot_in's geometry and table, and per
// element the steps of batch_units.h that the two norm passes apply to a staged batch, each rounding kept -- the first by cn / rn
// (SF_TIMES_NORM: times_norm, else over_norm), the second by b_scale[p] (SF_BY_C: c_scale[p]), then lower_replaced (SF_LOWER) or
// upper_replaced (SF_UPPER).  A start is a bound without a replacement: times_norm and by_scale are start_to_scaled.
enum SlotScaleOp : int { SF_TIMES_NORM = 1, SF_BY_C = 2, SF_LOWER = 4, SF_UPPER = 8 };
struct SlotScale {
    const double *src[kPanelVectors];   // the caller's arrays, column-major rows x count
    double *dst[kPanelVectors];         // padded panels
    const double *norm[kPanelVectors];  // cn / rn
    int rows[kPanelVectors], op[kPanelVectors];
    const double *q_bs, *q_cs;          // per problem of the queue
};
// grid (ceil(max rows * np / 256), vectors)
__global__ void __launch_bounds__(256) kb_slot_scale(SlotScale a, const SlotPair *pairs, int np, Geo g) {
    const int v = blockIdx.y, rows = a.rows[v], op = a.op[v];
    const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    const long i = e / np;
    if (i >= rows) return;
    const SlotPair pr = pairs[e % np];
    const double x = a.src[v][static_cast<size_t>(pr.problem) * rows + i], nrm = a.norm[v][i];
    const double x1 = (op & SF_TIMES_NORM) ? times_norm(x, nrm) : over_norm(x, nrm);
    double r = by_scale(x1, (op & SF_BY_C) ? a.q_cs[pr.problem] : a.q_bs[pr.problem]);
    if (op & SF_LOWER) r = lower_replaced(r);
    if (op & SF_UPPER) r = upper_replaced(r);
    a.dst[v][slot_elem(g, rows, static_cast<int>(i), pr.slot)] = r;
}

// ---- a start from a result column (DESIGN.md "Streamed batches", "Parents") --------------------------------------------------------
// The listed problems' starts into their slots' columns of X (v = 0) and Y (v = 1): kb_slot_scale's geometry and table, and beside
// each pair the pass's table carries the start's SOURCE.  source >= 0: that column of the result x / y -- the parent's returned
// point, which kb_slot_out wrote in the caller's units earlier on this stream; source <= kSourceOwn: column kSourceOwn - source of
// the caller's X0 / Y0 (a root's own); kSourceNone: a cold root, whose columns become 0.0.  The stored value is start_to_scaled of
// the source -- times_norm by cn / rn, then by_scale by the ENTERING problem's b_scale / c_scale: what kb_slot_scale does to a start.
constexpr int kSourceNone = -1, kSourceOwn = -2;
struct SlotStart {
    const double *res[2];   // the result's x, y (a device-entry call: the caller's dx, dy), column-major rows x count
    const double *own[2];   // the caller's X0, Y0 (null: the call has none)
    double *dst[2];         // the padded panels X, Y
    const double *norm[2];  // cn, rn
    int rows[2];
    const double *q_bs, *q_cs;  // per problem of the queue
    const int *source;          // per listed pair
};
// grid (ceil(max rows * np / 256), 2)
__global__ void __launch_bounds__(256) kb_slot_start(SlotStart a, const SlotPair *pairs, int np, Geo g) {
    const int v = blockIdx.y, rows = a.rows[v];
    const long e = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
    const long i = e / np;
    if (i >= rows) return;
    const int j = static_cast<int>(e % np);
    const SlotPair pr = pairs[j];
    const int s = a.source[j];
    double r = 0.0;
    if (s != kSourceNone) {
        const double *col = s >= 0 ? a.res[v] + static_cast<size_t>(s) * rows : a.own[v] + static_cast<size_t>(kSourceOwn - s) * rows;
        r = start_to_scaled(col[i], a.norm[v][i], v == 0 ? a.q_bs[pr.problem] : a.q_cs[pr.problem]);
    }
    a.dst[v][slot_elem(g, rows, static_cast<int>(i), pr.slot)] = r;
}

// ---- host side ----------------------------------------------------------------------------------
// BatchedSolver::solve at the end of the file is the order of things; every kernel is launched by a named launcher.
struct BatchWS {
    // -- depends on the matrix only (and on the chunk geometry): ws_matrix_part
    int m = 0, n = 0;
    Solver *shared = nullptr;  // scaled A, A^T, row_norm, col_norm
    std::vector<double> rn, cn;  // ... and the host's copies of the two (fetched by solve_batched_impl)
    hipStream_t stream = nullptr;
    Geo geo{};
    int gx = 1, gy = 1;  // row blocks of the n- / m-row launches with partials (the grid is geo.nchunk times that)
    int grid_cap = 0;    // HPRLP_BATCH_GRID of this call: most row blocks of a normal half-step launch (0: as many as the rows need)
    DBuf<int> order_x, order_y;  // launch order of the 4-row groups of A^T / A in kb_half64 (groups with long rows first)
    // -- sized by the padded batch and the chunk geometry, kept while those stay (ws_panels); filled per batch (ws_fill)
    int B = 0, Bp = 0;
    const BatchData *data = nullptr;
    DBuf<double> C, AL, AU, L, U;
    DBuf<double> X, Xh, Xb, DX, Zb, lastX, Y, Yb, DY, Yobj, lastY;
    DBuf<double> sigma, SC, partials;
    DBuf<int> active, kx, ky, rflag;
    DBuf<double> bsc, csc, bsc_prev, csc_prev;  // b / c scales per member of this batch and of the one before (kb_carry_start)
    // infeasibility detection (allocated at its first use): previous X_bar / Y_bar, the rays, the certificates' z
    DBuf<double> prevX, DS, prevY, YS, Zray;
    int nslot = B_NSLOT;  // scalar slots per member that fetch() brings back (B_NSLOT_DETECT with detection on; SC holds those always)
    HBuf<double> SC_h;
    // a batch's way in and out: device block and its pinned twin, column-major regions (BatchedSolver::solve lays them out)
    DBuf<double> stage_d;
    HBuf<double> stage_h;
    // a device-entry call (DESIGN.md "Device-resident batches"): the segment partials of its norms; the per-member scalars
    // (DS_COUNT x B) with the DF_COUNT flag words behind them, and their pinned twin
    DBuf<double> data_part, data_scal;
    HBuf<double> data_scal_h;
    // a streamed call (DESIGN.md "Streamed batches"): the result block (x, y, z and, with detection, the rays: column p = problem
    // p); the refill pass's tables and start mask on the device, and their pinned twin
    DBuf<double> res_d;
    DBuf<int> tab_d;
    HBuf<int> tab_h;
    BatchCtl ctl{};
    double lambda_max = 1.0;
    long bumps = 0;  // evaluations of the weighted norm that raised lambda_max, over the handle's life
    std::map<int, hipGraphExec_t> graphs;
    double graph_lambda = 0.0;  // the lambda_max the graphs alive were captured with
    long captures = 0, panel_allocs = 0;
    // The captured launches hold lambda_max BY VALUE (HalfArgs), and every panel's address: whoever changes one of them drops
    // them, and run_normal captures anew.
    void drop_graphs() {
        for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
    ~BatchWS() { drop_graphs(); }
};

int grid_for(int rows, const Geo &g) {
    long need = (static_cast<long>(rows) + g.rows_per_block - 1) / g.rows_per_block;
    return static_cast<int>(std::max(1L, std::min(need, 2048L)));
}

void finalize(BatchWS &w, int nblocks, std::initializer_list<int> slots, unsigned max_mask = 0) {
    BFin f{};
    f.nacc = 0;
    f.max_mask = max_mask;
    for (int s : slots) f.slot[f.nacc++] = s;
    hipLaunchKernelGGL(kb_finalize, dim3((w.Bp + 63) / 64, f.nacc), dim3(1024), 0, w.stream, w.partials.p, nblocks, w.Bp, f,
                       w.SC.p);
}

void launch_half_pair(BatchWS &w, bool check) {
    const CsrDev &A = w.shared->A.view, &AT = w.shared->AT.view;
    HalfArgs xa{w.Y.p, w.m, w.X.p, w.Xh.p, w.L.p, w.U.p, w.C.p, w.lastX.p, w.Xb.p, w.Zb.p, w.DX.p, w.ctl, w.lambda_max, w.partials.p, w.order_x.p};
    HalfArgs ya{w.Xh.p, w.n, w.Y.p, nullptr, w.AL.p, w.AU.p, nullptr, w.lastY.p, w.Yb.p, w.Yobj.p, w.DY.p, w.ctl, w.lambda_max, w.partials.p, w.order_y.p};
    const Geo &g = w.geo;
    const dim3 gxd(w.gx * g.nchunk), gyd(w.gy * g.nchunk), blk(256);
    // kernel by chunk width: 64 -> a wave = one row (kb_half64); 8 / 16 / 32 -> lane groups with their own rows (kb_halfN);
    // below: the plain row loop (kb_half)
    auto launch = [&](auto xhalf, auto check, dim3 grid, const CsrDev &M, const HalfArgs &ha) {
        constexpr bool X = decltype(xhalf)::value, C = decltype(check)::value;
        switch (g.Bw) {
            case 64: hipLaunchKernelGGL((kb_half64<X, C>), grid, blk, 0, w.stream, M.rows, M.rowptr, M.col, M.val, g, ha); break;
            case 32: hipLaunchKernelGGL((kb_halfN<X, C, 32>), grid, blk, 0, w.stream, M.rows, M.rowptr, M.col, M.val, g, ha); break;
            case 16: hipLaunchKernelGGL((kb_halfN<X, C, 16>), grid, blk, 0, w.stream, M.rows, M.rowptr, M.col, M.val, g, ha); break;
            case 8: hipLaunchKernelGGL((kb_halfN<X, C, 8>), grid, blk, 0, w.stream, M.rows, M.rowptr, M.col, M.val, g, ha); break;
            default: hipLaunchKernelGGL((kb_half<X, C>), grid, blk, 0, w.stream, M.rows, M.rowptr, M.col, M.val, g, ha); break;
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    if (check) {
        launch(T{}, T{}, gxd, AT, xa);
        finalize(w, w.gx, {B_CX, B_XZ, B_DX2});
        launch(F{}, T{}, gyd, A, ya);
        finalize(w, w.gy, {B_YOBJ_Y, B_DY2});
    } else {
        // no reduction partials in the normal variant: one pass over the rows, as many workgroups as rows need
        const int rpb = g.Bw >= 8 ? 4 * kRowsPerWave * (64 / g.Bw) : g.rows_per_block;
        auto cap = [&](int gr) { return w.grid_cap > 0 ? std::min(gr, w.grid_cap) : gr; };
        launch(T{}, F{}, dim3(cap((AT.rows + rpb - 1) / rpb) * g.nchunk), AT, xa);
        launch(F{}, F{}, dim3(cap((A.rows + rpb - 1) / rpb) * g.nchunk), A, ya);
    }
}

void run_normal(BatchWS &w, int count) {
    if (!w.shared->use_graph) {  // HPRLP_NO_GRAPH=1 (read by the shared solver's set-up): the same launches, eagerly
        for (int i = 0; i < count; ++i) launch_half_pair(w, false);
        return;
    }
    while (count > 0) {
        const int len = std::min(count, 32);
        auto it = w.graphs.find(len);
        hipGraphExec_t ge;
        if (it == w.graphs.end()) {
            hipGraph_t g = nullptr;
            HIP_CHECK(hipStreamBeginCapture(w.stream, hipStreamCaptureModeThreadLocal));
            for (int i = 0; i < len; ++i) launch_half_pair(w, false);
            HIP_CHECK(hipStreamEndCapture(w.stream, &g));
            HIP_CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphDestroy(g));
            if (w.graphs.empty()) w.graph_lambda = w.lambda_max;
            w.graphs[len] = ge;
            ++w.captures;
        } else {
            ge = it->second;
        }
        HIP_CHECK(hipGraphLaunch(ge, w.stream));
        count -= len;
    }
}

// The launches with kb_resid's geometry: x-side ones run over the n rows of A^T (w.gx row blocks), y-side ones over the m rows of
// A (w.gy), elementwise ones over both (the larger of the two); each is followed by the finalize of the slots it fills.
constexpr const double *kUnread = nullptr;  // an operand that the launched variant of a kernel does not read
inline dim3 grid_of(const BatchWS &w, int row_blocks) { return dim3(row_blocks * w.geo.nchunk); }
inline int both_grids(const BatchWS &w) { return std::max(w.gx, w.gy); }

// compute_residuals :578-624, dual part: |(C - A^T Ybar - Zbar) .* col_norm|^2
void launch_dual_residual(BatchWS &w) {
    const CsrDev &AT = w.shared->AT.view;
    hipLaunchKernelGGL((kb_resid<0>), grid_of(w, w.gx), dim3(256), 0, w.stream, AT.rows, AT.rowptr, AT.col, AT.val, w.geo, w.m,
                       /*V*/ w.Yb.p, /*V2*/ kUnread, /*p0*/ w.C.p, /*p1*/ w.Zb.p, /*norm*/ w.shared->col_norm.p, /*dvec*/ kUnread,
                       w.partials.p);
    finalize(w, w.gx, {B_RD2});
}
// ... primal part: |row_norm .* (A Xbar out of [AL, AU])|^2
void launch_primal_residual(BatchWS &w) {
    const CsrDev &A = w.shared->A.view;
    hipLaunchKernelGGL((kb_resid<1>), grid_of(w, w.gy), dim3(256), 0, w.stream, A.rows, A.rowptr, A.col, A.val, w.geo, w.n,
                       /*V*/ w.Xb.p, /*V2*/ kUnread, /*p0*/ w.AL.p, /*p1*/ w.AU.p, /*norm*/ w.shared->row_norm.p, /*dvec*/ kUnread,
                       w.partials.p);
    finalize(w, w.gy, {B_RP2});
}
// the weighted norm's <A DX, DY>
void launch_cross_term(BatchWS &w) {
    const CsrDev &A = w.shared->A.view;
    hipLaunchKernelGGL((kb_resid<3>), grid_of(w, w.gy), dim3(256), 0, w.stream, A.rows, A.rowptr, A.col, A.val, w.geo, w.n,
                       /*V*/ kUnread, /*V2*/ w.DX.p, /*p0*/ kUnread, /*p1*/ kUnread, /*norm*/ kUnread, /*dvec*/ w.DY.p, w.partials.p);
    finalize(w, w.gy, {B_ADX_DY});
}
void launch_bound_violation(BatchWS &w) {  // iteration 0 only
    hipLaunchKernelGGL(kb_lu, grid_of(w, w.gx), dim3(256), 0, w.stream, w.n, w.geo, w.Xb.p, w.L.p, w.U.p, w.shared->col_norm.p,
                       w.DX.p, w.partials.p);
    finalize(w, w.gx, {B_LU2});
}
// update_sigma :702-745, device part: movement norms for every problem
void launch_movement(BatchWS &w) {
    hipLaunchKernelGGL(kb_movement, grid_of(w, both_grids(w)), dim3(256), 0, w.stream, w.n, w.m, w.geo, w.Xb.p, w.lastX.p, w.DX.p,
                       w.Yb.p, w.lastY.p, w.DY.p, w.partials.p);
    finalize(w, both_grids(w), {B_MOVE_X2, B_MOVE_Y2});
}
void launch_restart_copy(BatchWS &w) {  // do_restart :747-769
    hipLaunchKernelGGL(kb_restart, grid_of(w, both_grids(w)), dim3(256), 0, w.stream, w.n, w.m, w.geo, w.X.p, w.lastX.p, w.Xb.p,
                       w.Y.p, w.lastY.p, w.Yb.p, w.ctl);
}
constexpr const int *kAllMembers = nullptr;  // the start kernels' mask of a plain solve
void launch_start_seed(BatchWS &w, const int *mask) {
    hipLaunchKernelGGL(kb_start_seed, grid_of(w, both_grids(w)), dim3(256), 0, w.stream, w.n, w.m, w.geo, w.X.p, w.Xh.p, w.Xb.p,
                       w.lastX.p, w.L.p, w.U.p, w.Y.p, w.Yb.p, w.lastY.p, w.AL.p, w.AU.p, mask);
}
void launch_start_col(BatchWS &w, const int *mask) {  // Z_bar, C.X_bar and the bound terms of the start
    const CsrDev &AT = w.shared->AT.view;
    hipLaunchKernelGGL(kb_start_spmm<true>, grid_of(w, w.gx), dim3(256), 0, w.stream, AT.rows, AT.rowptr, AT.col, AT.val, w.geo, w.m,
                       /*V*/ w.Yb.p, /*p0*/ w.C.p, /*lo*/ w.L.p, /*hi*/ w.U.p, /*bar*/ w.Xb.p, /*out*/ w.Zb.p, w.partials.p, mask);
    finalize(w, w.gx, {B_CX, B_XZ});
}
void launch_start_row(BatchWS &w, const int *mask) {  // Y_obj and Y_obj.Y_bar of the start
    const CsrDev &A = w.shared->A.view;
    hipLaunchKernelGGL(kb_start_spmm<false>, grid_of(w, w.gy), dim3(256), 0, w.stream, A.rows, A.rowptr, A.col, A.val, w.geo, w.n,
                       /*V*/ w.Xb.p, /*p0*/ kUnread, /*lo*/ w.AL.p, /*hi*/ w.AU.p, /*bar*/ w.Yb.p, /*out*/ w.Yobj.p, w.partials.p, mask);
    finalize(w, w.gy, {B_YOBJ_Y});
}

// one of a streamed call's slot kernels: a thread per element of the longest vector for each of np listed (slot, problem) pairs, ny vectors
template <class Kernel, class Args>
void launch_slot(BatchWS &w, Kernel kernel, const Args &a, const SlotPair *pairs, int np, int ny) {
    const dim3 grid(static_cast<unsigned>((static_cast<long>(std::max(w.n, w.m)) * np + 255) / 256), ny);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, w.stream, a, pairs, np, w.geo);
    HIP_CHECK(hipGetLastError());
}

void fetch(BatchWS &w) {
    HIP_CHECK(hipMemcpyAsync(w.SC_h.p, w.SC.p, sizeof(double) * w.nslot * w.Bp, hipMemcpyDeviceToHost, w.stream));
    HIP_CHECK(hipStreamSynchronize(w.stream));
}
inline double sc(const BatchWS &w, int slot, int k) { return w.SC_h.p[static_cast<size_t>(slot) * w.Bp + k]; }

RayArgs ray_args(const BatchWS &w) {
    return RayArgs{w.Xb.p, w.Yb.p, w.prevX.p, w.prevY.p, w.DS.p, w.YS.p, w.L.p, w.U.p, w.C.p, w.AL.p, w.AU.p,
                   w.shared->col_norm.p, w.shared->row_norm.p, w.bsc.p, w.csc.p, w.active.p};
}

// Infeasibility detection at a periodic evaluation: the active members' rays and, when `test` (every evaluation but the first,
// which only stores X_bar / Y_bar), their ratio-test scalars into the slots B_RAY_*, fetched with the evaluation's own.
void ray_step(BatchWS &w, bool test) {
    const CsrDev &A = w.shared->A.view, &AT = w.shared->AT.view;
    const Geo &g = w.geo;
    const RayArgs a = ray_args(w);
    const int gf = std::max(w.gx, w.gy);
    hipLaunchKernelGGL(kb_ray_form, dim3(gf * g.nchunk), dim3(256), 0, w.stream, w.n, w.m, g, a, w.partials.p);
    if (!test) return;
    finalize(w, gf, {B_RAY_DY, B_RAY_CD, B_RAY_VY, B_RAY_WD, B_RAY_YN, B_RAY_DN}, 0x3cu);
    hipLaunchKernelGGL(kb_ray_col, dim3(w.gx * g.nchunk), dim3(256), 0, w.stream, AT.rows, AT.rowptr, AT.col, AT.val, g,
                       w.m, static_cast<const double *>(w.YS.p), static_cast<const double *>(w.L.p),
                       static_cast<const double *>(w.U.p), static_cast<const double *>(w.shared->col_norm.p), a, w.partials.p);
    finalize(w, w.gx, {B_RAY_DZ, B_RAY_VZ}, 0x2u);
    hipLaunchKernelGGL(kb_ray_row, dim3(w.gy * g.nchunk), dim3(256), 0, w.stream, A.rows, A.rowptr, A.col, A.val, g,
                       w.n, static_cast<const double *>(w.DS.p), static_cast<const double *>(w.AL.p),
                       static_cast<const double *>(w.AU.p), static_cast<const double *>(w.shared->row_norm.p), a, w.partials.p);
    finalize(w, w.gy, {B_RAY_WQ}, 0x1u);
}
// the certificates' z = -A^T y: the plain product A^T YS for every member, into the scratch panel (no partials, no finalize)
void launch_ray_product(BatchWS &w) {
    const CsrDev &AT = w.shared->AT.view;
    hipLaunchKernelGGL(kb_ray_product, grid_of(w, w.gx), dim3(256), 0, w.stream, AT.rows, AT.rowptr, AT.col, AT.val, w.geo, w.m,
                       /*V*/ static_cast<const double *>(w.YS.p), /*lo*/ kUnread, /*hi*/ kUnread, /*norm*/ kUnread, ray_args(w),
                       w.Zray.p);
}

// member k's ratio-test sums from the fetched ray slots (Solver::ray_scalars)
RayScalars ray_scalars(const BatchWS &w, int k) {
    return RayScalars{sc(w, B_RAY_DY, k) + sc(w, B_RAY_DZ, k), std::max(sc(w, B_RAY_VY, k), sc(w, B_RAY_VZ, k)), sc(w, B_RAY_CD, k),
                      std::max(sc(w, B_RAY_WD, k), sc(w, B_RAY_WQ, k)), sc(w, B_RAY_YN, k), sc(w, B_RAY_DN, k)};
}

// reference compute_weighted_norm :626-666.  DX/DY norms come from the slots the check step filled,
// unless a movement pass has overwritten DX/DY since (then B_MOVE_* hold the matching norms).
void weighted_norm(BatchWS &w, bool dxdy_from_movement, std::vector<double> &sigma, std::vector<double> &out) {
    launch_cross_term(w);
    fetch(w);
    out.assign(w.B, 0.0);
    const double lambda_before = w.lambda_max;
    for (int k = 0; k < w.B; ++k) {
        const double dot_prod = 2.0 * sc(w, B_ADX_DY, k);
        // the reference squares cublasDnrm2 results (:653-654); sqrt-then-square keeps that rounding
        const double dyn = std::sqrt(sc(w, dxdy_from_movement ? B_MOVE_Y2 : B_DY2, k));
        const double dxn = std::sqrt(sc(w, dxdy_from_movement ? B_MOVE_X2 : B_DX2, k));
        const double dy_sq = dyn * dyn, dx_sq = dxn * dxn;
        double value = sigma[k] * (w.lambda_max * dy_sq) + dx_sq / sigma[k] + dot_prod;
        if (value < 0.0 && dy_sq > 0.0) {
            const double cand = -(dot_prod + dx_sq / sigma[k]) / (sigma[k] * dy_sq) * 1.05;
            w.lambda_max = std::max(w.lambda_max, cand);
            value = sigma[k] * (w.lambda_max * dy_sq) + dx_sq / sigma[k] + dot_prod;
        }
        out[k] = std::sqrt(std::max(value, 0.0));
    }
    // a bump: the graphs replay the old lambda (the stream is idle after fetch(): nothing of theirs is in flight)
    if (w.lambda_max != lambda_before) {
        w.drop_graphs();
        ++w.bumps;
    }
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// Launch order of the row groups of one matrix (kb_half64 / kb_halfN): groups of kRowsPerWave rows with more than kLongGroup
// nonzeros go first, longest first; the rest keep their order.  A wave's group: subs = 64 / Bw lane groups of kRowsPerWave rows
// each; its length = the longest lane group's entry count.  `out` stays empty (identity: no table) without a long group.
void build_order(const DBuf<int> &rowptr_dev, int rows, int subs, DBuf<int> &out) {
    constexpr int kLongGroup = 32;
    const int gr = kRowsPerWave * subs;
    out.release();
    std::vector<int> rp(static_cast<size_t>(rows) + 1);
    rowptr_dev.download(rp.data(), rp.size());
    const int ng = (rows + gr - 1) / gr;
    std::vector<int> longg, order;
    order.reserve(static_cast<size_t>(ng));
    auto len = [&](int g) {
        int longest = 0;
        for (int sb = 0; sb < subs; ++sb) {  // lane group sb: rows g * gr + i * subs + sb (kb_halfN; kb_half64: subs = 1)
            int cnt = 0;
            for (int i = 0; i < kRowsPerWave; ++i) {
                const int r = g * gr + i * subs + sb;
                if (r < rows) cnt += rp[r + 1] - rp[r];
            }
            longest = std::max(longest, cnt);
        }
        return longest;
    };
    for (int g = 0; g < ng; ++g)
        if (len(g) > kLongGroup) longg.push_back(g);
    if (longg.empty()) return;
    std::stable_sort(longg.begin(), longg.end(), [&](int x, int y) { return len(x) > len(y); });
    order = longg;
    for (int g = 0; g < ng; ++g)
        if (len(g) <= kLongGroup) order.push_back(g);
    out.alloc(order.size());
    out.upload(order.data(), order.size());
}

// What depends on the (scaled) shared matrix and the chunk geometry alone: grids and order tables (and w.rn / w.cn, which
// BatchedSolver's constructor fetches: the batch's vectors are scaled with them).
void ws_matrix_part(BatchWS &w, Solver &shared, const Geo &geo) {
    w.m = shared.m; w.n = shared.n;
    w.shared = &shared;
    w.stream = shared.stream;
    w.geo = geo;
    w.gx = grid_for(w.n, geo);
    w.gy = grid_for(w.m, geo);
    w.order_x.release();
    w.order_y.release();
    if (geo.Bw >= 8) {
        build_order(shared.AT.rowptr, w.n, 64 / geo.Bw, w.order_x);
        build_order(shared.A.rowptr, w.m, 64 / geo.Bw, w.order_y);
    }
}

std::vector<double> padded(const std::vector<double> &v, int Bp, double pad) {  // per-member values, padding members included
    std::vector<double> out(Bp, pad);
    std::copy(v.begin(), v.end(), out.begin());
    return out;
}

// The buffers of a padded batch in w.geo (:479-532): row-major padded panels of the batch's vectors, work vectors, scalar slots
// (with the detection's: whether a call detects does not move a buffer), control arrays.  Allocation only; ws_fill fills them.
void ws_panels(BatchWS &w) {
    const size_t Bp = static_cast<size_t>(w.geo.Bp), nB = w.n * Bp, mB = w.m * Bp;
    w.Bp = w.geo.Bp;
    for (DBuf<double> *p : {&w.C, &w.L, &w.U, &w.X, &w.Xh, &w.Xb, &w.DX, &w.Zb, &w.lastX}) p->alloc(nB);
    for (DBuf<double> *p : {&w.AL, &w.AU, &w.Y, &w.Yb, &w.DY, &w.Yobj, &w.lastY}) p->alloc(mB);
    for (DBuf<double> *p : {&w.prevX, &w.DS, &w.prevY, &w.YS, &w.Zray}) p->release();
    w.SC.alloc(B_NSLOT_DETECT * Bp);
    w.SC_h.alloc(B_NSLOT_DETECT * Bp);
    w.partials.alloc(static_cast<size_t>(std::max(w.gx, w.gy)) * kRayFormAccs * Bp);
    for (DBuf<double> *p : {&w.sigma, &w.bsc, &w.csc, &w.bsc_prev, &w.csc_prev}) p->alloc(Bp);
    for (DBuf<int> *p : {&w.active, &w.kx, &w.ky, &w.rflag}) p->alloc(Bp);
    w.ctl = BatchCtl{w.sigma.p, w.active.p, w.kx.p, w.ky.p, w.rflag.p};
    ++w.panel_allocs;
}

template <class T>
void zero_async(BatchWS &w, DBuf<T> &b) {
    HIP_CHECK(hipMemsetAsync(b.p, 0, (b.n ? b.n : 1) * sizeof(T), w.stream));
}

// The detection's panels, allocated at their first use in this geometry, and zeroed: no stored iterate, no rays.  (A detecting
// solve's ws_fill, and the ray step outside the loop where it starts over: batched_solver_ray_step.)
void ws_ray_panels(BatchWS &w) {
    const size_t Bp = static_cast<size_t>(w.Bp);
    if (!w.prevX.p) {
        for (DBuf<double> *p : {&w.prevX, &w.DS}) p->alloc(w.n * Bp);
        for (DBuf<double> *p : {&w.prevY, &w.YS}) p->alloc(w.m * Bp);
        ++w.panel_allocs;
    }
    for (DBuf<double> *p : {&w.prevX, &w.DS, &w.prevY, &w.YS}) zero_async(w, *p);
}

// One batch into the resident buffers, all of it on the stream.  The pinned block holds, in this order: sigma, b_scale, c_scale
// (Bp doubles each), active (Bp ints in the room of Bp doubles), then the column-major regions of `in` (BatchedSolver::solve
// wrote all of them there).  carry: X / Y from the panels of the batch before (kb_carry_start, before anything is zeroed;
// bsc_prev / csc_prev hold that batch's scales).  Zeroed: what a fresh workspace has zeroed -- the work panels, counters, flags, slots and partials.
// stage_count 0: a device-entry call, whose kernels have left the header and the regions in the staging block already.
// nvec 0: the header alone (a device-entry stream); no panel of the batch's vectors is written here.
void ws_fill(BatchWS &w, const BatchData &d, size_t stage_count, const PanelIn &in, int nvec, bool has_x, bool has_y, bool carry,
             bool detect) {
    const int m = w.m, n = w.n;
    const size_t Bp = static_cast<size_t>(w.Bp);
    w.B = d.B;
    w.data = &d;
    w.nslot = detect ? B_NSLOT_DETECT : B_NSLOT;
    if (stage_count) HIP_CHECK(hipMemcpyAsync(w.stage_d.p, w.stage_h.p, stage_count * sizeof(double), hipMemcpyHostToDevice, w.stream));
    const double *hd = w.stage_d.p;
    HIP_CHECK(hipMemcpyAsync(w.sigma.p, hd, Bp * sizeof(double), hipMemcpyDeviceToDevice, w.stream));
    HIP_CHECK(hipMemcpyAsync(w.bsc.p, hd + Bp, Bp * sizeof(double), hipMemcpyDeviceToDevice, w.stream));
    HIP_CHECK(hipMemcpyAsync(w.csc.p, hd + 2 * Bp, Bp * sizeof(double), hipMemcpyDeviceToDevice, w.stream));
    HIP_CHECK(hipMemcpyAsync(w.active.p, hd + 3 * Bp, Bp * sizeof(int), hipMemcpyDeviceToDevice, w.stream));
    if (carry)
        hipLaunchKernelGGL(kb_carry_start, grid_of(w, both_grids(w)), dim3(256), 0, w.stream, n, m, w.B, w.geo, w.Xb.p, w.Yb.p, w.X.p,
                           w.Y.p, w.shared->col_norm.p, w.shared->row_norm.p, w.bsc_prev.p, w.bsc.p, w.csc_prev.p, w.csc.p);
    for (DBuf<double> *p : {&w.Xh, &w.Xb, &w.DX, &w.Zb, &w.lastX, &w.Yb, &w.DY, &w.Yobj, &w.lastY, &w.SC, &w.partials}) zero_async(w, *p);
    if (!has_x && !carry) zero_async(w, w.X);
    if (!has_y && !carry) zero_async(w, w.Y);
    for (DBuf<int> *p : {&w.kx, &w.ky, &w.rflag}) zero_async(w, *p);
    if (detect) ws_ray_panels(w);
    if (!nvec) return;  // (a device-entry stream: its slots are filled from the caller's arrays, StreamRun::fill_first)
    const int longest = std::max(n, m);
    hipLaunchKernelGGL(kb_panel_in, dim3((longest + kPanelTile - 1) / kPanelTile, (w.Bp + kPanelTile - 1) / kPanelTile, nvec), dim3(256), 0,
                       w.stream, in, w.B, w.geo);
}

// Warm start: X / Y hold the starts in scaled units (the inverse of the results' map; kb_panel_in or kb_carry_start put them
// there): their projection, the seeding of every panel the first iteration reads, and the iteration-0 evaluation's sums.
void ws_start(BatchWS &w, const int *mask = kAllMembers) {
    launch_start_seed(w, mask);
    launch_start_col(w, mask);
    launch_start_row(w, mask);
}

// ---- the loop --------------------------------------------------------------------------------------------------------------
// one LP of the batch: the host side of its iteration, and how it ended
struct Member {
    RestartState rs;
    Residuals r;
    std::string status = "CONTINUE";
    int final_iter = 0;
    int verdict = 0;  // detection: 1 primal, 2 dual infeasible
    RayScalars ray;   // ... and the sums the verdict was reached with
};

struct BatchLoop {
    const HPRLP_parameters &prm;
    const Detection *det;  // null: detection off
    const int check_iter;
    clock_type::time_point solve_start;
    int iter = 0;
    std::vector<Member> mem;  // (every way out of the loop sets each member's status and final_iter)
    std::vector<double> sigma, gaps;
    std::vector<int> active, flags;
    bool dxdy_from_movement = false;
    // Per member, for a streamed batch (DESIGN.md "Streamed batches"): the loop iteration at which the member entered its slot --
    // every rule that reads the iteration number reads iter - base[k], the member's LOCAL one -- and whether the detection has
    // stored an iterate of it.  A plain solve: base 0 throughout, and the members active at an evaluation have all stored theirs
    // at the same one.
    std::vector<int> base;
    std::vector<char> ray_prev, ray_tested;
    // restart state (:534-556)
    BatchLoop(const BatchData &d, int Bp, const HPRLP_parameters &p, const Detection *dt)
        : prm(p), det(dt), check_iter(std::max(p.check_iter, 1)), mem(d.B), sigma(padded(d.sigma, Bp, 1.0)), active(Bp, 0), flags(Bp, 0),
          base(d.B, 0), ray_prev(d.B, 0), ray_tested(d.B, 0) {
        std::fill_n(active.begin(), d.B, 1);
        for (int k = 0; k < d.B; ++k) mem[k].rs.best_sigma = sigma[k];
    }
};

// The evaluation at a periodic event: residuals, stopping test and the detection's verdicts of the active members.  first: the
// iteration-0 evaluation (the bound term; no weighted norm, no ray test) -- of a plain solve the one at iteration 0; a streamed
// batch gives it to the members that have just entered, only[k] != 0 (null: every member), at whatever iteration the loop is.
void loop_evaluate(BatchWS &w, BatchLoop &L, bool first, const char *only = nullptr) {
    const BatchData &d = *w.data;
    const int B = w.B, iter = L.iter;
    if (!first) {
        weighted_norm(w, L.dxdy_from_movement, L.sigma, L.gaps);
        for (int k = 0; k < B; ++k) L.mem[k].rs.current_gap = L.gaps[k];
    }
    launch_dual_residual(w);
    launch_primal_residual(w);
    if (first) launch_bound_violation(w);
    bool ray_tested = false;
    if (L.det && !first) {  // a member's first periodic evaluation only stores its iterate
        for (int k = 0; k < B; ++k) {
            L.ray_tested[k] = L.active[k] && L.ray_prev[k];
            ray_tested = ray_tested || L.ray_tested[k];
        }
        ray_step(w, ray_tested);
        for (int k = 0; k < B; ++k)
            if (L.active[k]) L.ray_prev[k] = 1;
    }
    fetch(w);
    auto taken = [&](int k) { return L.active[k] && (!only || only[k]); };
    for (int k = 0; k < B; ++k) {
        // a frozen member's X_bar/Y_bar/Z_bar no longer change, so its residuals keep the
        // values of the check that froze it (the fused dot slots only cover active members)
        if (!taken(k)) continue;
        Residuals &r = L.mem[k].r;
        assemble_residuals(&r, {sc(w, B_CX, k), sc(w, B_YOBJ_Y, k), sc(w, B_XZ, k), sc(w, B_RD2, k), sc(w, B_RP2, k), sc(w, B_LU2, k)},
                           {d.b_scale[k], d.c_scale[k], d.norm_b_org[k], d.norm_c_org[k], d.objc[k]}, first);
        r.kkt = std::max(r.err_Rp, std::max(r.err_Rd, r.rel_gap));  // (solver.cpp nests the max() the other way, as the reference)
    }
    for (int k = 0; k < B; ++k)
        if (taken(k) && L.mem[k].r.kkt <= L.prm.stop_tol) {  // (<= here, strict in solver.cpp, as in the reference)
            L.mem[k].status = "OPTIMAL";
            L.mem[k].final_iter = iter - L.base[k];
            L.active[k] = 0;
        }
    if (ray_tested)
        for (int k = 0; k < B; ++k) {
            if (!L.active[k] || !L.ray_tested[k]) continue;  // (OPTIMAL at this evaluation takes precedence)
            const RayScalars s = ray_scalars(w, k);
            const int v = s.verdict(*L.det);
            if (!v) continue;
            Member &mb = L.mem[k];
            mb.status = v == 1 ? "PRIMAL_INFEASIBLE" : "DUAL_INFEASIBLE";
            mb.final_iter = iter - L.base[k];
            L.active[k] = 0;
            mb.verdict = v;
            mb.ray = s;
        }
    w.active.upload(L.active.data(), w.Bp);
}

// True when the loop is over: every member has a status, or the iteration / time limit gives the rest theirs.
bool loop_ended(BatchLoop &L, double elapsed) {
    bool all_done = true;
    for (const Member &mb : L.mem) all_done = all_done && (mb.status != "CONTINUE");
    if (all_done) return true;
    if (L.iter >= L.prm.max_iter || elapsed >= L.prm.time_limit) {  // (>= here, strict in solver.cpp, as in the reference)
        const char *fs = elapsed >= L.prm.time_limit ? "TIME_LIMIT" : "ITER_LIMIT";
        for (size_t k = 0; k < L.mem.size(); ++k)
            if (L.mem[k].status == "CONTINUE") {
                L.mem[k].status = fs;
                L.mem[k].final_iter = L.iter;
                L.active[k] = 0;
            }
        return true;
    }
    return false;
}

// The restart decision of every member and, where one restarts (the return value), the sigma update and the restart copy.
bool loop_restart(BatchWS &w, BatchLoop &L, bool periodic) {
    const int B = w.B;
    bool restarted = false;
    for (int k = 0; k < B; ++k) {  // check_restart :667-700
        RestartState &rs = L.mem[k].rs;
        if (periodic && L.active[k]) check_restart(rs, L.iter - L.base[k], L.check_iter, L.sigma[k], false);
        else rs.flag = 0;
        restarted = restarted || rs.flag > 0;
    }
    if (!restarted) return false;
    // update_sigma :702-745 (movement norms for every problem, formula for the flagged ones)
    launch_movement(w);
    fetch(w);
    L.dxdy_from_movement = true;
    for (int k = 0; k < B; ++k) {
        const Member &mb = L.mem[k];
        if (!L.active[k] || mb.rs.flag < 1) continue;
        L.sigma[k] = restart_sigma(std::sqrt(sc(w, B_MOVE_X2, k)), std::sqrt(sc(w, B_MOVE_Y2, k)), w.lambda_max, mb.rs, mb.r);
    }
    w.sigma.upload(L.sigma.data(), w.Bp);
    // do_restart :747-769
    for (int k = 0; k < w.Bp; ++k) L.flags[k] = (k < B && L.mem[k].rs.flag > 0) ? 1 : 0;
    w.rflag.upload(L.flags.data(), w.Bp);
    launch_restart_copy(w);
    for (int k = 0; k < B; ++k)
        if (L.active[k] && L.mem[k].rs.flag > 0) {
            L.mem[k].rs.inner = 0;
            L.mem[k].rs.save_gap = std::numeric_limits<double>::infinity();
        }
    return true;
}

// Iterations iter .. next-1; check variant where the reference's to_check holds (:1067-1068).  Unlike solver.cpp's
// next_event, the events are the periodic checks and the iteration limit only, not the log steps, as in the reference.
void loop_advance(BatchWS &w, BatchLoop &L, bool restarted) {
    const int iter = L.iter, check_iter = L.check_iter;
    int next = iter + 1;
    while (next % check_iter != 0 && next < L.prm.max_iter) ++next;
    int it = iter;
    while (it < next) {
        const bool first_after_restart = (it == iter) && restarted;
        int run = 0;  // normal iterations before the next check-variant one
        while (it + run < next && !(((it + run + 1) % check_iter) == 0 || ((it + run + 1) % log_step(it + run + 1)) == 0 ||
                                    (first_after_restart && run == 0)))
            ++run;
        run_normal(w, run);
        it += run;
        if (it < next) {
            launch_half_pair(w, true);
            L.dxdy_from_movement = false;
            ++it;
            if (first_after_restart) {
                weighted_norm(w, false, L.sigma, L.gaps);
                for (int k = 0; k < w.B; ++k)
                    if (L.mem[k].rs.flag > 0) L.mem[k].rs.last_gap = L.gaps[k];
            }
        }
    }
    for (int k = 0; k < w.B; ++k)
        if (L.active[k]) L.mem[k].rs.inner += next - iter;
    L.iter = next;
}

// ---- after the loop --------------------------------------------------------------------------------------------------------
// the first B members of a device panel, column-major on the host
std::vector<double> download_panel(const BatchWS &w, const DBuf<double> &P, int rows) {
    std::vector<double> panel(static_cast<size_t>(rows) * w.Bp), cm(static_cast<size_t>(rows) * w.B);
    P.download(panel.data(), panel.size());
    from_panel(panel, rows, w.B, w.geo, cm.data());
    return cm;
}

// one member's certificate from column `col` of the rays y, A^T y (primal) or d (dual): host arrays, scaled units, column-major
void member_certificate(const BatchWS &w, Certificate &c, const Member &mb, size_t col, const double *y, const double *z, const double *d,
                        double b_scale, double c_scale) {
    const size_t m = w.m, n = w.n;
    if (mb.verdict == 1) {
        c.y.assign(y + col * m, y + col * m + m);
        c.z.assign(z + col * n, z + col * n + n);
    } else {
        c.d.assign(d + col * n, d + col * n + n);
    }
    finish_certificate(&c, mb.verdict, mb.final_iter, mb.ray, w.rn.data(), w.cn.data(), b_scale, c_scale);
}

// the certificates of the members with a verdict: their YS / DS columns have not changed since (Solver::collect_certificate)
void collect_certificates(BatchWS &w, const BatchLoop &L, std::vector<Certificate> *certs) {
    const int m = w.m, n = w.n;
    certs->assign(w.B, Certificate());
    bool any_y = false, any_d = false;
    for (const Member &mb : L.mem) {
        any_y = any_y || mb.verdict == 1;
        any_d = any_d || mb.verdict == 2;
    }
    std::vector<double> hYS, hZS, hDS;
    if (any_y) {  // z = -A^T y: the plain product on the device, into the scratch panel
        w.Zray.alloc(static_cast<size_t>(n) * w.Bp);
        launch_ray_product(w);
        HIP_CHECK(hipStreamSynchronize(w.stream));
        hYS = download_panel(w, w.YS, m);
        hZS = download_panel(w, w.Zray, n);
    }
    if (any_d) hDS = download_panel(w, w.DS, n);
    for (int k = 0; k < w.B; ++k)
        if (L.mem[k].verdict)
            member_certificate(w, (*certs)[k], L.mem[k], k, hYS.data(), hZS.data(), hDS.data(), w.data->b_scale[k], w.data->c_scale[k]);
}

// the bars in the caller's units, column-major rows x B, to device addresses x, y, z (kb_panel_out)
void launch_panel_out(BatchWS &w, double *x, double *y, double *z) {
    const int m = w.m, n = w.n;
    const PanelOut po{{w.Xb.p, w.Yb.p, w.Zb.p}, {x, y, z}, {w.shared->col_norm.p, w.shared->row_norm.p, w.shared->col_norm.p},
                      {w.bsc.p, w.csc.p, w.csc.p}, {n, m, n}};
    hipLaunchKernelGGL(kb_panel_out, dim3((std::max(n, m) + kPanelTile - 1) / kPanelTile, (w.Bp + kPanelTile - 1) / kPanelTile, 3), dim3(256),
                       0, w.stream, po, w.B, w.geo);
}

// every member's evaluation, iteration and status (arrays of B; status 64 bytes per member; a null array is not wanted)
void member_results(const std::vector<Member> &mem, int B, double *primal_obj, double *residuals, double *gap, int *iter, char *status) {
    for (int k = 0; k < B; ++k) {
        if (primal_obj) primal_obj[k] = mem[k].r.primal_obj;
        if (residuals) residuals[k] = mem[k].r.kkt;
        if (gap) gap[k] = mem[k].r.rel_gap;
        if (iter) iter[k] = mem[k].final_iter;
        if (status) std::strncpy(status + 64 * k, mem[k].status.c_str(), 63);
    }
}

// collect_results :887-935: the bars in the caller's units (kb_panel_out into the staging block, one download), and every
// member's evaluation, iteration and status
HPRLP_batched_results collect_results(BatchWS &w, const BatchLoop &L, std::vector<Certificate> *certs) {
    const int m = w.m, n = w.n, B = w.B;
    const size_t nB = static_cast<size_t>(n) * B, mB = static_cast<size_t>(m) * B;
    HPRLP_batched_results out = alloc_batched_results(m, n, B);
    try {
        double *sd = w.stage_d.p;
        launch_panel_out(w, sd, sd + nB, sd + nB + mB);
        HIP_CHECK(hipMemcpyAsync(w.stage_h.p, sd, (2 * nB + mB) * sizeof(double), hipMemcpyDeviceToHost, w.stream));
        HIP_CHECK(hipStreamSynchronize(w.stream));
        std::memcpy(out.x, w.stage_h.p, nB * sizeof(double));
        std::memcpy(out.y, w.stage_h.p + nB, mB * sizeof(double));
        std::memcpy(out.z, w.stage_h.p + nB + mB, nB * sizeof(double));
        if (certs) collect_certificates(w, L, certs);
    } catch (...) {
        free_batched_results(&out);
        throw;
    }
    member_results(L.mem, B, out.primal_obj, out.residuals, out.gap, out.iter, out.status);
    return out;
}

// ---- a call's way into the staging block (all three entries) ------------------------------------------------------------------------
// The block: the header, sigma | b_scale | c_scale (Bp doubles each) | active (Bp ints in the room of Bp doubles), then the
// column-major regions C, L, U, AL, AU and, where the call has them, X0 and Y0, of `members` members (a stream: the whole queue).
struct Regions {
    int nvec = 0, iX = -1, iY = -1;  // the starts' places among the regions (-1: none)
    int rows[kPanelVectors];
    size_t start[kPanelVectors], count[kPanelVectors], end;  // in doubles from the block's start; end: its length
    Regions(int Bp, int n, int m, int members, bool has_x, bool has_y) : end(4 * static_cast<size_t>(Bp)) {
        auto region = [&](int r) {
            rows[nvec] = r;
            start[nvec] = end;
            end += count[nvec] = static_cast<size_t>(r) * members;
            return nvec++;
        };
        for (int r : {n, n, n, m, m}) region(r);
        if (has_x) iX = region(n);
        if (has_y) iY = region(m);
    }
};

// Host entries: the staging blocks grow, each by its own size (the pinned one also serves a streamed call's download); into the pinned
// one go the header of the Bp members the loop starts with, `first` (stage_header: all that a device-entry stream uploads), and d's
// scaled vectors and the caller's starts, in scaled units.
void stage_header(BatchWS &w, const BatchLoop &L, const BatchData &first, size_t pinned, size_t device) {
    if (w.stage_h.n < pinned) w.stage_h.alloc(pinned, /*zero=*/false);
    if (w.stage_d.n < device) w.stage_d.alloc(device);
    const size_t Bp = L.sigma.size();
    double *sh = w.stage_h.p;
    const std::vector<double> bs = padded(first.b_scale, Bp, 1.0), cs = padded(first.c_scale, Bp, 1.0);
    std::copy(L.sigma.begin(), L.sigma.end(), sh);
    std::copy(bs.begin(), bs.end(), sh + Bp);
    std::copy(cs.begin(), cs.end(), sh + 2 * Bp);
    std::memcpy(sh + 3 * Bp, L.active.data(), sizeof(int) * Bp);
}
void stage_host(BatchWS &w, const BatchLoop &L, const BatchData &first, const Regions &r, const BatchData &d, const double *X0,
                const double *Y0, size_t pinned, size_t device) {
    stage_header(w, L, first, pinned, device);
    double *sh = w.stage_h.p;
    const double *src[kPanelVectors] = {d.C.data(), d.L.data(), d.U.data(), d.AL.data(), d.AU.data(), X0 ? X0 : Y0, Y0};
    for (int v = 0; v < r.nvec; ++v) std::memcpy(sh + r.start[v], src[v], r.count[v] * sizeof(double));
    if (X0) start_to_scaled(sh + r.start[r.iX], w.n, d.B, w.cn.data(), d.b_scale);
    if (Y0) start_to_scaled(sh + r.start[r.iY], w.m, d.B, w.rn.data(), d.c_scale);
}

// the regions as kb_panel_in's argument: from the device block into the workspace's panels, once both are at their addresses
PanelIn bind_panels(const BatchWS &w, const Regions &r) {
    PanelIn in{};
    double *const panels[5] = {w.C.p, w.L.p, w.U.p, w.AL.p, w.AU.p};
    for (int v = 0; v < r.nvec; ++v) {
        in.src[v] = w.stage_d.p + r.start[v];
        in.rows[v] = r.rows[v];
        in.dst[v] = v < 5 ? panels[v] : (v == r.iX ? w.X.p : w.Y.p);
    }
    return in;
}

// ---- the device entry's own steps (DESIGN.md "Device-resident batches") ---------------------------------------------------------
static_assert(DS_COUNT == kMemberScalars - 1, "member_scalars() lists the device entry's scalars in DataScalar's order, then objc");
inline int *data_flags(const BatchWS &w, int B) { return reinterpret_cast<int *>(w.data_scal.p + static_cast<size_t>(DS_COUNT) * B); }
inline const int *data_flags_host(const BatchWS &w, int B) {
    return reinterpret_cast<const int *>(w.data_scal_h.p + static_cast<size_t>(DS_COUNT) * B);
}

// the segment partials and the scalars (with their pinned twin) of B members
void data_buffers(BatchWS &w, int B, int nseg) {
    const size_t part_count = static_cast<size_t>(4) * B * nseg, scal_count = static_cast<size_t>(DS_COUNT) * B + DF_COUNT;
    if (w.data_part.n < part_count) w.data_part.alloc(part_count);
    if (w.data_scal.n != scal_count) {  // (the flag words sit behind the scalars of exactly B members)
        w.data_scal.alloc(scal_count);
        w.data_scal_h.alloc(scal_count);
    }
}
// the scalars of B members and the flag words to the host in one copy: the BatchData a loop needs (it reads none of the vectors)
BatchData fetch_member_scalars(BatchWS &w, int B, const double *obj_constants, double model_obj_constant) {
    HIP_CHECK(hipMemcpyAsync(w.data_scal_h.p, w.data_scal.p, static_cast<size_t>(DS_COUNT) * B * sizeof(double) + DF_COUNT * sizeof(int),
                             hipMemcpyDeviceToHost, w.stream));
    HIP_CHECK(hipStreamSynchronize(w.stream));
    BatchData d;
    d.m = w.m; d.n = w.n; d.B = B;
    const double *h = w.data_scal_h.p;
    const auto dst = member_scalars(d);
    for (int i = 0; i < DS_COUNT; ++i) dst[i]->assign(h + static_cast<size_t>(i) * B, h + static_cast<size_t>(i + 1) * B);
    d.objc.assign(B, model_obj_constant);
    if (obj_constants) d.objc.assign(obj_constants, obj_constants + B);
    return d;
}

// prepare_batch on the device, for B members whose vectors lie in device memory (ordered on `stream`): the per-member scalars on the
// host -- the BatchData a loop needs (it reads none of the vectors) -- and DF_START for a non-finite start anywhere.  The two norm
// passes run in slices of what one grid dimension takes.
// r given (a batch): the vectors in scaled units into the regions r of the staging block, and its header for Bp padded members.
// r null (a queue): nothing else; sigma, b_scale and c_scale stay in w.data_scal for the refills (kb_slot_clear, kb_slot_scale).
BatchData device_prep(BatchWS &w, int B, int Bp, const Regions *r, const double *C, const double *AL, const double *AU, const double *l,
                      const double *u, const double *X0, const double *Y0, const double *obj_constants, double model_obj_constant,
                      bool use_bc, hipStream_t stream, hipEvent_t ready) {
    constexpr int kGridSlice = 65535;
    const int m = w.m, n = w.n, nseg = norm_segments(std::max(n, m));
    if (r && w.stage_d.n < r->end) w.stage_d.alloc(r->end);
    data_buffers(w, B, nseg);
    HIP_CHECK(hipEventRecord(ready, stream));
    HIP_CHECK(hipStreamWaitEvent(w.stream, ready, 0));
    int *flags = data_flags(w, B);
    HIP_CHECK(hipMemsetAsync(flags, 0, DF_COUNT * sizeof(int), w.stream));
    const double *cn = w.shared->col_norm.p, *rn = w.shared->row_norm.p;
    double *sd = r ? w.stage_d.p : nullptr, *reg[kPanelVectors] = {};  // the header and the regions (a queue: none)
    for (int v = 0; r && v < r->nvec; ++v) reg[v] = sd + r->start[v];
    double *rX = r && X0 ? reg[r->iX] : nullptr, *rY = r && Y0 ? reg[r->iY] : nullptr;
    const DataIn in{C, l, u, AL, AU, reg[0], reg[1], reg[2], reg[3], reg[4], cn, rn, w.data_part.p, n, m, nseg};
    // the second pass reads what the first left: a batch's regions, or again the caller's arrays
    const DataBc bc{r ? reg[0] : C, reg[1], reg[2], r ? reg[3] : AL, r ? reg[4] : AU, reg[0], reg[1], reg[2], reg[3], reg[4],
                    X0, Y0, rX, rY, cn, rn, w.data_scal.p, w.data_part.p, flags, n, m, nseg};
    const auto pass = [&](auto kernel, const auto &args) {
        for (int k0 = 0; k0 < B; k0 += kGridSlice)
            hipLaunchKernelGGL(kernel, dim3(nseg, std::min(kGridSlice, B - k0), 2), dim3(kNormLanes), 0, w.stream, args, B, k0);
    };
    pass(r ? kb_data_in<true> : kb_data_in<false>, in);
    hipLaunchKernelGGL(kb_data_scales, dim3((B + 255) / 256), dim3(256), 0, w.stream, static_cast<const double *>(w.data_part.p), B, n, m, nseg,
                       use_bc ? 1 : 0, w.data_scal.p);
    pass(r ? kb_data_bc<true> : kb_data_bc<false>, bc);
    const int members = r ? Bp : B;
    hipLaunchKernelGGL(kb_data_header, dim3((members + 255) / 256), dim3(256), 0, w.stream, static_cast<const double *>(w.data_part.p), B,
                       members, n, m, nseg, w.data_scal.p, sd);
    HIP_CHECK(hipGetLastError());
    return fetch_member_scalars(w, B, obj_constants, model_obj_constant);
}

// the device entry's results, straight into the caller's buffers; the flag word that comes back: x or y holds a non-finite entry
bool device_results(BatchWS &w, const BatchLoop &L, DeviceBatch &dev, std::vector<Certificate> *certs) {
    const int B = w.B;
    const size_t nB = static_cast<size_t>(w.n) * B, mB = static_cast<size_t>(w.m) * B;
    launch_panel_out(w, dev.x, dev.y, dev.z);
    hipLaunchKernelGGL(kb_flag_nonfinite, dim3(static_cast<unsigned>(std::min<size_t>((nB + mB + 255) / 256, 1024))), dim3(256), 0, w.stream,
                       static_cast<const double *>(dev.x), nB, static_cast<const double *>(dev.y), mB, data_flags(w, B) + DF_RESULT);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(const_cast<int *>(data_flags_host(w, B)) + DF_RESULT, data_flags(w, B) + DF_RESULT, sizeof(int),
                             hipMemcpyDeviceToHost, w.stream));
    HIP_CHECK(hipStreamSynchronize(w.stream));
    if (certs) collect_certificates(w, L, certs);
    member_results(L.mem, B, dev.primal_obj, dev.residuals, dev.gap, dev.iter, dev.status);
    return data_flags_host(w, B)[DF_RESULT] != 0;
}

// ---- a streamed call's state: the slots' side of the loop, which problem sits in which slot and the record of it, the members that
// have ended, the queue, the counters, and the refill pass's argument blocks and tables -------------------------------------------
struct StreamRun {
    BatchWS &w;
    const BatchData &q;  // the whole queue in scaled units (a device-entry call: its scalars alone)
    DeviceBatch *const dev;  // a device-entry call (DESIGN.md "Device-resident streams"): the caller's buffers; null: the host entry
    const int *const parent;  // a parents call (DESIGN.md "Streamed batches", "Parents"): count entries; null: the plain queue
    const int count, W, max_iter;  // max_iter: each member's own limit (the loop's own is unlimited)
    const bool warm, detect;
    BatchData sd;  // the scalars of the problems in the slots: what the loop reads as "the batch" (it reads none of the vectors)
    HPRLP_parameters loop_prm;  // the call's, but for max_iter: unlimited
    BatchLoop L;
    const Regions regions;  // of the whole queue; behind them, at regions.end, sigma | b_scale | c_scale of every problem
                            // (a device-entry call stages no queue: the header alone, and the scalars are in w.data_scal)
    // res_count: x, y, z and, with detection, the rays y, A^T y, d of every problem (a device-entry call: the rays alone, x, y, z go
    // to the caller's buffers); tab_count: out pairs | in pairs | the start mask
    // a parents call: behind the scalars the caller's X0 | Y0 as they are (the host entry; kb_slot_start scales a root's columns),
    // and behind the start mask the source of each in pair
    const size_t nN, mN, stage_count, res_count, tab_count;
    SlotClear sclr{};
    SlotIn sin{};
    SlotScale sscale{};  // a device-entry call's way in, in sin's place
    SlotOut sout{};
    SlotStart sstart{};  // a parents call's way into X and Y, in the X / Y regions' place
    std::vector<Member> done;
    std::vector<int> occ, freed, ps, pp;   // the problem in each slot (-1: empty); a pass's freed slots and its (slot, problem) pairs
    std::vector<char> is_new;
    std::vector<int> r_slot, r_in, r_out;  // the record: the handle takes it when the call has succeeded
    StreamQueue queue;
    StreamParentQueue pqueue;  // ... of a parents call
    std::vector<int> avail;    // a parents call's free slots of a pass: the freed ones and those that stood empty, ascending
    bool pass_starts = false;  // a parents call's pass lists a member with a start: the masked start kernels run
    long entered_roots = 0, entered_cold = 0, entered_children = 0, idle_slot_events = 0;  // hprlp_batched_solver_stream_parents_info
    long evals = 0, refill_events = 0, refills = 0, passes = 0;
    const long bumps0;
    bool ray_y = false, any_verdict = false;      // of a pass's freed members: which rays their harvest copies

    StreamRun(BatchWS &w_, const BatchData &q_, int W_, int Bp, const HPRLP_parameters &prm, const Detection *det, bool has_x, bool has_y,
              DeviceBatch *dev_, const int *parent_ = nullptr)
        : w(w_), q(q_), dev(dev_), parent(parent_), count(q_.B), W(W_), max_iter(prm.max_iter), warm(has_x || has_y), detect(det != nullptr),
          sd(first_members(q_, W_)), loop_prm(prm), L(sd, Bp, loop_prm, det),
          regions(Bp, q_.n, q_.m, dev_ ? 0 : q_.B, has_x && !parent_, has_y && !parent_),
          nN(static_cast<size_t>(q_.n) * count), mN(static_cast<size_t>(q_.m) * count),
          stage_count(regions.end + (dev_ ? 0 : 3 * static_cast<size_t>(count)) + (parent_ && !dev_ && warm ? nN + mN : 0)),
          res_count(dev_ ? (detect ? 2 * nN + mN : 0) : (2 * nN + mN) * (detect ? 2 : 1)),
          tab_count(4 * static_cast<size_t>(W_) + Bp + (parent_ ? W_ : 0)),
          done(count), occ(W), freed(W), ps(W), pp(W), is_new(W, 0), r_slot(count, -1), r_in(count, -1), r_out(count, -1),
          bumps0(w_.bumps) {
        loop_prm.max_iter = std::numeric_limits<int>::max();
        if (parent) {  // every slot empty and inactive: the initial fill is a pass (first_pass)
            std::fill(occ.begin(), occ.end(), -1);
            std::fill(L.active.begin(), L.active.end(), 0);
            pqueue = StreamParentQueue(count, parent);
            avail.resize(W);
            return;
        }
        for (int k = 0; k < W; ++k) occ[k] = r_slot[k] = k;  // (where the initial fill puts the first W problems)
        std::fill_n(r_in.begin(), W, 0);
        queue = StreamQueue{count, W};
    }

    // the whole queue into the pinned block, behind the header of the first W members; behind it the scalars a refill reads.  A
    // device-entry call: the header alone.
    void stage(const double *X0, const double *Y0) {
        if (dev) stage_header(w, L, sd, stage_count, stage_count);
        else stage_host(w, L, sd, regions, q, parent ? nullptr : X0, parent ? nullptr : Y0, std::max(stage_count, res_count), stage_count);
        if (w.res_d.n < res_count) w.res_d.alloc(res_count);
        if (dev) return;
        double *qh = w.stage_h.p + regions.end;
        std::copy(q.sigma.begin(), q.sigma.end(), qh);
        std::copy(q.b_scale.begin(), q.b_scale.end(), qh + count);
        std::copy(q.c_scale.begin(), q.c_scale.end(), qh + 2 * static_cast<size_t>(count));
        if (parent && warm) {  // in the caller's units: the roots' columns are scaled on their way in, like a child's start
            std::memcpy(qh + 3 * static_cast<size_t>(count), X0, nN * sizeof(double));
            std::memcpy(qh + 3 * static_cast<size_t>(count) + nN, Y0, mN * sizeof(double));
        }
    }

    // Behind the initial fill, when every panel is at its address: the harvest's scratch panel, the tables (they only grow), and the
    // refill pass's argument blocks.  in: the initial fill's way in, which a refill shares.
    void bind(const PanelIn &in) {
        const int n = w.n, m = w.m;
        if (detect && w.Zray.n != static_cast<size_t>(n) * w.Bp) w.Zray.alloc(static_cast<size_t>(n) * w.Bp);
        if (w.tab_h.n < tab_count) {
            w.tab_h.alloc(tab_count);
            w.tab_d.alloc(tab_count);
        }
        std::copy(in.src, in.src + kPanelVectors, sin.src);
        std::copy(in.dst, in.dst + kPanelVectors, sin.dst);
        std::copy(in.rows, in.rows + kPanelVectors, sin.rows);
        const double *qd = w.stage_d.p + regions.end;
        sclr.n = n; sclr.m = m;
        for (double *pn : {w.Xh.p, w.Xb.p, w.DX.p, w.Zb.p, w.lastX.p}) sclr.pn[sclr.npn++] = pn;
        for (double *pm : {w.Yb.p, w.DY.p, w.Yobj.p, w.lastY.p}) sclr.pm[sclr.npm++] = pm;
        if (regions.iX < 0 && !parent) sclr.pn[sclr.npn++] = w.X.p;  // (a parents call: kb_slot_start writes every listed column)
        if (regions.iY < 0 && !parent) sclr.pm[sclr.npm++] = w.Y.p;
        if (detect) {
            sclr.pn[sclr.npn++] = w.prevX.p; sclr.pn[sclr.npn++] = w.DS.p;
            sclr.pm[sclr.npm++] = w.prevY.p; sclr.pm[sclr.npm++] = w.YS.p;
        }
        sclr.SC = w.SC.p; sclr.ctl = w.ctl; sclr.bsc = w.bsc.p; sclr.csc = w.csc.p;
        sclr.q_sigma = qd; sclr.q_bs = qd + count; sclr.q_cs = qd + 2 * static_cast<size_t>(count);
        if (dev) {  // (where device_prep left them)
            const double *sc = w.data_scal.p;
            sclr.q_sigma = sc + static_cast<size_t>(DS_SIGMA) * count;
            sclr.q_bs = sc + static_cast<size_t>(DS_B_SCALE) * count;
            sclr.q_cs = sc + static_cast<size_t>(DS_C_SCALE) * count;
        }
        double *rd = w.res_d.p;
        double *const rx = dev ? dev->x : rd, *const ry = dev ? dev->y : rd + nN, *const rz = dev ? dev->z : rd + nN + mN;
        if (!dev) rd += 2 * nN + mN;  // the rays y, A^T y, d: behind the solutions, or the whole of a device-entry call's block
        const double *cnd = w.shared->col_norm.p, *rnd = w.shared->row_norm.p;
        // (the ray d before the rays y, A^T y: a pass without a primal verdict stops short of them -- nobody has written Zray then)
        sout = SlotOut{{w.Xb.p, w.Yb.p, w.Zb.p, w.DS.p, w.YS.p, w.Zray.p},
                       {rx, ry, rz, rd + nN + mN, rd, rd + mN},
                       {cnd, rnd, cnd, nullptr, nullptr, nullptr},
                       {w.bsc.p, w.csc.p, w.csc.p, nullptr, nullptr, nullptr},
                       {n, m, n, n, m, n},
                       {SLOT_OUT_POINT, SLOT_OUT_POINT, SLOT_OUT_REDUCED_COST, SLOT_OUT_RAW, SLOT_OUT_RAW, SLOT_OUT_RAW}};
    }
    const SlotPair *out_pairs() const { return reinterpret_cast<const SlotPair *>(w.tab_d.p); }
    const SlotPair *in_pairs() const { return reinterpret_cast<const SlotPair *>(w.tab_d.p + 2 * static_cast<size_t>(W)); }
    const int *new_mask() const { return w.tab_d.p + 4 * static_cast<size_t>(W); }
    const int *sources() const { return new_mask() + w.Bp; }

    // A parents call's way into X and Y (after bind): a child from its parent's column of the results, a root from its own column of
    // the caller's X0 / Y0 -- the device entry's arrays, or the host entry's staged copy.
    void bind_starts(const double *X0, const double *Y0) {
        const double *own = w.stage_d.p + regions.end + 3 * static_cast<size_t>(count);
        sstart = SlotStart{{sout.dst[0], sout.dst[1]}, {nullptr, nullptr}, {w.X.p, w.Y.p},
                           {w.shared->col_norm.p, w.shared->row_norm.p}, {w.n, w.m}, sclr.q_bs, sclr.q_cs, sources()};
        if (warm) {
            sstart.own[0] = dev ? X0 : own;
            sstart.own[1] = dev ? Y0 : own + nN;
        }
    }
    int source_of(int pr) const { return parent[pr] >= 0 ? parent[pr] : (warm ? kSourceOwn - pr : kSourceNone); }
    // ... and its initial fill.  Before the loop: the five data panels 0.0 throughout, as kb_panel_in leaves padding members (a
    // slot nobody has entered yet is one).  first_pass, at the loop's start: a pass of event 0 with every slot free and nothing to
    // harvest, in which only roots are ready; it is the iteration-0 evaluation of the members it puts in.
    void clear_data_panels() {
        for (int v = 0; v < regions.nvec; ++v)
            HIP_CHECK(hipMemsetAsync(sin.dst[v], 0, static_cast<size_t>(sin.rows[v]) * w.Bp * sizeof(double), w.stream));
    }
    void first_pass() {
        for (int k = 0; k < W; ++k) avail[k] = k;
        const int nin = stream_assign_parents(pqueue, avail.data(), W, ps.data(), pp.data());
        if (!nin) throw std::logic_error("batched stream: no root among the queued problems");  // (parent[0] is -1: checked at entry)
        harvest(0, nin);
        refill(nin);
        refills = passes = 0;  // (the counts are of the entries after the initial fill, as the plain queue's)
    }

    // A device-entry call's way into the slots (after bind): the caller's arrays in the regions' order, each with its norm and its
    // operations (kb_slot_scale).
    void bind_caller(const double *C, const double *AL, const double *AU, const double *l, const double *u, const double *X0,
                     const double *Y0) {
        const double *cnd = w.shared->col_norm.p, *rnd = w.shared->row_norm.p;
        const double *src[kPanelVectors] = {C, l, u, AL, AU, X0 ? X0 : Y0, Y0};
        const double *norm[5] = {cnd, cnd, cnd, rnd, rnd};
        const int op[5] = {SF_BY_C, SF_TIMES_NORM | SF_LOWER, SF_TIMES_NORM | SF_UPPER, SF_LOWER, SF_UPPER};
        for (int v = 0; v < regions.nvec; ++v) {
            sscale.src[v] = src[v];
            sscale.dst[v] = sin.dst[v];
            sscale.rows[v] = regions.rows[v];
            sscale.norm[v] = v < 5 ? norm[v] : (v == regions.iX ? cnd : rnd);
            sscale.op[v] = v < 5 ? op[v] : (v == regions.iX ? SF_TIMES_NORM : SF_TIMES_NORM | SF_BY_C);
        }
        sscale.q_bs = sclr.q_bs;
        sscale.q_cs = sclr.q_cs;
    }
    // ... and its initial fill: problems 0 .. W-1 into slots 0 .. W-1 by the refill's own kernel; padding members and dead columns 0.0,
    // as kb_panel_in leaves them
    void fill_first() {
        for (int v = 0; v < regions.nvec; ++v)
            HIP_CHECK(hipMemsetAsync(sscale.dst[v], 0, static_cast<size_t>(sscale.rows[v]) * w.Bp * sizeof(double), w.stream));
        int *th = w.tab_h.p;
        std::fill(th, th + tab_count, 0);
        for (int k = 0; k < W; ++k) th[2 * (W + k)] = th[2 * (W + k) + 1] = k;
        HIP_CHECK(hipMemcpyAsync(w.tab_d.p, th, tab_count * sizeof(int), hipMemcpyHostToDevice, w.stream));
        launch_slot(w, kb_slot_scale, sscale, in_pairs(), W, regions.nvec);
    }

    // the limit rule (time first, as loop_ended; then the member's own max_iter), then the slots whose member has a status: freed[0 .. return)
    int expire_and_collect(bool time_up, bool &active_stale) {
        int nout = 0;
        ray_y = any_verdict = false;
        for (int k = 0; k < W; ++k) {
            if (occ[k] < 0) continue;
            Member &mb = L.mem[k];
            const int local = L.iter - L.base[k];
            if (mb.status == "CONTINUE" && (time_up || local >= max_iter)) {
                mb.status = time_up ? "TIME_LIMIT" : "ITER_LIMIT";
                mb.final_iter = local;
                L.active[k] = 0;
                active_stale = true;
            }
            if (mb.status == "CONTINUE") continue;
            freed[nout++] = k;
            ray_y = ray_y || mb.verdict == 1;
            any_verdict = any_verdict || mb.verdict != 0;
        }
        return nout;
    }

    // the pass's table up (freed slots; the refill's pairs and start mask), then the freed members' x, y, z and rays into the result block
    void harvest(int nout, int nin) {
        const int event = L.iter / L.check_iter;
        int *th = w.tab_h.p;
        for (int i = 0; i < nout; ++i) {  // (and the host's side of the hand-over: the member is kept, its slot is empty)
            const int k = freed[i], pr = occ[k];
            th[2 * i] = k;
            th[2 * i + 1] = pr;
            done[pr] = L.mem[k];
            r_out[pr] = event;
            occ[k] = -1;
        }
        std::fill(th + 4 * static_cast<size_t>(W), th + tab_count, 0);
        pass_starts = false;
        for (int i = 0; i < nin; ++i) {
            th[2 * (W + i)] = ps[i];
            th[2 * (W + i) + 1] = pp[i];
            const int source = parent ? source_of(pp[i]) : 0;
            if (parent) th[4 * static_cast<size_t>(W) + w.Bp + i] = source;
            if (source == kSourceNone) continue;  // a cold root: the start kernels' mask leaves it out
            th[4 * static_cast<size_t>(W) + ps[i]] = 1;
            pass_starts = true;
        }
        HIP_CHECK(hipMemcpyAsync(w.tab_d.p, th, tab_count * sizeof(int), hipMemcpyHostToDevice, w.stream));
        if (!nout) return;  // (a parents call's initial fill)
        if (ray_y) {  // z = -A^T y of a primal verdict: the plain product of every column, as collect_certificates has it
            launch_ray_product(w);
            HIP_CHECK(hipGetLastError());
        }
        launch_slot(w, kb_slot_out, sout, out_pairs(), nout, ray_y ? kSlotOutVectors : (any_verdict ? kSlotOutDual : kSlotOutPlain));
    }

    // the queued problems into their slots (cleared, filled, started), the slots' host side re-seated, the new members' iteration-0 evaluation
    void refill(int nin) {
        const int event = L.iter / L.check_iter;
        launch_slot(w, kb_slot_clear, sclr, in_pairs(), nin, sclr.npn + sclr.npm + 1);
        if (dev) launch_slot(w, kb_slot_scale, sscale, in_pairs(), nin, regions.nvec);
        else launch_slot(w, kb_slot_in, sin, in_pairs(), nin, regions.nvec);
        if (parent) launch_slot(w, kb_slot_start, sstart, in_pairs(), nin, 2);
        if (parent ? pass_starts : warm) {
            ws_start(w, new_mask());
            HIP_CHECK(hipGetLastError());
        }
        const auto slot = member_scalars(sd);
        const auto queued = member_scalars(q);
        std::fill(is_new.begin(), is_new.end(), 0);
        for (int i = 0; i < nin; ++i) {
            const int k = ps[i], pr = pp[i];
            occ[k] = pr;
            r_slot[pr] = k;
            r_in[pr] = event;
            L.mem[k] = Member();
            L.mem[k].rs.best_sigma = q.sigma[pr];
            L.sigma[k] = q.sigma[pr];
            L.active[k] = 1;
            L.base[k] = L.iter;
            L.ray_prev[k] = 0;
            L.ray_tested[k] = 0;
            is_new[k] = 1;
            for (int s = 0; s < kMemberScalars; ++s) (*slot[s])[k] = (*queued[s])[pr];
            if (parent) {
                const int source = source_of(pr);
                ++(source >= 0 ? entered_children : entered_roots);
                if (source == kSourceNone) ++entered_cold;
            }
        }
        refills += nin;
        ++passes;
        loop_evaluate(w, L, /*first=*/true, is_new.data());
    }

    // A parents call's side of a pass.  The members that end release their children first -- a child is ready in the very pass that
    // harvests its parent: kb_slot_out writes the column before kb_slot_start reads it, on one stream -- or, where the parent's
    // final evaluation is not finite, drop them for good.  Then the free slots (the freed ones and those that stood empty),
    // ascending, take the ready problems, ascending.  Nothing enters once the time is up.
    int assign_ready(int nout, bool time_up) {
        for (int i = 0; i < nout; ++i) {
            const Residuals &r = L.mem[freed[i]].r;
            pqueue.release(occ[freed[i]], std::isfinite(r.kkt) && std::isfinite(r.primal_obj) && std::isfinite(r.rel_gap));
        }
        if (time_up) return 0;
        int nfree = 0;
        for (int k = 0, i = 0; k < W; ++k) {
            const bool ends = i < nout && freed[i] == k;
            if (ends) ++i;
            if (ends || occ[k] < 0) avail[nfree++] = k;
        }
        return stream_assign_parents(pqueue, avail.data(), nfree, ps.data(), pp.data());
    }
    int occupied_slots() const { return static_cast<int>(std::count_if(occ.begin(), occ.end(), [](int pr) { return pr >= 0; })); }
    // the problems that never entered a slot: the time limit's, and, in a parents call, the descendants of an unusable point
    void mark_never_entered() {
        for (int pr = 0; pr < count; ++pr)
            if (r_slot[pr] < 0) done[pr].status = parent && pqueue.dropped[pr] ? "ERROR" : "TIME_LIMIT";  // (iteration 0, no residuals)
    }

    // one pass of an event; false when it handed no slot on (nobody ended, the queue is empty, the time is up): the event is over
    bool pass(bool time_up, bool &active_stale) {
        const int nout = expire_and_collect(time_up, active_stale);
        if (!nout) return false;
        const int nin = parent ? assign_ready(nout, time_up) : (time_up ? 0 : stream_assign(queue, freed.data(), nout, ps.data(), pp.data()));
        harvest(nout, nin);
        if (!nin) {
            HIP_CHECK(hipStreamSynchronize(w.stream));  // (the pinned table is free again)
            return false;
        }
        refill(nin);
        active_stale = false;
        return true;
    }
    bool occupied() const { return std::any_of(occ.begin(), occ.end(), [](int pr) { return pr >= 0; }); }

    // all `count` problems: one download of the result block, the members' evaluations, the certificates from the rays beside the solutions
    HPRLP_batched_results results(std::vector<Certificate> *certs) {
        mark_never_entered();
        HPRLP_batched_results res = alloc_batched_results(w.m, w.n, count);
        try {
            HIP_CHECK(hipMemcpyAsync(w.stage_h.p, w.res_d.p, res_count * sizeof(double), hipMemcpyDeviceToHost, w.stream));
            HIP_CHECK(hipStreamSynchronize(w.stream));
            const double *rh = w.stage_h.p;
            std::memcpy(res.x, rh, nN * sizeof(double));
            std::memcpy(res.y, rh + nN, mN * sizeof(double));
            std::memcpy(res.z, rh + nN + mN, nN * sizeof(double));
            if (certs) {
                certs->assign(count, Certificate());
                const double *cy = rh + 2 * nN + mN, *cz = cy + mN, *cd = cz + nN;
                for (int pr = 0; pr < count && detect; ++pr)
                    if (done[pr].verdict) member_certificate(w, (*certs)[pr], done[pr], pr, cy, cz, cd, q.b_scale[pr], q.c_scale[pr]);
            }
        } catch (...) {
            free_batched_results(&res);
            throw;
        }
        member_results(done, count, res.primal_obj, res.residuals, res.gap, res.iter, res.status);
        return res;
    }

    // A device-entry call: x, y, z are in the caller's buffers already; the members' evaluations go to its host arrays, and of the
    // ray block only the columns of the problems with a verdict come to the host.  Returns the bytes of those.
    size_t results_device(std::vector<Certificate> *certs) {
        mark_never_entered();
        HIP_CHECK(hipStreamSynchronize(w.stream));
        const size_t m = w.m, n = w.n;
        size_t ray_doubles = 0;
        if (certs) {
            certs->assign(count, Certificate());
            std::vector<double> cy(m), cz(n), cd(n);
            const double *ry = w.res_d.p, *rz = ry + mN, *rd = rz + nN;
            for (int pr = 0; pr < count && detect; ++pr) {
                if (!done[pr].verdict) continue;
                if (done[pr].verdict == 1) {
                    HIP_CHECK(hipMemcpy(cy.data(), ry + pr * m, m * sizeof(double), hipMemcpyDeviceToHost));
                    HIP_CHECK(hipMemcpy(cz.data(), rz + pr * n, n * sizeof(double), hipMemcpyDeviceToHost));
                    ray_doubles += m + n;
                } else {
                    HIP_CHECK(hipMemcpy(cd.data(), rd + pr * n, n * sizeof(double), hipMemcpyDeviceToHost));
                    ray_doubles += n;
                }
                member_certificate(w, (*certs)[pr], done[pr], 0, cy.data(), cz.data(), cd.data(), q.b_scale[pr], q.c_scale[pr]);
            }
        }
        member_results(done, count, dev->primal_obj, dev->residuals, dev->gap, dev->iter, dev->status);
        return ray_doubles * sizeof(double);
    }
};

}  // namespace

// A pointer of the caller's passes only as device memory of `device` that the runtime knows, with room for `count` doubles where
// the runtime reports the allocation's range.  Nothing is launched before every pointer of a call has passed.
// (declared in common.h: the resident solver's device entries check their pointers with it too)
void check_device_pointer(const void *p, size_t count, int device, const char *name, const char *entry, DeviceRange *range) {
    if (range) *range = DeviceRange();
    const std::string who = std::string(entry) + ": " + name;
    if (!p) throw std::runtime_error(who + " is null");
    if (reinterpret_cast<uintptr_t>(p) % sizeof(double)) throw std::runtime_error(who + " is not aligned to 8 bytes");
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        throw std::runtime_error(who + " is not a pointer the HIP runtime knows (a host address?)");
    }
    if (attr.type != hipMemoryTypeDevice) throw std::runtime_error(who + " is not device memory");
    if (attr.device != device)
        throw std::runtime_error(who + " is memory of device " + std::to_string(attr.device) + ", the solver's is " + std::to_string(device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess || !base) {
        (void)hipGetLastError();
        return;  // (no range reported)
    }
    const char *end = static_cast<const char *>(base) + size;
    if (static_cast<const char *>(p) + count * sizeof(double) > end)
        throw std::runtime_error(who + " is too short: " + std::to_string(count) + " doubles wanted, " +
                                 std::to_string((end - static_cast<const char *>(p)) / sizeof(double)) + " left in its allocation");
    if (range) *range = DeviceRange{static_cast<const char *>(base), size};
}

// warm-up (abi.cpp: hprlp_warmup): an attribute query makes the runtime load this translation unit's code object now instead
// of at the first launch of one of its kernels
void warm_batched_tu() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&kb_finalize));
}

// ---- the resident solver (DESIGN.md "Resident batches": what is kept over the handle's life, and what while Bp and Bc stay) -------
// Every call, of whichever entry, is one sequence of steps: refuse (before the handle changes); call_parameters; plan_geometry; the
// batch in scaled units into the staging block (prepare_batch and stage_host, or device_prep where it lies); ensure_workspace;
// bind_panels, ws_fill, ws_start; the loop (a streamed call's StreamRun hands slots on inside it); the results; call_succeeded or call_failed.
struct BatchedSolver {
    int m = 0, n = 0;
    double obj_constant = 0.0;
    HPRLP_parameters param;
    Solver shared;  // (before w: the workspace goes first)
    BatchWS w;
    double lambda_created = 1.0;
    bool have_geo = false;   // w holds a workspace
    bool have_prev = false;  // the last call succeeded: X_bar / Y_bar of prev_B members and their scales are on the device,
    int prev_B = 0;          // ... and their caller's-units copy is at the front of w.stage_h (x, then y) -- or, after a
    bool prev_on_device = false, prev_nonfinite = false;  // device-entry call, went to the caller's buffers and left this flag
    long solves = 0, device_solves = 0;
    double seconds[6] = {0, 0, 0, 0, 0, 0};
    int device = 0;                       // the device the matrix lives on
    int norm_rule = kNormRuleReference;   // of the HOST entry (batched_solver_set_norms); the device entry's is the tree rule
    hipEvent_t inputs_ready = nullptr;    // device entry: recorded on the caller's stream, waited for by w.stream
    std::vector<double> last_scalars;     // DS_COUNT x B of the last successful call
    long staged[2] = {0, 0};              // ... and its staging bytes host -> device, device -> host
    // the ray test outside the loop (batched_solver_ray_step): a step since the last solve has stored an iterate; X_bar / Y_bar
    // have been written by name since the last solve (they are no longer that solve's solution: carry is refused)
    bool ray_have_prev = false, bars_written = false;
    // a streamed call (DESIGN.md "Streamed batches"): the last call was one (its panels hold members of many problems: carry, the
    // ray step and the panels by name are refused until the next plain solve); the record and the counts of the last one
    bool streamed = false, have_stream = false;
    std::vector<int> rec_slot, rec_in, rec_out;
    long stream_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool stream_had_parents = false;       // the last streamed call was a parents call ...
    long parents_stats[4] = {0, 0, 0, 0};  // ... and its counts (hprlp_batched_solver_stream_parents_info)
    long stream_mem[4] = {0, 0, 0, 0};  // hprlp_batched_solver_stream_memory: what the last one held beside the workspace
    double stream_seconds[2] = {0, 0};  // of the last streamed call: its refill passes (harvest, refill, iteration-0 evaluation); the rest of its loop
    double lambda_last = 0.0;           // lambda_max at the end of the last successful call of either kind (0: none yet)

    BatchedSolver(const LP_info_cpu *model, const HPRLP_parameters *p);
    ~BatchedSolver() {
        if (inputs_ready) (void)hipEventDestroy(inputs_ready);
    }
    // dev null: the host entry, C .. Y0 host arrays, the results into `out`.  dev set: the device entry, C .. Y0 device arrays
    // ordered on dev->stream, x / y / z into dev's device buffers and the members' scalars into its host arrays.
    void solve(int B, const double *C, const double *AL, const double *AU, const double *l, const double *u, const double *obj_constants,
               const HPRLP_parameters *p, const double *X0, const double *Y0, bool carry, const Detection *det,
               std::vector<Certificate> *certs, HPRLP_batched_results *out, DeviceBatch *dev = nullptr);
    // count problems through min(width, count) slots, a freed slot taking the next queued problem at once.  dev null: host arrays,
    // the results into `out`; dev set: the queue lies in device memory (solve()'s rule for dev).  parents_entry: the call of
    // hprlp_batched_solver_solve_stream_parents[_device] -- parent (host, count entries) says which problem starts from which
    // other's returned point (DESIGN.md "Streamed batches", "Parents").
    void solve_stream(int count, int width, const double *C, const double *AL, const double *AU, const double *l, const double *u,
                      const double *obj_constants, const HPRLP_parameters *p, const double *X0, const double *Y0, const Detection *det,
                      std::vector<Certificate> *certs, HPRLP_batched_results *out, DeviceBatch *dev = nullptr, const int *parent = nullptr,
                      bool parents_entry = false);

    // the handle's parameters with the caller's max_iter, stop_tol, time_limit, check_iter and use_bc_scaling (p null: the handle's)
    HPRLP_parameters call_parameters(const HPRLP_parameters *p) const {
        HPRLP_parameters actual = param;
        if (p) {
            actual.max_iter = p->max_iter; actual.stop_tol = p->stop_tol; actual.time_limit = p->time_limit;
            actual.check_iter = p->check_iter; actual.use_bc_scaling = p->use_bc_scaling;
        }
        return actual;
    }
    // the panel geometry of `members` members (HPRLP_BATCH_CHUNK: per call), and whether the workspace has another
    Geo plan_geometry(int members) const {
        const int Bp = padded_batch(members);
        return make_geo(Bp, choose_chunk(m, n, Bp));
    }
    bool new_geometry(const Geo &g) const { return !have_geo || g.Bp != w.geo.Bp || g.Bw != w.geo.Bw; }
    // what a streamed call has left -- slots that held several problems each -- serves no carry, ray step or panel by name
    void refuse_after_stream(const char *who) const {
        if (streamed)
            throw std::runtime_error(std::string(who) + " refused after a streamed call (its slots held several problems each); a plain solve comes first");
    }
    // a carry's refusals, in this order: what the call asks for, what the handle holds, the geometry, the previous solution's values
    void refuse_carry(int B, const double *X0, const double *Y0, bool new_geo) const {
        if (X0 || Y0) throw std::runtime_error("batched solver: carry takes its starts from the previous batch; X0 and Y0 must be null");
        refuse_after_stream("batched solver: carry");
        if (!have_prev) throw std::runtime_error("batched solver: carry needs a previous successful solve on this handle");
        if (B != prev_B)
            throw std::runtime_error("batched solver: carry needs the previous batch_size (" + std::to_string(prev_B) + "), got " +
                                     std::to_string(B));
        if (bars_written)
            throw std::runtime_error("batched solver: carry refused, X_bar / Y_bar were written by name since the previous solve "
                                     "(they are no longer its solution)");
        if (new_geo) throw std::runtime_error("batched solver: carry needs the previous call's chunk width (HPRLP_BATCH_CHUNK changed)");
        const double *prev = w.stage_h.p;  // x (n x B) and y (m x B) as the previous call returned them
        bool bad = prev_on_device && prev_nonfinite;
        for (size_t i = 0; !prev_on_device && !bad && i < (static_cast<size_t>(n) + m) * B; ++i) bad = !std::isfinite(prev[i]);
        if (bad) throw std::runtime_error("batched solver: carry refused, the previous batch's solution holds a non-finite value");
    }
    // the device entry: no pointer reaches a kernel before all of them have passed
    // (stream: a queue of B problems, whose norm passes are launched in slices: no limit on B)
    void check_device_call(const DeviceBatch &dev, int B, const double *C, const double *AL, const double *AU, const double *l,
                           const double *u, const double *X0, const double *Y0, bool stream = false) {
        const size_t nB = static_cast<size_t>(n) * B, mB = static_cast<size_t>(m) * B;
        const char *entry = stream ? "batched stream" : "batched solver";
        if (B > 65535 && !stream) throw std::runtime_error("batched solver: the device entry takes at most 65535 members");
        const std::pair<const double *, size_t> in_ptrs[5] = {{C, nB}, {AL, mB}, {AU, mB}, {l, nB}, {u, nB}};
        const char *in_names[5] = {"C", "AL", "AU", "l", "u"};
        for (int i = 0; i < 5; ++i) check_device_pointer(in_ptrs[i].first, in_ptrs[i].second, device, in_names[i], entry);
        if (X0) check_device_pointer(X0, nB, device, "X0", entry);
        if (Y0) check_device_pointer(Y0, mB, device, "Y0", entry);
        check_device_pointer(dev.x, nB, device, "x", entry);
        check_device_pointer(dev.y, mB, device, "y", entry);
        check_device_pointer(dev.z, nB, device, "z", entry);
        if (!inputs_ready) HIP_CHECK(hipEventCreateWithFlags(&inputs_ready, hipEventDisableTiming));
    }
    // the workspace of geometry g and lambda_max as created, whatever the handle solved before; the graphs go with a panel, the grid cap or their lambda
    void ensure_workspace(const Geo &g) {
        const char *grid_hook = env_get("HPRLP_BATCH_GRID");
        const int grid_cap = grid_hook ? std::atoi(grid_hook) : 0;
        w.lambda_max = lambda_created;
        if (new_geometry(g)) {
            w.drop_graphs();
            have_geo = false;
            ws_matrix_part(w, shared, g);
            ws_panels(w);
            have_geo = true;
        }
        if (grid_cap != w.grid_cap || (!w.graphs.empty() && w.graph_lambda != w.lambda_max)) w.drop_graphs();
        w.grid_cap = grid_cap;
    }
    template <class Result>  // HPRLP_batched_results, DeviceBatch
    void set_times(Result &r) const {
        r.setup_time = seconds[2] + seconds[3]; r.solve_time = seconds[4]; r.power_time = 0.0;
        r.time = r.setup_time + r.solve_time;
    }
    // what every successful call leaves; data: the batch a later call may carry -- null after a streamed call, which leaves none
    void call_succeeded(size_t h2d_bytes, size_t d2h_bytes, const BatchData *data, bool device_entry) {
        staged[0] = static_cast<long>(h2d_bytes);
        staged[1] = static_cast<long>(d2h_bytes);
        w.data = nullptr;
        if (data) {
            last_scalars.clear();
            const auto scalars = member_scalars(*data);
            for (int i = 0; i < DS_COUNT; ++i) last_scalars.insert(last_scalars.end(), scalars[i]->begin(), scalars[i]->end());
            have_prev = true;
            prev_B = data->B;
        }
        prev_on_device = device_entry;
        ray_have_prev = bars_written = false;
        streamed = !data;
        have_stream = have_stream || streamed;
        lambda_last = w.lambda_max;
        ++solves;
        if (device_entry) ++device_solves;
    }
    // a call that failed half-way: nothing of it is carried, and the next call builds its workspace anew
    void call_failed(bool streamed_call) {
        (void)hipStreamSynchronize(w.stream);
        (void)hipGetLastError();
        w.drop_graphs();
        w.data = nullptr;
        have_geo = false;
        if (streamed_call) streamed = true;
    }
};

// Test hook HPRLP_BATCH_LAMBDA (0: not set): the caller's lambda_max for the power iteration's; of a computed one only the constructor checks
double checked_lambda(double v) {
    if (!(v > 0.0) || !std::isfinite(v)) throw std::runtime_error("HPRLP_BATCH_LAMBDA is not a positive finite number");
    return v;
}
double lambda_hook() {
    const char *hook = env_get("HPRLP_BATCH_LAMBDA");
    return hook ? checked_lambda(std::strtod(hook, nullptr)) : 0.0;
}

BatchedSolver::BatchedSolver(const LP_info_cpu *model, const HPRLP_parameters *p) {
    if (!model || !model->A) throw std::runtime_error("batched solver: null model");
    m = model->m; n = model->n;
    obj_constant = model->obj_constant;
    param = p ? *p : HPRLP_parameters();
    param.use_presolve = false;
    const auto t0 = time_now();
    // shared-A scaling with zero vectors and b/c scaling off (:959-981)
    std::vector<double> zero_m(m, 0.0), zero_n(n, 0.0);
    LP_info_cpu mat{};
    mat.m = m; mat.n = n; mat.A = model->A;
    mat.AL = zero_m.data(); mat.AU = zero_m.data(); mat.c = zero_n.data(); mat.l = zero_n.data(); mat.u = zero_n.data();
    HPRLP_parameters mp = param;
    mp.use_bc_scaling = false;
    shared.verbose = false;
    shared.allow_reorder = false;  // the panels and the returned X / Y / Z are in the caller's numbering
    shared.setup(&mat, &mp);
    shared.scale();
    w.rn.resize(m); w.cn.resize(n);
    shared.row_norm.download(w.rn.data(), m);
    shared.col_norm.download(w.cn.data(), n);
    w.m = m; w.n = n;
    w.shared = &shared;
    w.stream = shared.stream;
    HIP_CHECK(hipGetDevice(&device));
    seconds[0] = time_since(t0);
    const auto t1 = time_now();
    const double hook = lambda_hook();  // lambda_max on the scaled shared matrix (:994-1001), or the hook's
    lambda_created = checked_lambda(hook > 0.0 ? hook : shared.power_iteration(5000, 1.0e-4, nullptr) * 1.01);
    seconds[1] = time_since(t1);
}

void BatchedSolver::solve(int B, const double *C_in, const double *AL_in, const double *AU_in, const double *l_in, const double *u_in,
                          const double *obj_constants, const HPRLP_parameters *p, const double *X0, const double *Y0, bool carry,
                          const Detection *det, std::vector<Certificate> *certs, HPRLP_batched_results *out, DeviceBatch *dev) {
    // -- everything that can refuse the call, before the handle changes
    if (!out && !dev) throw std::runtime_error("batched solver: null results");
    if (B <= 0) throw std::runtime_error("batched solver: batch_size must be positive");
    if (!C_in || !AL_in || !AU_in || !l_in || !u_in) throw std::runtime_error("batched solver: null C / AL / AU / l / u");
    const Geo plan = plan_geometry(B);
    if (carry) refuse_carry(B, X0, Y0, new_geometry(plan));
    if (dev) check_device_call(*dev, B, C_in, AL_in, AU_in, l_in, u_in, X0, Y0);
    const HPRLP_parameters actual = call_parameters(p);
    const bool detect = det && det->on;

    const bool had_prev = have_prev;
    bool refused = false;  // the call is turned away before the workspace has changed
    have_prev = false;     // (until this call has succeeded)
    try {
        // -- the batch in scaled units (:792-885) in the staging block: scaled on the host, or by the device entry's kernels where it is
        const auto t_prep = time_now();
        const Regions regions(plan.Bp, n, m, B, X0 != nullptr, Y0 != nullptr);
        const size_t stage_count = dev ? 0 : regions.end;
        const BatchData data =
            dev ? device_prep(w, B, plan.Bp, &regions, C_in, AL_in, AU_in, l_in, u_in, X0, Y0, obj_constants, obj_constant,
                              actual.use_bc_scaling, static_cast<hipStream_t>(dev->stream), inputs_ready)
                : prepare_batch(m, n, B, C_in, AL_in, AU_in, l_in, u_in, obj_constants, obj_constant, w.rn.data(), w.cn.data(),
                                actual.use_bc_scaling, norm_rule);
        if (dev && data_flags_host(w, B)[DF_START]) {
            refused = true;
            throw std::runtime_error("batched solver: warm start: X0 or Y0 holds a non-finite entry");
        }
        BatchLoop L(data, plan.Bp, actual, detect ? det : nullptr);
        if (!dev) stage_host(w, L, data, regions, data, X0, Y0, stage_count, stage_count);
        seconds[2] = time_since(t_prep);

        // -- device: the workspace where the geometry is new, this batch into it, the start
        const auto t_fill = time_now();
        ensure_workspace(plan);
        std::swap(w.bsc, w.bsc_prev);  // (this batch's scales beside those of the batch before: the swap serves carry, so a
        std::swap(w.csc, w.csc_prev);  // streamed call, which carries nothing, does without it)
        ws_fill(w, data, stage_count, bind_panels(w, regions), regions.nvec, X0 != nullptr, Y0 != nullptr, carry, detect);
        if (X0 || Y0 || carry) ws_start(w);
        HIP_CHECK(hipStreamSynchronize(w.stream));
        seconds[3] = time_since(t_fill);

        L.solve_start = time_now();
        while (true) {  // one pass per event iteration (periodic check or iteration limit), :1017-1084
            const bool periodic = (L.iter % L.check_iter) == 0;
            const double elapsed = time_since(L.solve_start);
            if (periodic) loop_evaluate(w, L, L.iter == 0);
            if (loop_ended(L, elapsed)) break;
            const bool restarted = loop_restart(w, L, periodic);
            loop_advance(w, L, restarted);
        }
        seconds[4] = time_since(L.solve_start);

        const auto t_res = time_now();
        if (dev) prev_nonfinite = device_results(w, L, *dev, certs);
        else *out = collect_results(w, L, certs);
        seconds[5] = time_since(t_res);
        if (dev) set_times(*dev);
        else set_times(*out);
        const size_t back = dev ? static_cast<size_t>(DS_COUNT) * B * sizeof(double) + (DF_COUNT + 1) * sizeof(int)  // the scalars and flag words
                                : (2 * static_cast<size_t>(n) + m) * B * sizeof(double);                            // x, y, z
        call_succeeded(stage_count * sizeof(double), back, &data, dev != nullptr);
    } catch (...) {
        if (refused) {  // nothing the previous call left has been touched
            have_prev = had_prev;
            throw;
        }
        call_failed(/*streamed_call=*/false);
        throw;
    }
}

// ---- streamed batches (DESIGN.md "Streamed batches": the rule, the local iteration numbers, the memory of a call) ----------------
// `count` problems through W = min(width, count) slots of a workspace whose geometry is a plain solve's of W members.  The loop is
// solve()'s; a member that ends at an evaluation hands its slot on within that event (StreamRun).  No panel moves: the graphs survive.
// dev set (DESIGN.md "Device-resident streams"): the queue lies in device memory and is never staged -- device_prep takes its scalars
// where it lies, a problem is scaled on its way into a slot, and x, y, z go to the caller's buffers.
void BatchedSolver::solve_stream(int count, int width, const double *C_in, const double *AL_in, const double *AU_in, const double *l_in,
                                 const double *u_in, const double *obj_constants, const HPRLP_parameters *p, const double *X0,
                                 const double *Y0, const Detection *det, std::vector<Certificate> *certs, HPRLP_batched_results *out,
                                 DeviceBatch *dev, const int *parent, bool parents_entry) {
    // -- everything that can refuse the call, before the handle changes
    const HPRLP_parameters actual = call_parameters(p);
    stream_check_call(dev ? dev->x && dev->y && dev->z : out != nullptr, count, width, C_in && AL_in && AU_in && l_in && u_in,
                      actual.max_iter, actual.check_iter);
    if (parents_entry) {
        stream_check_parents_call(parent, X0 != nullptr, Y0 != nullptr);
        stream_check_parents(count, parent);
    }
    const size_t nN = static_cast<size_t>(n) * count, mN = static_cast<size_t>(m) * count;
    for (size_t i = 0; !dev && X0 && i < nN; ++i)
        if (!std::isfinite(X0[i])) throw std::runtime_error("batched stream: warm start: X0[" + std::to_string(i) + "] is not finite");
    for (size_t i = 0; !dev && Y0 && i < mN; ++i)
        if (!std::isfinite(Y0[i])) throw std::runtime_error("batched stream: warm start: Y0[" + std::to_string(i) + "] is not finite");
    if (dev) check_device_call(*dev, count, C_in, AL_in, AU_in, l_in, u_in, X0, Y0, /*stream=*/true);
    const int W = std::min(width, count);
    const Geo plan = plan_geometry(W);
    const bool detect = det && det->on;

    const bool had_prev = have_prev;
    bool refused = false;  // a device-entry call is turned away by its norm passes, before the workspace has changed
    have_prev = false;     // the panels will hold members of many problems: nothing of this call is carried
    try {
        // -- the whole queue in scaled units, into the pinned block behind the header of the first W members; a device-entry call: its
        //    scalars from where it lies, and the header
        const auto t_prep = time_now();
        const BatchData q =
            dev ? device_prep(w, count, count, nullptr, C_in, AL_in, AU_in, l_in, u_in, X0, Y0, obj_constants, obj_constant,
                              actual.use_bc_scaling, static_cast<hipStream_t>(dev->stream), inputs_ready)
                : prepare_batch(m, n, count, C_in, AL_in, AU_in, l_in, u_in, obj_constants, obj_constant, w.rn.data(), w.cn.data(),
                                actual.use_bc_scaling, norm_rule);
        if (dev && data_flags_host(w, count)[DF_START]) {
            refused = true;
            throw std::runtime_error("batched stream: warm start: X0 or Y0 holds an entry that is not finite");
        }
        StreamRun run(w, q, W, plan.Bp, actual, detect ? det : nullptr, X0 != nullptr, Y0 != nullptr, dev, parent);
        BatchLoop &L = run.L;
        run.stage(X0, Y0);
        seconds[2] = time_since(t_prep);

        // -- device: the first W problems as a plain solve's batch (no swap of bsc / csc with their _prev twins: see solve())
        const auto t_fill = time_now();
        ensure_workspace(plan);
        const PanelIn in = bind_panels(w, run.regions);  // the initial fill: the first W columns of every region
        if (dev) {  // (a problem that never started: zero vectors)
            HIP_CHECK(hipMemsetAsync(dev->x, 0, nN * sizeof(double), w.stream));
            HIP_CHECK(hipMemsetAsync(dev->y, 0, mN * sizeof(double), w.stream));
            HIP_CHECK(hipMemsetAsync(dev->z, 0, nN * sizeof(double), w.stream));
        }
        if (run.res_count) HIP_CHECK(hipMemsetAsync(w.res_d.p, 0, run.res_count * sizeof(double), w.stream));
        // (a parents call: the header alone, every slot inactive, X and Y zero throughout; its initial fill is the loop's first pass)
        ws_fill(w, run.sd, run.stage_count, in, dev || parent ? 0 : run.regions.nvec, X0 != nullptr && !parent, Y0 != nullptr && !parent,
                /*carry=*/false, detect);
        if (dev) {  // the first W problems from the caller's arrays, by the refill's kernel
            run.bind(in);
            run.bind_caller(C_in, AL_in, AU_in, l_in, u_in, X0, Y0);
            if (!parent) run.fill_first();
        }
        if ((X0 || Y0) && !parent) ws_start(w);
        if (!dev) run.bind(in);
        if (parent) {
            run.bind_starts(X0, Y0);
            run.clear_data_panels();
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(w.stream));
        seconds[3] = time_since(t_fill);

        double refill_seconds = 0.0;
        L.solve_start = time_now();
        while (true) {  // one pass per periodic event
            const double elapsed = time_since(L.solve_start);
            const bool time_up = elapsed >= actual.time_limit;
            if (parent && L.iter == 0) {  // 1. a parents call's initial fill: the roots' iteration-0 evaluation (nothing enters once the time is up)
                if (!time_up) run.first_pass();
            } else {
                loop_evaluate(w, L, L.iter == 0);  // 1. every occupied slot, by its local iteration
            }
            ++run.evals;
            const auto t_pass = time_now();
            bool refilled = false, active_stale = false;  // (stale: a limit has changed the active mask and no evaluation has uploaded it)
            while (run.pass(time_up, active_stale)) refilled = true;  // 2. harvest, 3. refill, 4. iteration-0 evaluation
            if (active_stale) w.active.upload(L.active.data(), w.Bp);
            if (refilled) ++run.refill_events;
            refill_seconds += time_since(t_pass);
            if (!run.occupied()) {
                // No deadlock: parent[p] < p, so with nothing running the lowest-numbered waiting problem has a parent that has been
                // harvested, and the pass above has taken it.  Were that ever violated the loop would spin on empty slots: fail instead.
                if (parent && !time_up && run.pqueue.left() > 0)
                    throw std::logic_error("batched stream: " + std::to_string(run.pqueue.left()) + " problems wait for a parent and no slot is occupied");
                break;
            }
            if (parent && run.pqueue.left() > 0) run.idle_slot_events += W - run.occupied_slots();
            const bool restarted = loop_restart(w, L, true);  // 5. an empty slot is an inactive one
            loop_advance(w, L, restarted);
        }
        seconds[4] = time_since(L.solve_start);

        // -- the results: one download; a device-entry call: the members' scalars, and the rays of the verdicts
        const auto t_res = time_now();
        size_t back = run.res_count * sizeof(double);
        if (dev) {
            back = static_cast<size_t>(DS_COUNT) * count * sizeof(double) + DF_COUNT * sizeof(int) + run.results_device(certs);
            seconds[5] = time_since(t_res);
            set_times(*dev);
        } else {
            HPRLP_batched_results res = run.results(certs);
            seconds[5] = time_since(t_res);
            set_times(res);
            *out = res;
        }
        const long stats[8] = {count, width, L.iter, run.evals, run.refill_events, run.refills, run.passes, w.bumps - run.bumps0};
        std::copy(stats, stats + 8, stream_stats);
        const long pstats[4] = {run.entered_roots, run.entered_cold, run.entered_children, run.idle_slot_events};
        std::copy(pstats, pstats + 4, parents_stats);
        stream_had_parents = parent != nullptr;
        rec_slot = std::move(run.r_slot); rec_in = std::move(run.r_in); rec_out = std::move(run.r_out);
        stream_seconds[0] = refill_seconds;
        stream_seconds[1] = seconds[4] - refill_seconds;
        const size_t header = 4 * static_cast<size_t>(plan.Bp);  // what the call held: the queue's vectors | the result / ray block |
        const size_t scalars = dev ? w.data_scal.n + w.data_part.n : 3 * static_cast<size_t>(count);  // scalars, partials, tables | pinned
        // (a parents call of the host entry: the caller's X0 / Y0, staged as they are, count among the queue's vectors)
        const long mem[4] = {static_cast<long>((run.stage_count - header - (dev ? 0 : scalars)) * sizeof(double)),
                             static_cast<long>(run.res_count * sizeof(double)),
                             static_cast<long>((header + scalars) * sizeof(double) + w.tab_d.n * sizeof(int)),
                             static_cast<long>((w.stage_h.n + (dev ? w.data_scal_h.n : 0)) * sizeof(double) + w.tab_h.n * sizeof(int))};
        std::copy(mem, mem + 4, stream_mem);
        call_succeeded(run.stage_count * sizeof(double), back, nullptr, /*device_entry=*/dev != nullptr);
    } catch (...) {
        if (refused) {  // nothing the previous call left has been touched
            have_prev = had_prev;
            throw;
        }
        call_failed(/*streamed_call=*/true);
        throw;
    }
}

BatchedSolver *batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param) { return new BatchedSolver(model, param); }
void batched_solver_solve_stream(BatchedSolver *h, int count, int width, const double *C, const double *AL, const double *AU, const double *l,
                                 const double *u, const double *obj_constants, const HPRLP_parameters *param, const double *X0,
                                 const double *Y0, const Detection *det, std::vector<Certificate> *certs, HPRLP_batched_results *out) {
    if (!h) throw std::runtime_error("batched stream: null handle");
    h->solve_stream(count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, det, certs, out);
}
void batched_solver_solve_stream_device(BatchedSolver *h, int count, int width, const double *C, const double *AL, const double *AU,
                                        const double *l, const double *u, const double *obj_constants, const HPRLP_parameters *param,
                                        const double *X0, const double *Y0, const Detection *det, std::vector<Certificate> *certs,
                                        DeviceBatch *dev) {
    if (!h || !dev) throw std::runtime_error("batched stream: null handle / device batch");
    h->solve_stream(count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, det, certs, nullptr, dev);
}
void batched_solver_solve_stream_parents(BatchedSolver *h, int count, int width, const double *C, const double *AL, const double *AU,
                                         const double *l, const double *u, const double *obj_constants, const HPRLP_parameters *param,
                                         const double *X0, const double *Y0, const int *parent, const Detection *det,
                                         std::vector<Certificate> *certs, HPRLP_batched_results *out, DeviceBatch *dev) {
    if (!h) throw std::runtime_error("batched stream: null handle");
    h->solve_stream(count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, det, certs, out, dev, parent, /*parents_entry=*/true);
}
void batched_solver_stream_parents_info(const BatchedSolver *h, long out[4]) {
    if (!h || !out) throw std::runtime_error("batched stream parents info: null handle / output");
    if (!h->have_stream || !h->stream_had_parents)
        throw std::runtime_error("batched stream parents info: the last successful stream call on this handle was not a parents call");
    std::copy(h->parents_stats, h->parents_stats + 4, out);
}
void batched_solver_stream_memory(const BatchedSolver *h, long out[4]) {
    if (!h || !out) throw std::runtime_error("batched stream memory: null handle / output");
    if (!h->have_stream) throw std::runtime_error("batched stream memory: no successful stream call on this handle");
    std::copy(h->stream_mem, h->stream_mem + 4, out);
}
int batched_solver_stream_record(const BatchedSolver *h, int *slot, int *event_in, int *event_out) {
    if (!h || !slot || !event_in || !event_out) throw std::runtime_error("batched stream record: null handle / output");
    if (!h->have_stream) throw std::runtime_error("batched stream record: no successful stream call on this handle");
    std::copy(h->rec_slot.begin(), h->rec_slot.end(), slot);
    std::copy(h->rec_in.begin(), h->rec_in.end(), event_in);
    std::copy(h->rec_out.begin(), h->rec_out.end(), event_out);
    return static_cast<int>(h->rec_slot.size());
}
void batched_solver_stream_info(const BatchedSolver *h, long out[8], double seconds[2]) {
    if (!h || !out) throw std::runtime_error("batched stream info: null handle / output");
    if (!h->have_stream) throw std::runtime_error("batched stream info: no successful stream call on this handle");
    std::copy(h->stream_stats, h->stream_stats + 8, out);
    if (seconds) std::copy(h->stream_seconds, h->stream_seconds + 2, seconds);
}
void batched_solver_lambda(const BatchedSolver *h, double out[2]) {
    if (!h || !out) throw std::runtime_error("batched solver lambda: null handle / output");
    out[0] = h->lambda_created;
    out[1] = h->lambda_last > 0.0 ? h->lambda_last : h->lambda_created;
}
void batched_solver_destroy(BatchedSolver *h) { delete h; }
void batched_solver_solve(BatchedSolver *h, int batch_size, const double *C, const double *AL, const double *AU, const double *l,
                          const double *u, const double *obj_constants, const HPRLP_parameters *param, const double *X0, const double *Y0,
                          bool carry, const Detection *det, std::vector<Certificate> *certs, HPRLP_batched_results *out) {
    if (!h) throw std::runtime_error("batched solver: null handle");
    h->solve(batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, carry, det, certs, out);
}
void batched_solver_solve_device(BatchedSolver *h, int batch_size, const double *C, const double *AL, const double *AU, const double *l,
                                 const double *u, const double *obj_constants, const HPRLP_parameters *param, const double *X0,
                                 const double *Y0, bool carry, const Detection *det, std::vector<Certificate> *certs, DeviceBatch *dev) {
    if (!h || !dev) throw std::runtime_error("batched solver: null handle / device batch");
    h->solve(batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, carry, det, certs, nullptr, dev);
}
// New values on the shared pattern (DESIGN.md "Matrix values"): what the constructor does after setup(), on the resident solver.
// Panels, staging blocks, order tables and the workspace stay; the graphs hold lambda by value and follow graph_lambda at the
// next call.  The previous solution was mapped with the old factors: nothing is carried across.
void batched_solver_set_matrix_values(BatchedSolver *h, const double *val, long nnz) {
    if (!h) throw std::runtime_error("batched solver: null handle");
    if (!val) throw std::runtime_error("batched solver: null matrix values");
    const double hook = lambda_hook();  // (a hook that is no lambda refuses the call here, before anything changes)
    HIP_CHECK(hipStreamSynchronize(h->w.stream));
    const auto t0 = time_now();
    const std::vector<double> zero_m(static_cast<size_t>(std::max(h->m, 1)), 0.0), zero_n(static_cast<size_t>(std::max(h->n, 1)), 0.0);
    // (refuses a wrong nnz and a non-finite value before the shared solver has changed)
    h->shared.set_matrix_values(val, nnz, zero_n.data(), nullptr, zero_m.data(), zero_m.data(), zero_n.data(), zero_n.data());
    h->have_prev = false;
    h->shared.row_norm.download(h->w.rn.data(), h->m);
    h->shared.col_norm.download(h->w.cn.data(), h->n);
    h->seconds[0] += time_since(t0);
    const auto t1 = time_now();
    h->lambda_created = hook > 0.0 ? hook : h->shared.power_iteration(5000, 1.0e-4, nullptr) * 1.01;
    h->seconds[1] += time_since(t1);
}
void batched_solver_set_norms(BatchedSolver *h, int rule) {
    if (!h) throw std::runtime_error("batched solver: null handle");
    if (rule != kNormRuleReference && rule != kNormRuleTree) throw std::runtime_error("batched solver: the norm rule is 0 (reference) or 1 (tree)");
    h->norm_rule = rule;
}
int batched_solver_scalars(const BatchedSolver *h, double *out) {
    if (!h || !out) throw std::runtime_error("batched solver: null handle / output");
    if (!h->have_prev) throw std::runtime_error("batched solver: no successful solve to report the scalars of");
    std::copy(h->last_scalars.begin(), h->last_scalars.end(), out);
    return h->prev_B;
}
void batched_solver_transfer(const BatchedSolver *h, long out[4]) {
    if (!h || !out) throw std::runtime_error("batched solver: null handle / output");
    const long v[4] = {h->staged[0], h->staged[1], h->prev_on_device ? 1 : 0, h->device_solves};
    std::copy(v, v + 4, out);
}
void batched_solver_info(const BatchedSolver *h, long out[8]) {
    if (!h || !out) throw std::runtime_error("batched solver: null handle / output");
    const long v[8] = {h->m, h->n, h->solves, h->have_geo ? h->w.geo.Bp : 0, h->have_geo ? h->w.geo.Bw : 0, h->w.captures,
                       static_cast<long>(h->w.graphs.size()), h->w.panel_allocs};
    std::copy(v, v + 8, out);
}
void batched_solver_seconds(const BatchedSolver *h, double out[6]) {
    if (!h || !out) throw std::runtime_error("batched solver: null handle / output");
    std::copy(h->seconds, h->seconds + 6, out);
}


// ---- the ray test outside the loop (DESIGN.md "Batched detection": the ray test by value) -----------------------------------------
// One ray test on the panels the last successful solve left: its B, its geometry, its scales on the device.  The launches, the
// fetch and the slot reads are the loop's own (ray_step, fetch, sc); nothing of the finished solve's host BatchData is read.
// active (B ints): the members that take part, as the loop's active mask; padding members never do.  restart: the stored iterate
// and the rays are forgotten (zeroed, as a detecting solve starts) and the step only stores X_bar / Y_bar of the active members --
// a member that sat out a restart step has a zero stored iterate at its first test.  out: 9 x B raw slots, slot-major, in the
// order of BRaySlot (DY, CD, VY, WD, YN, DN, DZ, VZ, WQ); tested[k]: 1 where member k was tested.  Returns 1 after a test, 0
// where the iterate was only stored.  The next solve on the handle fills every buffer a step touches (active, slots, partials, the
// detection's panels) as on a handle that never stepped.
int batched_solver_ray_step(BatchedSolver *h, const int *active, bool restart, double *out, int *tested) {
    if (!h || !active || !out || !tested) throw std::runtime_error("batched ray step: null handle / active / output");
    h->refuse_after_stream("batched ray step:");
    if (!h->have_prev || !h->have_geo) throw std::runtime_error("batched ray step: needs a successful solve on this handle");
    if (!restart && !h->ray_have_prev)
        throw std::runtime_error("batched ray step: no stored iterate, the first step after a solve needs restart != 0");
    BatchWS &w = h->w;
    const int B = w.B;
    std::vector<int> act(static_cast<size_t>(w.Bp), 0);
    for (int k = 0; k < B; ++k) act[k] = active[k] != 0 ? 1 : 0;
    if (restart) ws_ray_panels(w);
    w.active.upload(act.data(), act.size());
    w.nslot = B_NSLOT_DETECT;
    const bool test = !restart;
    ray_step(w, test);
    HIP_CHECK(hipGetLastError());
    fetch(w);
    h->ray_have_prev = true;
    for (int k = 0; k < B; ++k) {
        tested[k] = test ? act[k] : 0;
        for (int s = 0; s < B_NSLOT_DETECT - B_NSLOT; ++s) out[static_cast<size_t>(s) * B + k] = tested[k] ? sc(w, B_RAY_DY + s, k) : 0.0;
    }
    return test ? 1 : 0;
}

namespace {
// a panel by name: its buffer, its rows, and whether a caller may write it
struct NamedPanel {
    const char *name;
    DBuf<double> BatchWS::*buf;
    bool x_side;  // n rows (else m)
    bool ray;     // one of the detection's panels: unknown until a detecting solve or a ray step has allocated them
    bool writable;
};
constexpr NamedPanel kNamedPanels[] = {
    {"C", &BatchWS::C, true, false, false},          {"AL", &BatchWS::AL, false, false, false},
    {"AU", &BatchWS::AU, false, false, false},       {"L", &BatchWS::L, true, false, false},
    {"U", &BatchWS::U, true, false, false},          {"X_bar", &BatchWS::Xb, true, false, true},
    {"Y_bar", &BatchWS::Yb, false, false, true},     {"ray_d", &BatchWS::DS, true, true, false},
    {"ray_y", &BatchWS::YS, false, true, false},     {"ray_prev_x", &BatchWS::prevX, true, true, false},
    {"ray_prev_y", &BatchWS::prevY, false, true, false}, {"ray_z", &BatchWS::Zray, true, true, false},
    // what a warm start seeds and forms (ws_start), for the tests that check it by value
    {"X", &BatchWS::X, true, false, false},          {"X_hat", &BatchWS::Xh, true, false, false},
    {"last_X", &BatchWS::lastX, true, false, false}, {"Y", &BatchWS::Y, false, false, false},
    {"last_Y", &BatchWS::lastY, false, false, false}, {"Z_bar", &BatchWS::Zb, true, false, false},
    {"Y_obj", &BatchWS::Yobj, false, false, false},
};
const NamedPanel &named_panel(const BatchWS &w, const std::string &name, const char *who) {
    for (const NamedPanel &p : kNamedPanels)
        if (name == p.name) {
            if (p.ray && !w.prevX.p) throw std::runtime_error(std::string(who) + ": '" + name + "' does not exist before a detecting solve or a ray step");
            return p;
        }
    throw std::runtime_error(std::string(who) + ": unknown panel '" + name + "'");
}
}  // namespace

// The first B members of a panel of the last successful solve by name, column-major rows x B (download_panel): C, AL, AU, L, U,
// X_bar, Y_bar, X, X_hat, last_X, Y, last_Y, Z_bar, Y_obj, ray_d, ray_y, ray_prev_x, ray_prev_y; ray_z runs launch_ray_product and returns its product A^T ray_y; row_norm /
// col_norm: the shared matrix' norms (m / n values).  "raw:" in front of a panel's name: the whole padded panel in the device's
// layout, rows x Bp (panel_index).  out null: only the count.  Returns the count of values; throws where `len` is another.
long batched_solver_get_panel(BatchedSolver *h, const char *name, double *out, long len) {
    if (!h || !name) throw std::runtime_error("batched get_panel: null handle / name");
    h->refuse_after_stream("batched get_panel:");
    if (!h->have_prev || !h->have_geo) throw std::runtime_error("batched get_panel: needs a successful solve on this handle");
    BatchWS &w = h->w;
    std::string nm(name);
    const bool norm = nm == "row_norm" || nm == "col_norm";
    const bool raw = nm.rfind("raw:", 0) == 0;
    if (raw) nm = nm.substr(4);
    const NamedPanel *p = norm ? nullptr : &named_panel(w, nm, "batched get_panel");
    const int rows = norm ? (nm == "row_norm" ? w.m : w.n) : (p->x_side ? w.n : w.m);
    const long count = norm ? rows : static_cast<long>(rows) * (raw ? w.Bp : w.B);
    if (!out) return count;
    if (len != count) throw std::runtime_error("batched get_panel: '" + nm + "' has " + std::to_string(count) + " values, room for " + std::to_string(len));
    std::vector<double> v;
    if (norm) {
        v = nm == "row_norm" ? w.rn : w.cn;
    } else {
        if (nm == "ray_z") {
            w.Zray.alloc(static_cast<size_t>(w.n) * w.Bp);
            launch_ray_product(w);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(w.stream));
        const DBuf<double> &buf = w.*(p->buf);
        if (raw) {
            v.resize(static_cast<size_t>(count));
            buf.download(v.data(), v.size());
        } else {
            v = download_panel(w, buf, rows);
        }
    }
    std::copy(v.begin(), v.end(), out);
    return count;
}

// X_bar / Y_bar of the first B members from column-major rows x B (to_panel; the padding members' columns become 0.0, which is
// what they hold).  No other panel can be written.  carry is refused until the next successful solve.
void batched_solver_set_panel(BatchedSolver *h, const char *name, const double *in, long len) {
    if (!h || !name || !in) throw std::runtime_error("batched set_panel: null handle / name / values");
    h->refuse_after_stream("batched set_panel:");
    if (!h->have_prev || !h->have_geo) throw std::runtime_error("batched set_panel: needs a successful solve on this handle");
    BatchWS &w = h->w;
    const NamedPanel &p = named_panel(w, name, "batched set_panel");
    if (!p.writable) throw std::runtime_error(std::string("batched set_panel: '") + name + "' cannot be written (X_bar and Y_bar can)");
    const int rows = p.x_side ? w.n : w.m;
    const long count = static_cast<long>(rows) * w.B;
    if (len != count) throw std::runtime_error(std::string("batched set_panel: '") + name + "' takes " + std::to_string(count) + " values, got " + std::to_string(len));
    const std::vector<double> cm(in, in + count);
    std::vector<double> panel;
    to_panel(cm, rows, w.B, w.geo, 0.0, panel);
    HIP_CHECK(hipStreamSynchronize(w.stream));
    (w.*(p.buf)).upload(panel.data(), panel.size());
    h->bars_written = true;
}

// One batch and no more: a resident solver that lives for one call.  Its set-up, scaling and power iteration count as this call's set-up.
HPRLP_batched_results solve_batched_impl(const LP_info_cpu *model, int batch_size, const HPRLP_FLOAT *C_in, const HPRLP_FLOAT *AL_in,
                                         const HPRLP_FLOAT *AU_in, const HPRLP_FLOAT *l_in, const HPRLP_FLOAT *u_in,
                                         const HPRLP_FLOAT *obj_constants, const HPRLP_parameters *param, const Detection *det,
                                         std::vector<Certificate> *certs, const HPRLP_FLOAT *X0, const HPRLP_FLOAT *Y0) {
    if (!model || !model->A || batch_size <= 0 || !C_in || !AL_in || !AU_in || !l_in || !u_in)
        return make_batched_error("ERROR", model ? model->m : 0, model ? model->n : 0, std::max(batch_size, 0));
    try {
        BatchedSolver h(model, param);
        HPRLP_batched_results out;
        h.solve(batch_size, C_in, AL_in, AU_in, l_in, u_in, obj_constants, nullptr, X0, Y0, false, det, certs, &out);
        out.setup_time += h.seconds[0] + h.seconds[1];
        out.power_time = h.shared.power_time;
        out.time = out.setup_time + out.solve_time;
        return out;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        std::cerr << "[error] solve_batched failed: " << e.what() << std::endl;
        return make_batched_error("ERROR", model->m, model->n, batch_size);
    }
}

}  // namespace hprlp

using namespace hprlp;

extern "C" HPRLP_batched_results solve_batched(const LP_info_cpu *model, int batch_size, const HPRLP_FLOAT *C_in,
                                               const HPRLP_FLOAT *AL_in, const HPRLP_FLOAT *AU_in,
                                               const HPRLP_FLOAT *l_in, const HPRLP_FLOAT *u_in,
                                               const HPRLP_FLOAT *obj_constants, const HPRLP_parameters *param) {
    return solve_batched_impl(model, batch_size, C_in, AL_in, AU_in, l_in, u_in, obj_constants, param, nullptr, nullptr);
}

extern "C" void free_batched_results(HPRLP_batched_results *results) {  // :1094-1105
    if (!results) return;
    std::free(results->x); std::free(results->y); std::free(results->z);
    std::free(results->primal_obj); std::free(results->residuals); std::free(results->gap);
    std::free(results->iter); std::free(results->status);
    *results = HPRLP_batched_results();
}
