// batch_prep.cpp -- see batch_prep.h.  Host only.  The arithmetic of every element and scalar is batch_units.h's, the order of its
// operations included; tests/test_batch_prep.py holds every one of them to its bits.
#include "batch_prep.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "HPRLP.h"
#include "env.h"

namespace hprlp {

HPRLP_batched_results make_batched_error(const char *status, int m, int n, int B) {
    HPRLP_batched_results r;
    r.m = m;
    r.n = n;
    r.batch_size = B;
    if (B > 0) {
        r.status = static_cast<char *>(std::calloc(static_cast<size_t>(B) * 64, sizeof(char)));
        if (r.status)
            for (int k = 0; k < B; ++k) std::strncpy(r.status + 64 * k, status, 63);
    }
    return r;
}

HPRLP_batched_results alloc_batched_results(int m, int n, int B) {
    HPRLP_batched_results out;
    out.m = m; out.n = n; out.batch_size = B;
    out.x = static_cast<double *>(std::malloc(sizeof(double) * static_cast<size_t>(n) * B));
    out.y = static_cast<double *>(std::malloc(sizeof(double) * static_cast<size_t>(m) * B));
    out.z = static_cast<double *>(std::malloc(sizeof(double) * static_cast<size_t>(n) * B));
    out.primal_obj = static_cast<double *>(std::malloc(sizeof(double) * B));
    out.residuals = static_cast<double *>(std::malloc(sizeof(double) * B));
    out.gap = static_cast<double *>(std::malloc(sizeof(double) * B));
    out.iter = static_cast<int *>(std::malloc(sizeof(int) * B));
    out.status = static_cast<char *>(std::calloc(static_cast<size_t>(B) * 64, sizeof(char)));
    if (!out.x || !out.y || !out.z || !out.primal_obj || !out.residuals || !out.gap || !out.iter || !out.status) {
        free_batched_results(&out);
        throw std::runtime_error("host allocation of the batched results failed");
    }
    return out;
}

int padded_batch(int B) {
    if (B <= 64) {
        int p = 1;
        while (p < B) p <<= 1;
        return p;
    }
    return (B + 63) / 64 * 64;
}

int choose_chunk(int m, int n, int Bp) {
    if (Bp < 64) return Bp;
    if (const char *e = env_get("HPRLP_BATCH_CHUNK")) {
        const int c = std::atoi(e);
        if (c == 8 || c == 16 || c == 32 || c == 64) return c;
    }
    (void)m; (void)n;
    return 64;
}

void to_panel(const std::vector<double> &cm, int rows, int B, const Geo &g, double pad, std::vector<double> &out) {
    out.assign(static_cast<size_t>(rows) * g.Bp, pad);
    for (int k = 0; k < B; ++k)
        for (int i = 0; i < rows; ++i) out[panel_index(g, rows, i, k)] = cm[static_cast<size_t>(k) * rows + i];
}

void from_panel(const std::vector<double> &panel, int rows, int B, const Geo &g, double *cm) {
    for (int k = 0; k < B; ++k)
        for (int i = 0; i < rows; ++i) cm[static_cast<size_t>(k) * rows + i] = panel[panel_index(g, rows, i, k)];
}

namespace {

// the tree rule (batch_prep.h) for the values value(0) .. value(rows - 1)
template <class F>
double tree_sum_of_squares(int rows, F value) {
    double total = 0.0;
    for (int s = 0; s < norm_segments(rows); ++s) {
        double a[kNormLanes];
        std::fill(a, a + kNormLanes, 0.0);
        const int i0 = s * kNormSeg, end = std::min(rows, i0 + kNormSeg);
        for (int i = i0; i < end; ++i) {
            const double v = value(i);
            const double t = v * v;
            a[(i - i0) % kNormLanes] += t;
        }
        for (int stride = kNormLanes / 2; stride >= 1; stride /= 2)
            for (int j = 0; j < stride; ++j) a[j] += a[j + stride];
        total += a[0];
    }
    return total;
}

// the sum of squares of value(0) .. value(rows - 1) by either rule
template <class F>
double sum_of_squares(int rows, int rule, F value) {
    if (rule == kNormRuleTree) return tree_sum_of_squares(rows, value);
    long double sum = 0.0;
    for (int i = 0; i < rows; ++i) {
        const double v = value(i);
        sum += static_cast<long double>(v) * v;
    }
    return static_cast<double>(sum);
}
double bound_squares(const double *AL, const double *AU, int m, size_t off, int rule) {  // :332-345
    return sum_of_squares(m, rule, [&](int i) { return bound_value(AL[off + i], AU[off + i]); });
}
double column_squares(const double *X, int n, size_t off, int rule) {  // :347-354
    return sum_of_squares(n, rule, [&](int i) { return X[off + i]; });
}

}  // namespace

BatchData prepare_batch(int m, int n, int B, const double *C, const double *AL, const double *AU, const double *l, const double *u,
                        const double *obj_constants, double model_obj_constant, const double *rn, const double *cn,
                        bool use_bc_scaling, int norm_rule) {
    if (norm_rule != kNormRuleReference && norm_rule != kNormRuleTree) throw std::runtime_error("prepare_batch: norm rule must be 0 (reference) or 1 (tree)");
    BatchData d;
    d.m = m; d.n = n; d.B = B;
    const size_t nB = static_cast<size_t>(n) * B, mB = static_cast<size_t>(m) * B;
    d.C.assign(C, C + nB); d.AL.assign(AL, AL + mB); d.AU.assign(AU, AU + mB); d.L.assign(l, l + nB); d.U.assign(u, u + nB);
    std::vector<double> &hC = d.C, &hAL = d.AL, &hAU = d.AU, &hL = d.L, &hU = d.U;
    d.b_scale.assign(B, 1.0); d.c_scale.assign(B, 1.0); d.sigma.assign(B, 1.0);
    for (std::vector<double> *p : {&d.norm_b, &d.norm_c, &d.norm_b_org, &d.norm_c_org, &d.objc}) p->assign(B, 0.0);
    for (int k = 0; k < B; ++k) {
        const size_t om = static_cast<size_t>(k) * m, on = static_cast<size_t>(k) * n;
        d.norm_b_org[k] = one_plus_norm(bound_squares(hAL.data(), hAU.data(), m, om, norm_rule));
        d.norm_c_org[k] = one_plus_norm(column_squares(hC.data(), n, on, norm_rule));
        for (int i = 0; i < m; ++i) { hAL[om + i] = over_norm(hAL[om + i], rn[i]); hAU[om + i] = over_norm(hAU[om + i], rn[i]); }
        for (int i = 0; i < n; ++i) {
            hC[on + i] = over_norm(hC[on + i], cn[i]);
            hL[on + i] = times_norm(hL[on + i], cn[i]);
            hU[on + i] = times_norm(hU[on + i], cn[i]);
        }
    }
    if (use_bc_scaling) {
        for (int k = 0; k < B; ++k) {
            const size_t om = static_cast<size_t>(k) * m, on = static_cast<size_t>(k) * n;
            const double bs = d.b_scale[k] = one_plus_norm(bound_squares(hAL.data(), hAU.data(), m, om, norm_rule));
            const double cs = d.c_scale[k] = one_plus_norm(column_squares(hC.data(), n, on, norm_rule));
            for (int i = 0; i < m; ++i) { hAL[om + i] = by_scale(hAL[om + i], bs); hAU[om + i] = by_scale(hAU[om + i], bs); }
            for (int i = 0; i < n; ++i) {
                hC[on + i] = by_scale(hC[on + i], cs);
                hL[on + i] = by_scale(hL[on + i], bs);
                hU[on + i] = by_scale(hU[on + i], bs);
            }
        }
    }
    for (int k = 0; k < B; ++k) {
        const size_t om = static_cast<size_t>(k) * m, on = static_cast<size_t>(k) * n;
        d.norm_b[k] = std::sqrt(bound_squares(hAL.data(), hAU.data(), m, om, norm_rule));
        d.norm_c[k] = std::sqrt(column_squares(hC.data(), n, on, norm_rule));
        for (int i = 0; i < m; ++i) { hAL[om + i] = lower_replaced(hAL[om + i]); hAU[om + i] = upper_replaced(hAU[om + i]); }
        for (int i = 0; i < n; ++i) { hL[on + i] = lower_replaced(hL[on + i]); hU[on + i] = upper_replaced(hU[on + i]); }
        d.objc[k] = obj_constants ? obj_constants[k] : model_obj_constant;
        d.sigma[k] = first_sigma(d.norm_b[k], d.norm_c[k]);
    }
    return d;
}

void start_to_scaled(double *v, int rows, int B, const double *norm, const std::vector<double> &scale) {
    for (int k = 0; k < B; ++k)
        for (int i = 0; i < rows; ++i) v[static_cast<size_t>(k) * rows + i] = start_to_scaled(v[static_cast<size_t>(k) * rows + i], norm[i], scale[k]);
}

void point_to_caller(double *v, int rows, int B, const double *norm, const std::vector<double> &scale) {
    for (int k = 0; k < B; ++k)
        for (int i = 0; i < rows; ++i) v[static_cast<size_t>(k) * rows + i] = point_to_caller(v[static_cast<size_t>(k) * rows + i], norm[i], scale[k]);
}

void reduced_cost_to_caller(double *z, int n, int B, const double *cn, const std::vector<double> &c_scale) {
    for (int k = 0; k < B; ++k)
        for (int i = 0; i < n; ++i) z[static_cast<size_t>(k) * n + i] = reduced_cost_to_caller(z[static_cast<size_t>(k) * n + i], cn[i], c_scale[k]);
}

}  // namespace hprlp
