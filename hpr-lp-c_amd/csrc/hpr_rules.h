// hpr_rules.h -- the host side of the HPR restart, sigma and residual rules and of the infeasibility detection's verdict, shared
// by the single-LP loop (Solver::solve_loop, solver.cpp) and solve_batched (batched.hip), which applies them member by member.
// Plain host code: no HIP calls.
#pragma once

#include <algorithm>
#include <cmath>
#include <iostream>
#include <limits>
#include <vector>

namespace hprlp {

struct Residuals {  // reference HPRLP_residuals, include/structs.h:255-263
    double err_Rp = 0, err_Rd = 0, primal_obj = 0, dual_obj = 0, rel_gap = 0;
    double kkt = std::numeric_limits<double>::infinity();
};

struct RestartState {  // reference HPRLP_restart, include/structs.h:215-228
    int flag = 0;
    bool first = true;
    double last_gap = std::numeric_limits<double>::infinity();
    double current_gap = std::numeric_limits<double>::infinity();
    double save_gap = std::numeric_limits<double>::infinity();
    double best_gap = std::numeric_limits<double>::infinity();
    double best_sigma = 1.0;
    int inner = 0;
};

// Infeasibility detection (opt-in, one GPU; DESIGN.md "Infeasibility and unboundedness"): the Farkas ratio tests' tolerances ...
struct Detection {
    bool on = false;
    double eps_primal = 1e-8, eps_dual = 1e-8;
};
// ... and what a verdict leaves: kind 1 (primal infeasible: y, z = -A^T y) or 2 (dual infeasible: d), the ray in the caller's
// units and numbering, scaled to infinity norm 1; objective = D(y) resp. c'd, violation = V(y) resp. W(d) of that ray
struct Certificate {
    int kind = 0, iter = 0;
    double objective = 0.0, violation = 0.0;
    std::vector<double> y, z, d;
};

// The sums an evaluation fetches (scaled units): c'x_bar, y_obj'y_bar, x_bar'z_bar, |Rd|^2, |Rp|^2 and, read at iteration 0
// only, the bound violation |x_bar - proj(x_bar)|^2 ...
struct ResidualSums {
    double cx, yobj_y, xz, rd2, rp2, lu2;
};
// ... and the LP's scaling they are mapped back with
struct ResidualScales {
    double b_scale, c_scale, norm_b_org, norm_c_org, obj_constant;
};

// reference compute_residuals (main_iterate.cu:229-309), host part: every field of *r but kkt, whose order of max() is the caller's
inline void assemble_residuals(Residuals *r, const ResidualSums &s, const ResidualScales &k, bool iter0) {
    const double obj_scale = k.b_scale * k.c_scale;
    r->primal_obj = obj_scale * s.cx + k.obj_constant;
    r->dual_obj = obj_scale * (s.yobj_y + s.xz) + k.obj_constant;
    r->rel_gap = std::abs(r->primal_obj - r->dual_obj) / (1.0 + std::abs(r->primal_obj) + std::abs(r->dual_obj));
    r->err_Rd = k.c_scale * std::sqrt(s.rd2) / k.norm_c_org;
    r->err_Rp = k.b_scale * std::sqrt(s.rp2) / k.norm_b_org;
    if (iter0) r->err_Rp = std::max(r->err_Rp, k.b_scale * std::sqrt(s.lu2));
}

// reference check_restart (main_iterate.cu:324-365) at a periodic evaluation: rs.flag 1 sufficient, 2 necessary, 3 long, 0 none
inline void check_restart(RestartState &rs, int iter, int check_iter, double sigma, bool verbose) {
    rs.flag = 0;
    if (rs.first) {
        if (iter == check_iter) { rs.first = false; rs.flag = 1; rs.best_gap = rs.current_gap; rs.best_sigma = sigma; }
    } else if (iter % check_iter == 0) {
        if (rs.current_gap < 0) {
            rs.current_gap = 1e-6;
            if (verbose) std::cout << "current_gap < 0" << std::endl;
        }
        if (rs.current_gap <= 0.2 * rs.last_gap) rs.flag = 1;
        if (rs.current_gap <= 0.6 * rs.last_gap && rs.current_gap > 1.00 * rs.save_gap) rs.flag = 2;
        if (rs.inner >= 0.2 * iter) rs.flag = 3;
        if (rs.best_gap > rs.current_gap) { rs.best_gap = rs.current_gap; rs.best_sigma = sigma; }
        rs.save_gap = rs.current_gap;
    }
}

// reference update_sigma (main_iterate.cu:367-404): the sigma a restart sets, from the norms of x_bar - last_x and y_bar - last_y;
// 1 where either movement is outside (1e-16, 1e12)
inline double restart_sigma(double primal_move, double dual_move, double lambda_max, const RestartState &rs, const Residuals &r) {
    if (!(primal_move > 1e-16 && dual_move > 1e-16 && primal_move < 1e12 && dual_move < 1e12)) return 1.0;
    const double ratio = (primal_move / dual_move) / std::sqrt(lambda_max);
    const double fact = std::exp(-0.05 * (rs.current_gap / rs.best_gap));
    const double temp1 = std::max(std::min(r.err_Rd, r.err_Rp), std::min(r.rel_gap, rs.current_gap));
    const double sigma_cand = std::exp(fact * std::log(ratio) + (1 - fact) * std::log(rs.best_sigma));
    const double kappa = temp1 > 9e-10   ? 1.0
                         : temp1 > 5e-10 ? std::max(std::min(std::sqrt(r.err_Rd / r.err_Rp), 100.0), 1e-2)
                                         : std::max(std::min(r.err_Rd / r.err_Rp, 100.0), 1e-2);
    return kappa * sigma_cand;
}

// The detection's ratio-test sums at an evaluation (scaled iterates, caller's units): D(y) and V(y) of the dual ray y, c'd and
// W(d) of the primal ray d, and the rays' infinity norms
struct RayScalars {
    double D = 0, V = 0, cd = 0, W = 0, yn = 1, dn = 1;
    int verdict(const Detection &det) const {  // 1 primal infeasible, 2 dual infeasible, 0 neither
        if (D > 0.0 && V <= det.eps_primal * D) return 1;  // (NaN fails both tests)
        if (cd < 0.0 && W <= det.eps_dual * -cd) return 2;
        return 0;
    }
};

// A verdict's certificate, whose arrays hold the ray in scaled units (kind 1: y and A^T y in y and z; kind 2: d), into the
// caller's units as k_unscale maps y_bar, z_bar and x_bar (rn / cn: row / column scaling), scaled to infinity norm 1, with its
// kind, iteration, objective and violation.  The numbering is left as it is.
inline void finish_certificate(Certificate *c, int kind, int iter, const RayScalars &s, const double *rn, const double *cn,
                               double b_scale, double c_scale) {
    c->kind = kind;
    c->iter = iter;
    if (kind == 1) {
        for (size_t i = 0; i < c->y.size(); ++i) c->y[i] = ((c->y[i] / rn[i]) * c_scale) / s.yn;
        for (size_t j = 0; j < c->z.size(); ++j) c->z[j] = -((c->z[j] * cn[j]) * c_scale) / s.yn;
        c->objective = s.D / s.yn;
        c->violation = s.V / s.yn;
    } else {
        for (size_t j = 0; j < c->d.size(); ++j) c->d[j] = ((c->d[j] / cn[j]) * b_scale) / s.dn;
        c->objective = s.cd / s.dn;
        c->violation = s.W / s.dn;
    }
}

}  // namespace hprlp
