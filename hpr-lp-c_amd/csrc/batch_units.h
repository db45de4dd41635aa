// batch_units.h -- the maps between the caller's units and the scaled units of solve_batched, per element, and the per-member
// scalar rules, stated once for the host loops of batch_prep.cpp and the kernels of batched.hip.  Every entry of the batched solver
// agrees with every other to the bit because all of them call these; the order of the operations is part of the result:
// (v * cn) / b_scale is not v * (cn / b_scale).  Plain host code under a host compiler: no HIP header, no HIP call.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define HPRLP_HOST_DEVICE __host__ __device__
#else
#define HPRLP_HOST_DEVICE
#endif

namespace hprlp {

constexpr double kInfReplacement = 1.0e100;  // reference batched_solver.cu:17

// b_i = max(|AL_i|, |AU_i|), an infinite side counting 0.  A NaN lower side: the host keeps it (std::max's rule), the device's fmax
// drops it (DESIGN.md "Device-resident batches"); every other input gives the same bits on both.
HPRLP_HOST_DEVICE inline double bound_value(double lo, double hi) {
    const double a = (std::isinf(lo) && lo < 0) ? 0.0 : std::fabs(lo);
    const double b = (std::isinf(hi) && hi > 0) ? 0.0 : std::fabs(hi);
#ifdef __HIP_DEVICE_COMPILE__
    return fmax(a, b);
#else
    return a < b ? b : a;
#endif
}

// ---- a member's data into scaled units (reference batched_solver.cu:792-885) -------------------------------------------------------
// first step, by the shared matrix' norms: the cost c / cn and the row sides AL, AU / rn ...
HPRLP_HOST_DEVICE inline double over_norm(double v, double norm) { return v / norm; }
// ... and the bounds l, u * cn
HPRLP_HOST_DEVICE inline double times_norm(double v, double norm) { return v * norm; }
// second step, by the member's scale: the cost / c_scale; row sides and bounds / b_scale.  (Without use_bc_scaling the host skips
// this step and the kernels divide by 1.0, which is exact.)
HPRLP_HOST_DEVICE inline double by_scale(double v, double scale) { return v / scale; }
// last, and only after the norms of the scaled values are taken: an infinite lower side or bound, an infinite upper one
HPRLP_HOST_DEVICE inline double lower_replaced(double v) { return (std::isinf(v) && v < 0) ? -kInfReplacement : v; }
HPRLP_HOST_DEVICE inline double upper_replaced(double v) { return (std::isinf(v) && v > 0) ? kInfReplacement : v; }

// ---- points -------------------------------------------------------------------------------------------------------------------
// a start: X0 -> (x * cn) / b_scale[k], Y0 -> (y * rn) / c_scale[k]
HPRLP_HOST_DEVICE inline double start_to_scaled(double x, double norm, double scale) { return by_scale(times_norm(x, norm), scale); }
// a solution: x = (X / cn) * b_scale[k], y = (Y / rn) * c_scale[k] ...
HPRLP_HOST_DEVICE inline double point_to_caller(double p, double norm, double scale) { return over_norm(p, norm) * scale; }
// ... and z = (Z * cn) * c_scale[k]
HPRLP_HOST_DEVICE inline double reduced_cost_to_caller(double p, double norm, double scale) { return times_norm(p, norm) * scale; }

// ---- per-member scalars, from a sum of squares `total` (batch_prep.h: the norm rules) -------------------------------------------
// b_scale, c_scale, norm_b_org, norm_c_org
HPRLP_HOST_DEVICE inline double one_plus_norm(double total) { return 1.0 + std::sqrt(total); }
// the first sigma: norm_b / norm_c where both exceed 1e-8, else 1
HPRLP_HOST_DEVICE inline double first_sigma(double nb, double nc) { return (nb > 1.0e-8 && nc > 1.0e-8) ? nb / nc : 1.0; }

}  // namespace hprlp
