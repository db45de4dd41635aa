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

}  // namespace hprlp
