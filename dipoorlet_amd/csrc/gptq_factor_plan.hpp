// HOST side of the device factorisation (gptq_factor_kernels.hip), defined once — pure arithmetic, no HIP: the argument rules of
// dpl_gptq_factor / dpl_gptq_factor_phase in their order (gf_check), and the plan of a checked call (gf_plan): the padded size, where
// the three parts of the workspace begin, and the grid of every launch of a block step.  A wrong value here is an out-of-range
// address in a kernel, so a plain C++ compiler can build this.
#pragma once
#include <stdint.h>

#include "../../include/dipoorlet_hip.h"
#include "host_error.hpp"

namespace {

constexpr int kGfB = 64;      // block size: rows and columns of a tile, columns of a panel

// The workspace, in doubles from its base: P H' P / L [kp, kp] at 0, X [kp, kp] at x, the diagonal blocks' inverses [nb, 64, 64] at linv.
struct GfPlan {
    uint32_t k, nb;           // nb = ceil(k / 64) block steps
    uint64_t kp, x, linv, bytes;
    // Block step kb < nb.  Cholesky: one k_gf_diag, then below() k_gf_panel and lower(below()) k_gf_syrk workgroups (none at the last
    // step).  Inverse: kb + 1 k_gf_inv_row workgroups, then a (kb + 1) x below() grid of k_gf_inv_update.
    uint32_t below(uint32_t kb) const { return nb - kb - 1; }
    static uint32_t lower(uint32_t m) { return m * (m + 1) / 2; }      // tiles on and below the diagonal of m x m: nb <= 256, so < 2^16
};

inline GfPlan gf_plan(int64_t k) {      // 1 <= k <= DPL_GPTQ_FACTOR_MAX_K
    GfPlan p;
    p.k = (uint32_t)k;
    p.nb = (p.k + kGfB - 1) / kGfB;
    p.kp = (uint64_t)p.nb * kGfB;
    p.x = p.kp * p.kp;
    p.linv = 2 * p.x;
    p.bytes = (p.linv + p.kp * kGfB) * sizeof(double);
    return p;
}

// -> 0, or the refusal (-2, nothing launched).  phases: 1 the Cholesky factorisation, 2 the inverse, 3 both.
inline int gf_check(const void* d_h, int64_t k, double damp, const void* d_u, const void* d_status, const void* d_workspace,
                    uint64_t workspace_bytes, int32_t phases) {
    if (d_h == nullptr || d_u == nullptr || d_status == nullptr || d_workspace == nullptr) return fail_msg("dpl_gptq_factor: null pointer");
    if (k < 1 || k > DPL_GPTQ_FACTOR_MAX_K) return fail_msg("dpl_gptq_factor: k must be in [1, 16384]");
    if (!(damp > 0.0)) return fail_msg("dpl_gptq_factor: damp must be positive");      // (a NaN too)
    if (workspace_bytes < gf_plan(k).bytes) return fail_msg("dpl_gptq_factor: the workspace is smaller than dpl_gptq_factor_workspace(k)");
    if (phases < 1 || phases > 3) return fail_msg("dpl_gptq_factor_phase: phases must be 1 (Cholesky), 2 (inverse) or 3 (both)");
    return 0;
}

}  // namespace
