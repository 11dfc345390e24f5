// HOST side of the MX block kernels (mx_kernels.hip, mx_pack_kernels.hip, mx_search_kernels.hip), defined once — pure arithmetic, no
// HIP: the argument check of their entry points (mx_check), the launch plan of an fp32 [outer, K, inner] tensor in blocks of 32
// along K (mx_plan), and the way from (elem, inner == 1, vec) to a kernel instantiation (mx_dispatch).  A wrong value here is an
// out-of-range address in a kernel, so a plain C++ compiler can build this: tests/mx_plan_host.cpp is a stand-alone program that
// runs it under the address and undefined-behaviour sanitizers (tests/test_mx_plan_host.py).
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/dipoorlet_hip.h"
#include "host_error.hpp"

namespace {

constexpr int kMxRowsBlock = 256;     // threads per workgroup of the rows kernels (common.hpp kBlock)
constexpr int kMxRowsIter = 4;        // groups per lane group of the rows kernels (all loads issued before the first use)
constexpr int kMxColsBlock = 64;      // threads per workgroup of the cols kernels: one wave (no cross-lane traffic)

inline int mx_fail(const char* who, const char* what, const char* more = "") {
    snprintf(g_err, sizeof(g_err), "%s: %s%s", who, what, more);
    return -2;
}

// The argument rules of every entry point, in their order: elem, a zero size, null pointers, k and inner in [1, 2^31), a tensor
// whose elements 64-bit indices reach, the codes' alignment.  -> true: the call is over and rc its result (0: nothing to do).
//   names / ptrs  the pointers that must not be null, and what the message calls them;
//   padded        the bound holds for the padded tensor, 32 * nblk <= k + 31 along K (the packed forms index it), not the plain one;
//   codes         null, or the codes' base, which must be 16-byte aligned.
inline bool mx_check(int& rc, const char* who, int32_t elem, const char* names, std::initializer_list<const void*> ptrs, uint64_t outer,
                     uint64_t k, uint64_t inner, bool padded, const void* codes) {
    rc = 0;
    if (elem != DPL_MX_E4M3 && elem != DPL_MX_E2M1) return (rc = mx_fail(who, "elem must be DPL_MX_E4M3 or DPL_MX_E2M1")), true;
    if (outer == 0 || k == 0 || inner == 0) return true;
    for (const void* p : ptrs)
        if (p == nullptr) return (rc = mx_fail(who, names, " must not be null")), true;
    if (k > 0x7FFFFFFFull || inner > 0x7FFFFFFFull) return (rc = mx_fail(who, "k and inner must be in [1, 2^31)")), true;
    if (outer > (0x7FFFFFFFFFFFFFFFull / (padded ? 32ull * ((k + 31u) / 32u) : k)) / inner) return (rc = mx_fail(who, "tensor too large")), true;
    if (((uintptr_t)codes & 15u) != 0u)
        return (rc = mx_fail(who, "d_codes must be 16-byte aligned (a block's codes are stored and loaded as 16-byte vectors)")), true;
    return false;
}

struct MxPlan {
    uint32_t K, nblk, cs;     // cs: column groups of a row (inner / VEC; 1 for inner == 1)
    bool vec;                 // 16-byte vectors (VEC = 4) or single elements (VEC = 1)
    uint64_t n, blocks;       // groups (inner == 1) or slots, and workgroups
};

// The launch of a checked (mx_check) tensor.  -> 0, or the refusal of a grid above 2^31 - 1 workgroups.
//   fp     the OR of the fp32 side's base addresses: 16-byte vectors need them aligned, and K (inner == 1) or inner a multiple of 4;
//   tiles  the VEC = 4 cols kernels take a workgroup per tile of 4 K-blocks x 16 column groups (MxPackColsAt, mx_block.hpp), not per
//          64 slots (MxColsAt).
inline int mx_plan(MxPlan& p, const char* who, uintptr_t fp, uint64_t outer, uint64_t k, uint64_t inner, bool tiles) {
    p.K = (uint32_t)k;
    p.nblk = (p.K + 31u) / 32u;
    p.vec = (fp & 15u) == 0u && ((inner == 1 ? k : inner) & 3u) == 0u;
    p.cs = inner == 1 ? 1u : (uint32_t)(p.vec ? inner / 4 : inner);
    p.n = outer * p.nblk * p.cs;
    const uint64_t per_wg = inner == 1 ? (uint64_t)kMxRowsIter * kMxRowsBlock * (p.vec ? 4 : 1) / 32 : kMxColsBlock;
    p.blocks = inner != 1 && p.vec && tiles ? outer * ((p.nblk + 3u) / 4u) * ((p.cs + 15u) / 16u) : (p.n + per_wg - 1) / per_wg;
    return p.blocks > 0x7FFFFFFFull ? mx_fail(who, "tensor too large") : 0;
}

// f(element type, rows, VEC) with the three as std::integral_constant values: one instantiation of a kernel family per call.
template <class F>
inline int mx_dispatch(int32_t elem, bool rows, bool vec, F f) {
    const auto by_vec = [&](auto e, auto r) { return vec ? f(e, r, std::integral_constant<int, 4>{}) : f(e, r, std::integral_constant<int, 1>{}); };
    const auto by_rows = [&](auto e) { return rows ? by_vec(e, std::true_type{}) : by_vec(e, std::false_type{}); };
    return elem == DPL_MX_E4M3 ? by_rows(std::integral_constant<int, DPL_MX_E4M3>{}) : by_rows(std::integral_constant<int, DPL_MX_E2M1>{});
}

}  // namespace
