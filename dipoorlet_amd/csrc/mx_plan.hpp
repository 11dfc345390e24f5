// HOST side of the MX block kernels (mx_kernels.hip, mx_pack_kernels.hip, mx_search_kernels.hip), defined once — pure arithmetic, no
// HIP: the argument check of their entry points (mx_check), the launch plan of an fp32 [outer, K, inner] tensor in blocks of 32
// along K (mx_plan), and the way from (elem, inner == 1, vec) to a kernel instantiation (mx_dispatch, mx_dispatch_all).  And of the two kernels on the
// block-scaled MFMA (mx_gemm_kernels.hip, mx_conv_kernels.hip): what they hold a pair of packed operands to (mx_pair_elems,
// mx_pair_null, mx_pair_aligned), their grid of 64 x 64 tiles (mx_tiles), each entry point's rules in their order (mx_gemm_check,
// mx_gemm_err_check, mx_conv_check) and the way from (elem_a, elem_b) to an instantiation (mx_pair_dispatch, mx_pair_dispatch_all).  A wrong value here is an out-of-range
// address in a kernel, so a plain C++ compiler can build this: tests/mx_plan_host.cpp is a stand-alone program that runs it under
// the address and undefined-behaviour sanitizers (tests/test_mx_plan_host.py).
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

// The element formats there are: the two of mx_dispatch and the two FP6 formats mx_dispatch_all adds (2 .. 5 are no formats).
inline bool mx_known(int32_t elem) { return elem == DPL_MX_E4M3 || elem == DPL_MX_E2M1 || elem == DPL_MX_E2M3 || elem == DPL_MX_E3M2; }

// The argument rules of every entry point, in their order: elem, a zero size, null pointers, k and inner in [1, 2^31), a tensor
// whose elements 64-bit indices reach, the codes' alignment.  -> true: the call is over and rc its result (0: nothing to do).
//   names / ptrs  the pointers that must not be null, and what the message calls them;
//   padded        the bound holds for the padded tensor, 32 * nblk <= k + 31 along K (the packed forms index it), not the plain one;
//   codes         null, or the codes' base, which must be 16-byte aligned.
inline bool mx_check(int& rc, const char* who, int32_t elem, const char* names, std::initializer_list<const void*> ptrs, uint64_t outer,
                     uint64_t k, uint64_t inner, bool padded, const void* codes) {
    rc = 0;
    if (!mx_known(elem)) return (rc = mx_fail(who, "elem must be DPL_MX_E4M3 or DPL_MX_E2M1 (or DPL_MX_E2M3 / DPL_MX_E3M2)")), true;
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

// f(e, rows, VEC) for one element type e (a std::integral_constant), rows and VEC as such constants too: what both dispatches below
// do once they know the format.
template <class E, class F>
inline int mx_dispatch_elem(E e, bool rows, bool vec, F f) {
    const auto by_vec = [&](auto r) { return vec ? f(e, r, std::integral_constant<int, 4>{}) : f(e, r, std::integral_constant<int, 1>{}); };
    return rows ? by_vec(std::true_type{}) : by_vec(std::false_type{});
}

// f(element type, rows, VEC) with the three as std::integral_constant values: one instantiation of a kernel family per call.
template <class F>
inline int mx_dispatch(int32_t elem, bool rows, bool vec, F f) {
    return elem == DPL_MX_E4M3 ? mx_dispatch_elem(std::integral_constant<int, DPL_MX_E4M3>{}, rows, vec, f)
                               : mx_dispatch_elem(std::integral_constant<int, DPL_MX_E2M1>{}, rows, vec, f);
}

// The same over all four formats: the two FP6 formats are taken here, E4M3 and E2M1 go on to mx_dispatch.  What the entry points call.
template <class F>
inline int mx_dispatch_all(int32_t elem, bool rows, bool vec, F f) {
    if (elem == DPL_MX_E2M3) return mx_dispatch_elem(std::integral_constant<int, DPL_MX_E2M3>{}, rows, vec, f);
    if (elem == DPL_MX_E3M2) return mx_dispatch_elem(std::integral_constant<int, DPL_MX_E3M2>{}, rows, vec, f);
    return mx_dispatch(elem, rows, vec, f);
}

// ---- The two kernels on the block-scaled MFMA (mx_gemm_kernels.hip, mx_conv_kernels.hip; their device side is mx_mfma.hpp) ----

constexpr uint32_t kMxGemmTile = 64;      // rows and columns of C per workgroup

// What both entry points are given: two packed operands' element types, codes and scales, and C.
struct MxPair {
    int32_t elem_a, elem_b;
    const uint8_t *a_codes, *a_scales, *b_codes, *b_scales;
    float* c;
};

// The three rules both entry points hold the pair to, each -> 0 or the refusal (they stand apart: what lies between them differs).
inline int mx_pair_elems(const char* who, const MxPair& o) {
    return mx_known(o.elem_a) && mx_known(o.elem_b) ? 0
                                                    : mx_fail(who, "elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1 (or DPL_MX_E2M3 / DPL_MX_E3M2)");
}
// dpl_mx_gemm_err's: --mx_mixed chooses between E2M1 and E4M3, and its kernel is instantiated for those two (mx_pair_dispatch).
inline int mx_pair_elems_mixed(const char* who, const MxPair& o) {
    const auto known = [](int32_t e) { return e == DPL_MX_E4M3 || e == DPL_MX_E2M1; };
    return known(o.elem_a) && known(o.elem_b)
               ? 0
               : mx_fail(who, "elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1 (--mx_mixed chooses between these two: no FP6 format here)");
}
inline bool mx_pair_operands(const MxPair& o) {
    return o.a_codes != nullptr && o.a_scales != nullptr && o.b_codes != nullptr && o.b_scales != nullptr;
}
inline int mx_pair_null(const char* who, const MxPair& o) {
    return mx_pair_operands(o) && o.c != nullptr ? 0 : mx_fail(who, "the codes, the scales and d_c must not be null");
}
inline int mx_pair_aligned(const char* who, const MxPair& o) {
    if ((((uintptr_t)o.a_codes | (uintptr_t)o.b_codes) & 15u) == 0u) return 0;
    return mx_fail(who, "d_a_codes and d_b_codes must be 16-byte aligned (a block's codes are loaded as 16-byte vectors)");
}

// The grid of a [batch, m, n] product, m and n in [1, 2^31): a workgroup per 64 x 64 tile of C.
struct MxTiles {
    uint32_t tiles_m, tiles_n;
    uint64_t blocks;
};

// -> 0, or the refusal ("tensor too large" and more) of a grid above 2^31 - 1 workgroups.
inline int mx_tiles(MxTiles& t, const char* who, uint64_t batch, uint64_t m, uint64_t n, const char* more = "") {
    t.tiles_m = (uint32_t)((m + kMxGemmTile - 1) / kMxGemmTile);
    t.tiles_n = (uint32_t)((n + kMxGemmTile - 1) / kMxGemmTile);
    const uint64_t per_batch = (uint64_t)t.tiles_m * t.tiles_n;
    t.blocks = 0;
    if (per_batch > 0x7FFFFFFFull || batch > 0x7FFFFFFFull / per_batch) return mx_fail(who, "tensor too large", more);
    t.blocks = batch * per_batch;
    return 0;
}

// The sizes of a [batch, m, k] x [.., n, k] product, none of them 0 -> 0 or the refusal: m, n and k in range, and the padded
// operands, 32 * ceil(k / 32) <= k + 31 codes a row, and the [batch, m, n] array (C, or the reference) indexable.
inline int mx_gemm_sizes(const char* who, uint64_t batch, uint64_t m, uint64_t n, uint64_t k) {
    if (m > 0x7FFFFFFFull || n > 0x7FFFFFFFull || k > 0x7FFFFFFFull) return mx_fail(who, "m, n and k must be in [1, 2^31)");
    const uint64_t kp = 32ull * ((k + 31u) / 32u), big = m > n ? m : n;
    if (batch > (0x7FFFFFFFFFFFFFFFull / kp) / big || batch > (0x7FFFFFFFFFFFFFFFull / m) / n) return mx_fail(who, "tensor too large");
    return 0;
}

// dpl_mx_gemm's argument rules in their order.  -> true: the call is over and rc its result (0: nothing to do).
inline bool mx_gemm_check(int& rc, MxTiles& t, const MxPair& o, uint64_t batch, uint64_t m, uint64_t n, uint64_t k) {
    const char* who = "dpl_mx_gemm";
    if ((rc = mx_pair_elems(who, o)) != 0 || batch == 0 || m == 0 || n == 0 || k == 0 || (rc = mx_pair_null(who, o)) != 0) return true;
    return (rc = mx_gemm_sizes(who, batch, m, n, k)) != 0 || (rc = mx_pair_aligned(who, o)) != 0 || (rc = mx_tiles(t, who, batch, m, n)) != 0;
}

// dpl_mx_gemm_err's: dpl_mx_gemm's with the reference and the partial sums where that has C (o.c is not looked at).  The partial
// sums, two doubles a workgroup, are indexable wherever the grid is.
inline bool mx_gemm_err_check(int& rc, MxTiles& t, const MxPair& o, const float* ref, const double* part, uint64_t batch, uint64_t m, uint64_t n,
                              uint64_t k) {
    const char* who = "dpl_mx_gemm_err";
    if ((rc = mx_pair_elems_mixed(who, o)) != 0 || batch == 0 || m == 0 || n == 0 || k == 0) return true;
    if (!mx_pair_operands(o) || ref == nullptr || part == nullptr)
        return (rc = mx_fail(who, "the codes, the scales, d_ref and d_part must not be null")), true;
    return (rc = mx_gemm_sizes(who, batch, m, n, k)) != 0 || (rc = mx_pair_aligned(who, o)) != 0 || (rc = mx_tiles(t, who, batch, m, n)) != 0;
}

// acc *= f unless that passes limit
inline bool mx_mul(uint64_t& acc, uint64_t f, uint64_t limit) {
    if (f != 0 && acc > limit / f) return false;
    acc *= f;
    return true;
}

struct MxConvDims {
    int64_t n, h, w, c, cout, kh, kw, stride_h, stride_w, pad_top, pad_left, dil_h, dil_w, oh, ow;
};

struct MxConvPlan {
    uint64_t cb, nblk, m;     // channel blocks of 32, the K-blocks kh * kw * cb of a weight row, the output pixels oh * ow of an image
    MxTiles t;
};

// dpl_mx_conv's argument rules in their order.  -> true: the call is over and rc its result (0: nothing to do).
inline bool mx_conv_check(int& rc, MxConvPlan& p, const MxPair& o, const MxConvDims& d) {
    const char* who = "dpl_mx_conv";
    if ((rc = mx_pair_elems(who, o)) != 0) return true;
    if (d.kh < 1 || d.kw < 1 || d.stride_h < 1 || d.stride_w < 1 || d.dil_h < 1 || d.dil_w < 1)
        return (rc = mx_fail(who, "kh, kw, the strides and the dilations must be at least 1")), true;
    if (d.pad_top < 0 || d.pad_left < 0) return (rc = mx_fail(who, "pad_top and pad_left must not be negative")), true;
    for (int64_t v : {d.n, d.h, d.w, d.c, d.cout, d.kh, d.kw, d.stride_h, d.stride_w, d.pad_top, d.pad_left, d.dil_h, d.dil_w, d.oh, d.ow})
        if (v < 0 || v > 0x7FFFFFFFll) return (rc = mx_fail(who, "every dimension, stride, pad and dilation must be in [0, 2^31)")), true;
    if (d.n == 0 || d.h == 0 || d.w == 0 || d.c == 0 || d.cout == 0 || d.oh == 0 || d.ow == 0 || (rc = mx_pair_null(who, o)) != 0) return true;
    // (the K-blocks of a weight row and the output pixels of an image are 32-bit in the kernel; both operands' codes, at most 32
    // bytes a block, and C must be indexable)
    const uint64_t big = 0x7FFFFFFFFFFFFFFFull;
    uint64_t a_bytes = 32u, b_bytes = 32u, c_bytes = 4u;
    p.cb = ((uint64_t)d.c + 31u) / 32u, p.nblk = (uint64_t)d.kh, p.m = (uint64_t)d.oh;
    const bool fits = mx_mul(p.nblk, (uint64_t)d.kw, 0x7FFFFFFFull) && mx_mul(p.nblk, p.cb, 0x7FFFFFFFull) && mx_mul(p.m, (uint64_t)d.ow, 0x7FFFFFFFull) &&
                      mx_mul(a_bytes, (uint64_t)d.n, big) && mx_mul(a_bytes, (uint64_t)d.h, big) && mx_mul(a_bytes, (uint64_t)d.w, big) &&
                      mx_mul(a_bytes, p.cb, big) && mx_mul(b_bytes, (uint64_t)d.cout, big) && mx_mul(b_bytes, p.nblk, big) &&
                      mx_mul(c_bytes, (uint64_t)d.n, big) && mx_mul(c_bytes, p.m, big) && mx_mul(c_bytes, (uint64_t)d.cout, big);
    if (!fits) return (rc = mx_fail(who, "tensor too large")), true;
    return (rc = mx_tiles(p.t, who, (uint64_t)d.n, p.m, (uint64_t)d.cout, " (the grid)")) != 0 || (rc = mx_pair_aligned(who, o)) != 0;
}

// f(A's element type, B's) with the two as std::integral_constant values: one instantiation of k_mx_gemm or k_mx_conv per call.
template <class F>
inline int mx_pair_dispatch(const MxPair& o, F f) {
    const auto by_b = [&](auto ea) {
        return o.elem_b == DPL_MX_E4M3 ? f(ea, std::integral_constant<int, DPL_MX_E4M3>{}) : f(ea, std::integral_constant<int, DPL_MX_E2M1>{});
    };
    return o.elem_a == DPL_MX_E4M3 ? by_b(std::integral_constant<int, DPL_MX_E4M3>{}) : by_b(std::integral_constant<int, DPL_MX_E2M1>{});
}

// The same over all sixteen pairs of the four formats: a pair of E4M3 / E2M1 goes on to mx_pair_dispatch, a pair with an FP6 format
// on either side is taken here.  What dpl_mx_gemm and dpl_mx_conv call (dpl_mx_gemm_err stays with mx_pair_dispatch).
template <class F>
inline int mx_pair_dispatch_all(const MxPair& o, F f) {
    const auto old = [](int32_t e) { return e == DPL_MX_E4M3 || e == DPL_MX_E2M1; };
    if (old(o.elem_a) && old(o.elem_b)) return mx_pair_dispatch(o, f);
    const auto by_elem = [](int32_t e, auto g) {
        return e == DPL_MX_E4M3   ? g(std::integral_constant<int, DPL_MX_E4M3>{})
               : e == DPL_MX_E2M1 ? g(std::integral_constant<int, DPL_MX_E2M1>{})
               : e == DPL_MX_E2M3 ? g(std::integral_constant<int, DPL_MX_E2M3>{})
                                  : g(std::integral_constant<int, DPL_MX_E3M2>{});
    };
    return by_elem(o.elem_a, [&](auto ea) { return by_elem(o.elem_b, [&](auto eb) { return f(ea, eb); }); });
}

}  // namespace
