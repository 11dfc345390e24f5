// K7: the OCP Microscaling (MX) Q/DQ pair — blocks of 32 elements along one axis share a power-of-two scale (E8M0), the elements
// are FP8 E4M3 (MXFP8) or FP4 E2M1 (MXFP4).  y = round_elem(v / 2^se) * 2^se with se from the block's largest |v|
// (tests/mx_model.py is the definition; mx_format.hpp the arithmetic, on bit patterns).  The tensor is [outer, K, inner], blocks
// along K.  One read and one write per element (8 B), non-temporal; no atomics, no LDS, no scratch; 64-bit element indices.
//   inner == 1  k_fake_quant_mx_rows: blocks are contiguous.  A group of 32 / VEC lanes holds one block, VEC elements per lane —
//               16-byte vectors (VEC = 4, 8 lanes per block) when both bases are 16-byte aligned and K % 4 == 0, else element by
//               element (VEC = 1, 32 lanes per block).  The block maximum is taken on the bit patterns of |v| by log2(32 / VEC)
//               cross-lane steps inside the group.  Every row takes ceil(K / 32) groups: the lanes past a short last block are
//               masked (they read nothing, contribute 0 to the maximum and write nothing).
//   inner > 1   k_fake_quant_mx_cols: blocks are strided by `inner`.  A lane owns VEC adjacent columns (4 when inner % 4 == 0
//               and the bases are aligned, else 1) of one block and walks its 32 rows — each load is coalesced across the lanes —
//               keeping the 32 * VEC values in registers between the maximum and the rounding.
//   GIVEN (--mx_scale_search: dpl_fake_quant_mx_scaled; tests/mx_scale_model.py) either kernel reads the block's E8M0 byte from
//   `scales` instead of deriving and writing it; the block maximum is still taken, for the non-finite rule (mx_block_se_given).
#include "mx_block.hpp"

namespace {

// ---------------------------------------------------------------------------------------------- inner == 1
// (groups: MxRowsAt, mx_block.hpp)
// (GIVEN: `scales` is READ, one byte per block in the order it is otherwise written in)
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kBlock) void k_fake_quant_mx_rows(const float* x, float* y, uint64_t n_groups, uint32_t K, uint32_t nblk,
                                                               uint8_t* scales) {
    const MxRowsAt<VEC> w(nblk);
    MxVec<VEC> v[kMxRowsIter];
    uint64_t at[kMxRowsIter];
    bool live[kMxRowsIter];
    uint32_t byte[kMxRowsIter];
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        uint64_t row;
        uint32_t col;
        w.at(i, nblk, row, col);
        live[i] = w.group(i) < n_groups && col < K;    // (K % VEC == 0: a vector that starts inside a row ends inside it)
        at[i] = row * K + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[i].b[j] = 0u;
        if (live[i]) v[i] = mx_load<VEC>(x + at[i]);
        byte[i] = 0u;
        if constexpr (GIVEN)
            if (live[i]) byte[i] = ((gptr_u8)scales)[w.group(i)];
    }
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t a = mx_group_max<VEC>(v[i]);
        bool nan;
        const int se = GIVEN ? mx_block_se_given<ELEM>(a, byte[i], nan) : mx_block_se<ELEM>(a, nan);
        if (live[i]) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[i].b[j] = mx_elem<ELEM>(v[i].b[j], se, nan);
            mx_store<VEC>(y + at[i], v[i]);
            if (!GIVEN && scales != nullptr && w.lane == 0u)     // (lane 0 of a group with any live lane is live: col = blk * 32 < K)
                ((gptr_u8w)scales)[w.group(i)] = nan ? 0xFFu : (uint8_t)(se + 127);
        }
    }
}

// ---------------------------------------------------------------------------------------------- inner > 1
// (slots: MxColsAt, mx_block.hpp)
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_fake_quant_mx_cols(const float* x, float* y, uint64_t n_slots, uint32_t K, uint32_t nblk,
                                                                     uint32_t inner, uint32_t cs, uint8_t* scales) {
    if ((uint64_t)blockIdx.x * kMxColsBlock + threadIdx.x >= n_slots) return;
    const MxColsAt w(nblk, cs, VEC);
    const uint64_t o = w.o;
    const uint32_t kb = w.kb, col = w.col;
    const uint32_t rows = min(32u, K - kb * 32u);
    const uint64_t base = (o * K + (uint64_t)kb * 32u) * inner + col;
    MxVec<VEC> v[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[r].b[j] = 0u;
        if ((uint32_t)r < rows) v[r] = mx_load<VEC>(x + base + (uint64_t)r * inner);
    }
    uint32_t a[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) a[j] = 0u;
#pragma unroll
    for (int r = 0; r < 32; ++r)
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[j] = max(a[j], v[r].b[j] & 0x7FFFFFFFu);
    int se[VEC];
    bool nan[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        if constexpr (GIVEN)
            se[j] = mx_block_se_given<ELEM>(a[j], ((gptr_u8)scales)[(o * nblk + kb) * inner + col + (uint32_t)j], nan[j]);
        else
            se[j] = mx_block_se<ELEM>(a[j], nan[j]);
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if ((uint32_t)r < rows) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[r].b[j] = mx_elem<ELEM>(v[r].b[j], se[j], nan[j]);
            mx_store<VEC>(y + base + (uint64_t)r * inner, v[r]);
        }
    }
    if constexpr (GIVEN) return;
    if (scales != nullptr) {
        const uint64_t sb = (o * nblk + kb) * inner + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) ((gptr_u8w)scales)[sb + j] = nan[j] ? 0xFFu : (uint8_t)(se[j] + 127);
    }
}

template <int ELEM, bool GIVEN = false>
int fake_quant_mx_launch(const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales, dpl_stream_t s) {
    const char* too_large = GIVEN ? "dpl_fake_quant_mx_scaled: tensor too large" : "dpl_fake_quant_mx: tensor too large";
    const uint32_t K = (uint32_t)k, nblk = (K + 31u) / 32u;
    const bool aligned = ((((uintptr_t)d_x | (uintptr_t)d_y) & 15u) == 0u);
    if (inner == 1) {
        const uint64_t n_groups = outer * nblk;
        const bool vec = aligned && (K & 3u) == 0u;
        const uint64_t per_wg = (uint64_t)kMxRowsIter * kBlock * (vec ? 4 : 1) / 32;
        const uint64_t blocks = (n_groups + per_wg - 1) / per_wg;
        if (blocks > 0x7FFFFFFFull) return fail_msg(too_large);
        if (vec)
            hipLaunchKernelGGL((k_fake_quant_mx_rows<ELEM, 4, GIVEN>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups, K,
                               nblk, d_scales);
        else
            hipLaunchKernelGGL((k_fake_quant_mx_rows<ELEM, 1, GIVEN>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups, K,
                               nblk, d_scales);
        DPL_LAUNCH_CHECK("k_fake_quant_mx_rows");
        return 0;
    }
    const bool vec = aligned && (inner & 3u) == 0u;
    const uint32_t cs = (uint32_t)(vec ? inner / 4 : inner);
    const uint64_t n_slots = outer * nblk * cs;
    const uint64_t blocks = (n_slots + kMxColsBlock - 1) / kMxColsBlock;
    if (blocks > 0x7FFFFFFFull) return fail_msg(too_large);
    if (vec)
        hipLaunchKernelGGL((k_fake_quant_mx_cols<ELEM, 4, GIVEN>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_y, n_slots, K,
                           nblk, (uint32_t)inner, cs, d_scales);
    else
        hipLaunchKernelGGL((k_fake_quant_mx_cols<ELEM, 1, GIVEN>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_y, n_slots, K,
                           nblk, (uint32_t)inner, cs, d_scales);
    DPL_LAUNCH_CHECK("k_fake_quant_mx_cols");
    return 0;
}

}  // namespace

extern "C" int dpl_fake_quant_mx(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                                 uint8_t* d_scales_or_null, dpl_stream_t s) {
    if (elem != DPL_MX_E4M3 && elem != DPL_MX_E2M1) return fail_msg("dpl_fake_quant_mx: elem must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (outer == 0 || k == 0 || inner == 0) return 0;
    if (d_x == nullptr || d_y == nullptr) return fail_msg("dpl_fake_quant_mx: d_x and d_y must not be null");
    if (k > 0x7FFFFFFFull || inner > 0x7FFFFFFFull) return fail_msg("dpl_fake_quant_mx: k and inner must be in [1, 2^31)");
    if (outer > (0x7FFFFFFFFFFFFFFFull / k) / inner) return fail_msg("dpl_fake_quant_mx: tensor too large");
    return elem == DPL_MX_E4M3 ? fake_quant_mx_launch<DPL_MX_E4M3>(d_x, d_y, outer, k, inner, d_scales_or_null, s)
                               : fake_quant_mx_launch<DPL_MX_E2M1>(d_x, d_y, outer, k, inner, d_scales_or_null, s);
}

extern "C" int dpl_fake_quant_mx_scaled(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                                        const uint8_t* d_scales, dpl_stream_t s) {
    if (elem != DPL_MX_E4M3 && elem != DPL_MX_E2M1) return fail_msg("dpl_fake_quant_mx_scaled: elem must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (outer == 0 || k == 0 || inner == 0) return 0;
    if (d_x == nullptr || d_y == nullptr || d_scales == nullptr) return fail_msg("dpl_fake_quant_mx_scaled: d_x, d_y and d_scales must not be null");
    if (k > 0x7FFFFFFFull || inner > 0x7FFFFFFFull) return fail_msg("dpl_fake_quant_mx_scaled: k and inner must be in [1, 2^31)");
    if (outer > (0x7FFFFFFFFFFFFFFFull / k) / inner) return fail_msg("dpl_fake_quant_mx_scaled: tensor too large");
    uint8_t* given = const_cast<uint8_t*>(d_scales);      // (read only: the GIVEN kernels never store through it)
    return elem == DPL_MX_E4M3 ? fake_quant_mx_launch<DPL_MX_E4M3, true>(d_x, d_y, outer, k, inner, given, s)
                               : fake_quant_mx_launch<DPL_MX_E2M1, true>(d_x, d_y, outer, k, inner, given, s);
}
