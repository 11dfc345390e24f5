// K7: the OCP Microscaling (MX) Q/DQ pair — blocks of 32 elements along one axis share a power-of-two scale (E8M0), the elements
// are FP8 E4M3 (MXFP8), FP6 E2M3 or E3M2 (the two MXFP6: tests/mx_fp6_model.py) or FP4 E2M1 (MXFP4).  y = round_elem(v / 2^se) * 2^se with se from the block's largest |v|
// (tests/mx_model.py is the definition; mx_format.hpp the arithmetic, on bit patterns).  The tensor is [outer, K, inner], blocks
// along K.  One read and one write per element (8 B), non-temporal; no atomics, no LDS, no scratch; 64-bit element indices.
// The block walk is mx_block.hpp's (MxRowsLoad, MxColsLoad), the argument check, launch plan and dispatch mx_plan.hpp's: a kernel
// here is "load; per block: maximum, exponent, round and store".
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
// (GIVEN: `scales` is READ, one byte per block in the order it is otherwise written in — by the live lanes only)
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kBlock) void k_fake_quant_mx_rows(const float* x, float* y, uint64_t n_groups, uint32_t K, uint32_t nblk,
                                                               uint8_t* scales) {
    MxRowsLoad<VEC> in(n_groups, K, nblk);
    in.load(x);
    uint32_t byte[kMxRowsIter];
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) byte[i] = in.template given_byte<GIVEN>(scales, i, in.live[i]);
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t a = mx_group_max<VEC>(in.v[i]);
        bool nan;
        const int se = GIVEN ? mx_block_se_given<ELEM>(a, byte[i], nan) : mx_block_se<ELEM>(a, nan);
        if (in.live[i]) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) in.v[i].b[j] = mx_elem<ELEM>(in.v[i].b[j], se, nan);
            mx_store<VEC>(y + in.at[i], in.v[i]);
            if (!GIVEN && scales != nullptr && in.first(i)) ((gptr_u8w)scales)[in.group(i)] = mx_scale_byte(se, nan);
        }
    }
}

// ---------------------------------------------------------------------------------------------- inner > 1
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_fake_quant_mx_cols(const float* x, float* y, uint64_t n_slots, uint32_t K, uint32_t nblk,
                                                                     uint32_t inner, uint32_t cs, uint8_t* scales) {
    const MxColsAt<VEC> w(n_slots, nblk, cs);
    if (!w.live) return;
    MxColsLoad<VEC> in(w, K, inner);
    in.load(x);
    int se[VEC];
    bool nan[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const uint32_t a = MX_COL_MAX(in, j);
        if constexpr (GIVEN)
            se[j] = mx_block_se_given<ELEM>(a, ((gptr_u8)scales)[w.block(nblk, inner, j)], nan[j]);
        else
            se[j] = mx_block_se<ELEM>(a, nan[j]);
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if (in.has(r)) {               // (rounded in place: into a second vector, the compiler folds the maxima into the guarded loads
#pragma unroll                         //  above and waits for each load where it is issued)
            for (int j = 0; j < VEC; ++j) in.v[r].b[j] = mx_elem<ELEM>(in.v[r].b[j], se[j], nan[j]);
            mx_store<VEC>(y + in.at(r), in.v[r]);
        }
    }
    if constexpr (GIVEN) return;
    if (scales != nullptr) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) ((gptr_u8w)scales)[w.block(nblk, inner, j)] = mx_scale_byte(se[j], nan[j]);
    }
}

template <bool GIVEN>
int fake_quant_mx_launch(const char* who, int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales,
                         dpl_stream_t s) {
    MxPlan p;
    if (const int rc = mx_plan(p, who, (uintptr_t)d_x | (uintptr_t)d_y, outer, k, inner, false)) return rc;
    return mx_dispatch_all(elem, inner == 1, p.vec, [&](auto E, auto ROWS, auto VEC) {
        if constexpr (ROWS) {
            hipLaunchKernelGGL((k_fake_quant_mx_rows<E, VEC, GIVEN>), dim3((unsigned)p.blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, p.n, p.K,
                               p.nblk, d_scales);
            DPL_LAUNCH_CHECK("k_fake_quant_mx_rows");
        } else {
            hipLaunchKernelGGL((k_fake_quant_mx_cols<E, VEC, GIVEN>), dim3((unsigned)p.blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_y, p.n,
                               p.K, p.nblk, (uint32_t)inner, p.cs, d_scales);
            DPL_LAUNCH_CHECK("k_fake_quant_mx_cols");
        }
        return 0;
    });
}

}  // namespace

extern "C" int dpl_fake_quant_mx(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                                 uint8_t* d_scales_or_null, dpl_stream_t s) {
    int rc;
    if (mx_check(rc, "dpl_fake_quant_mx", elem, "d_x and d_y", {d_x, d_y}, outer, k, inner, false, nullptr)) return rc;
    return fake_quant_mx_launch<false>("dpl_fake_quant_mx", elem, d_x, d_y, outer, k, inner, d_scales_or_null, s);
}

extern "C" int dpl_fake_quant_mx_scaled(int32_t elem, const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner,
                                        const uint8_t* d_scales, dpl_stream_t s) {
    int rc;
    if (mx_check(rc, "dpl_fake_quant_mx_scaled", elem, "d_x, d_y and d_scales", {d_x, d_y, d_scales}, outer, k, inner, false, nullptr)) return rc;
    uint8_t* given = const_cast<uint8_t*>(d_scales);      // (read only: the GIVEN kernels never store through it)
    return fake_quant_mx_launch<true>("dpl_fake_quant_mx_scaled", elem, d_x, d_y, outer, k, inner, given, s);
}
