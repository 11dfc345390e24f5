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
#include "common.hpp"
#include "mx_format.hpp"

namespace {

typedef __attribute__((address_space(1))) float* gptr_f32w;
typedef __attribute__((address_space(1))) f4* gptr_f4w;
typedef __attribute__((address_space(1))) uint8_t* gptr_u8w;

constexpr uint32_t kQuietNaN = 0x7FC00000u;
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr int kMxRowsIter = 4;        // groups per lane group of k_fake_quant_mx_rows (all loads issued before the first use)
constexpr int kMxColsBlock = 64;      // threads per workgroup of k_fake_quant_mx_cols: one wave (no cross-lane traffic)

template <int VEC>
struct MxVec {
    uint32_t b[VEC];
};

template <int VEC>
__device__ __forceinline__ MxVec<VEC> mx_load(const float* p) {
    MxVec<VEC> r;
    if constexpr (VEC == 4) {
        const f4 v = __builtin_nontemporal_load((gptr_f4)p);
        r.b[0] = __float_as_uint(v.x);
        r.b[1] = __float_as_uint(v.y);
        r.b[2] = __float_as_uint(v.z);
        r.b[3] = __float_as_uint(v.w);
    } else {
        r.b[0] = __float_as_uint(__builtin_nontemporal_load((gptr_f32)p));
    }
    return r;
}

template <int VEC>
__device__ __forceinline__ void mx_store(float* p, const MxVec<VEC>& r) {
    if constexpr (VEC == 4) {
        const f4 v = {__uint_as_float(r.b[0]), __uint_as_float(r.b[1]), __uint_as_float(r.b[2]), __uint_as_float(r.b[3])};
        __builtin_nontemporal_store(v, (gptr_f4w)p);
    } else {
        __builtin_nontemporal_store(__uint_as_float(r.b[0]), (gptr_f32w)p);
    }
}

// One element of a block whose largest |v| has the pattern `a` (`nan`: a is NaN or inf — E8M0 0xFF: every element NaN).
template <int ELEM>
__device__ __forceinline__ uint32_t mx_elem(uint32_t vbits, int se, bool nan) {
    const uint32_t y = (vbits & 0x80000000u) | dpl_mx::round_bits<ELEM>(vbits & 0x7FFFFFFFu, se);
    return nan ? kQuietNaN : y;
}

// se and the NaN flag of a block from its maximum pattern; an all-zero block: se = -127 (its zeros come out with their signs)
template <int ELEM>
__device__ __forceinline__ int mx_block_se(uint32_t a, bool& nan) {
    nan = a >= kInfBits;
    return (nan || a == 0u) ? -127 : dpl_mx::shared_exponent<ELEM>(a);
}

// ---------------------------------------------------------------------------------------------- inner == 1
// Group g of the launch is block g % nblk of row g / nblk (nblk = ceil(K / 32)); a workgroup owns kMxRowsIter * 256 * VEC / 32
// consecutive groups.  The workgroup's first (row, block) comes from one 64-bit division on uniform values; a lane's own from a
// 32-bit one per group.
template <int ELEM, int VEC>
__global__ __launch_bounds__(kBlock) void k_fake_quant_mx_rows(const float* x, float* y, uint64_t n_groups, uint32_t K, uint32_t nblk,
                                                               uint8_t* scales) {
    constexpr uint32_t LPG = 32 / VEC;                 // lanes per group
    constexpr uint32_t GPI = kBlock / LPG;             // groups per iteration of the workgroup
    const uint32_t tid = threadIdx.x, lane = tid % LPG;
    const uint64_t g0 = (uint64_t)blockIdx.x * (GPI * kMxRowsIter);
    const uint64_t row0 = g0 / nblk;
    const uint32_t blk0 = (uint32_t)(g0 - row0 * nblk);
    MxVec<VEC> v[kMxRowsIter];
    uint64_t at[kMxRowsIter];
    bool live[kMxRowsIter];
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t gi = (uint32_t)i * GPI + tid / LPG;
        const uint32_t b = blk0 + gi, dr = b / nblk, blk = b - dr * nblk;
        const uint32_t col = blk * 32u + lane * VEC;
        live[i] = g0 + gi < n_groups && col < K;       // (K % VEC == 0: a vector that starts inside a row ends inside it)
        at[i] = (row0 + dr) * K + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[i].b[j] = 0u;
        if (live[i]) v[i] = mx_load<VEC>(x + at[i]);
    }
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        uint32_t a = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) a = max(a, v[i].b[j] & 0x7FFFFFFFu);
#pragma unroll
        for (uint32_t o = 1; o < LPG; o <<= 1) a = max(a, (uint32_t)__shfl_xor((int)a, (int)o, kWave));
        bool nan;
        const int se = mx_block_se<ELEM>(a, nan);
        if (live[i]) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[i].b[j] = mx_elem<ELEM>(v[i].b[j], se, nan);
            mx_store<VEC>(y + at[i], v[i]);
            if (scales != nullptr && lane == 0u)       // (lane 0 of a group with any live lane is live: col = blk * 32 < K)
                ((gptr_u8w)scales)[g0 + (uint32_t)i * GPI + tid / LPG] = nan ? 0xFFu : (uint8_t)(se + 127);
        }
    }
}

// ---------------------------------------------------------------------------------------------- inner > 1
// Slot t of the launch is column group t % cs (cs = inner / VEC) of block (t / cs) % nblk of outer slice t / (cs * nblk): adjacent
// lanes read adjacent columns of the same row.  The workgroup's first slot is decomposed once (64-bit, uniform), a lane's own with
// 32-bit divisions.
template <int ELEM, int VEC>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_fake_quant_mx_cols(const float* x, float* y, uint64_t n_slots, uint32_t K, uint32_t nblk,
                                                                     uint32_t inner, uint32_t cs, uint8_t* scales) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kMxColsBlock;
    if (t0 + threadIdx.x >= n_slots) return;
    const uint64_t r0 = t0 / cs;                       // (outer slice, block) of the workgroup's first slot, flattened
    const uint32_t c0 = (uint32_t)(t0 - r0 * cs);
    const uint64_t o0 = r0 / nblk;
    const uint32_t kb0 = (uint32_t)(r0 - o0 * nblk);
    const uint32_t c = c0 + threadIdx.x, dc = c / cs, col = (c - dc * cs) * VEC;
    const uint32_t kb1 = kb0 + dc, dk = kb1 / nblk, kb = kb1 - dk * nblk;
    const uint64_t o = o0 + dk;
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
    for (int j = 0; j < VEC; ++j) se[j] = mx_block_se<ELEM>(a[j], nan[j]);
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if ((uint32_t)r < rows) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[r].b[j] = mx_elem<ELEM>(v[r].b[j], se[j], nan[j]);
            mx_store<VEC>(y + base + (uint64_t)r * inner, v[r]);
        }
    }
    if (scales != nullptr) {
        const uint64_t sb = (o * nblk + kb) * inner + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) ((gptr_u8w)scales)[sb + j] = nan[j] ? 0xFFu : (uint8_t)(se[j] + 127);
    }
}

template <int ELEM>
int fake_quant_mx_launch(const float* d_x, float* d_y, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales, dpl_stream_t s) {
    const uint32_t K = (uint32_t)k, nblk = (K + 31u) / 32u;
    const bool aligned = ((((uintptr_t)d_x | (uintptr_t)d_y) & 15u) == 0u);
    if (inner == 1) {
        const uint64_t n_groups = outer * nblk;
        const bool vec = aligned && (K & 3u) == 0u;
        const uint64_t per_wg = (uint64_t)kMxRowsIter * kBlock * (vec ? 4 : 1) / 32;
        const uint64_t blocks = (n_groups + per_wg - 1) / per_wg;
        if (blocks > 0x7FFFFFFFull) return fail_msg("dpl_fake_quant_mx: tensor too large");
        if (vec)
            hipLaunchKernelGGL((k_fake_quant_mx_rows<ELEM, 4>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups, K,
                               nblk, d_scales);
        else
            hipLaunchKernelGGL((k_fake_quant_mx_rows<ELEM, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups, K,
                               nblk, d_scales);
        DPL_LAUNCH_CHECK("k_fake_quant_mx_rows");
        return 0;
    }
    const bool vec = aligned && (inner & 3u) == 0u;
    const uint32_t cs = (uint32_t)(vec ? inner / 4 : inner);
    const uint64_t n_slots = outer * nblk * cs;
    const uint64_t blocks = (n_slots + kMxColsBlock - 1) / kMxColsBlock;
    if (blocks > 0x7FFFFFFFull) return fail_msg("dpl_fake_quant_mx: tensor too large");
    if (vec)
        hipLaunchKernelGGL((k_fake_quant_mx_cols<ELEM, 4>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_y, n_slots, K,
                           nblk, (uint32_t)inner, cs, d_scales);
    else
        hipLaunchKernelGGL((k_fake_quant_mx_cols<ELEM, 1>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_y, n_slots, K,
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
