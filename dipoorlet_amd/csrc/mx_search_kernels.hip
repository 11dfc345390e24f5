// K7c: `--mx_scale_search` — per block of a constant MX operand, whichever of the floor-rule shared exponent se0 and se0 + 1 gives
// the smaller squared Q/DQ error (tests/mx_scale_model.py is the definition; mx_search.hpp the arithmetic, which also compiles for
// the host; mx_block.hpp the loads, the block maximum and the decompositions shared with the Q/DQ pair).  The tensor is fp32
// [outer, K, inner], blocks of 32 along K.  One read of x; per block one byte stored ([outer, nblk, inner], the order of
// dpl_fake_quant_mx's scales) and optionally two fp64 values, the error at the floor and at the chosen byte ([outer, nblk, inner, 2]).
// No atomics, no LDS, no scratch; 64-bit element indices; masked lanes read and write nothing.
// The error of a block is the fp64 sum of its 32 squared differences as a balanced tree in index order — e = e[0::2] + e[1::2] five
// times — which is what every form below computes: a lane's own VEC terms first, then xor-shuffle steps 1, 2, 4, .. across the
// lanes of the group (fp64 addition commutes bit for bit, so both lanes of a pair hold the same sum), or all five levels in one
// lane's registers.  The library is built with -ffp-contract=off and without fast-math: the tree is neither contracted nor
// reassociated.  Every fp64 operand is built from bit patterns (mx_search.hpp f32_bits_to_f64): no result depends on the fp32
// denormal mode.
//   inner == 1  k_mx_scale_search_rows: the lane groups of k_fake_quant_mx_rows (VEC = 4: 8 lanes a block, 16-byte loads when the
//               base is 16-byte aligned and K % 4 == 0; VEC = 1: 32 lanes).  Lane 0 of a group stores.
//   inner > 1   k_mx_scale_search_cols: the slots of k_fake_quant_mx_cols; a lane owns VEC adjacent columns of one block, keeps its
//               32 rows in registers between the maximum and the two roundings, and stores its columns' bytes and errors.
#include "mx_block.hpp"

namespace {

typedef __attribute__((address_space(1))) double* gptr_f64w;

// The chosen byte and the two errors from the block's maximum pattern and its two error sums.
struct MxChoice {
    uint32_t byte;
    double floor_err, chosen_err;
};

template <int ELEM>
__device__ __forceinline__ void mx_candidates(uint32_t a, bool& nan, int& se0, int& se1) {
    se0 = mx_block_se<ELEM>(a, nan);
    se1 = dpl_mx::upper_candidate<ELEM>(se0);
}

__device__ __forceinline__ MxChoice mx_choose(bool nan, int se0, double e0, double e1) {
    const bool up = e1 < e0;          // (ties keep the floor; se1 == se0 at the format's limit: e1 == e0)
    const double inf = dpl_mx::f64_from_bits(dpl_mx::kF64InfBits);
    MxChoice c;
    c.byte = nan ? 0xFFu : (uint32_t)(se0 + 127) + (up ? 1u : 0u);
    c.floor_err = nan ? inf : e0;
    c.chosen_err = nan ? inf : (up ? e1 : e0);
    return c;
}

__device__ __forceinline__ void mx_store_choice(uint8_t* scales, double* err, uint64_t block, const MxChoice& c) {
    ((gptr_u8w)scales)[block] = (uint8_t)c.byte;
    if (err != nullptr) {
        ((gptr_f64w)err)[2 * block] = c.floor_err;
        ((gptr_f64w)err)[2 * block + 1] = c.chosen_err;
    }
}

// ---------------------------------------------------------------------------------------------- inner == 1
// (groups: MxRowsAt, mx_block.hpp)
template <int ELEM, int VEC>
__global__ __launch_bounds__(kBlock) void k_mx_scale_search_rows(const float* x, uint64_t n_groups, uint32_t K, uint32_t nblk, uint8_t* scales,
                                                                 double* err) {
    const MxRowsAt<VEC> w(nblk);
    MxVec<VEC> v[kMxRowsIter];
    bool live[kMxRowsIter];
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        uint64_t row;
        uint32_t col;
        w.at(i, nblk, row, col);
        live[i] = w.group(i) < n_groups && col < K;    // (K % VEC == 0: a vector that starts inside a row ends inside it)
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[i].b[j] = 0u;  // (+0.0 past a short block's end: it adds 0 to either sum)
        if (live[i]) v[i] = mx_load<VEC>(x + row * K + col);
    }
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t a = mx_group_max<VEC>(v[i]);
        bool nan;
        int se0, se1;
        mx_candidates<ELEM>(a, nan, se0, se1);
        double t0[VEC], t1[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double d = dpl_mx::f32_bits_to_f64(v[i].b[j]);
            t0[j] = dpl_mx::elem_sq_err<ELEM>(v[i].b[j], d, se0);
            t1[j] = dpl_mx::elem_sq_err<ELEM>(v[i].b[j], d, se1);
        }
        double e0, e1;
        if constexpr (VEC == 4) {
            e0 = (t0[0] + t0[1]) + (t0[2] + t0[3]);
            e1 = (t1[0] + t1[1]) + (t1[2] + t1[3]);
        } else {
            e0 = t0[0];
            e1 = t1[0];
        }
#pragma unroll
        for (uint32_t o = 1; o < 32u / VEC; o <<= 1) {
            e0 = e0 + __shfl_xor(e0, (int)o, kWave);
            e1 = e1 + __shfl_xor(e1, (int)o, kWave);
        }
        if (live[i] && w.lane == 0u)                   // (lane 0 of a group with any live lane is live: col = blk * 32 < K)
            mx_store_choice(scales, err, w.group(i), mx_choose(nan, se0, e0, e1));
    }
}

// ---------------------------------------------------------------------------------------------- inner > 1
// (slots: MxColsAt, mx_block.hpp)
template <int ELEM, int VEC>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_mx_scale_search_cols(const float* x, uint64_t n_slots, uint32_t K, uint32_t nblk, uint32_t inner,
                                                                       uint32_t cs, uint8_t* scales, double* err) {
    if ((uint64_t)blockIdx.x * kMxColsBlock + threadIdx.x >= n_slots) return;
    const MxColsAt w(nblk, cs, VEC);
    const uint32_t rows = min(32u, K - w.kb * 32u);
    const uint64_t base = (w.o * K + (uint64_t)w.kb * 32u) * inner + w.col;
    MxVec<VEC> v[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[r].b[j] = 0u;
        if ((uint32_t)r < rows) v[r] = mx_load<VEC>(x + base + (uint64_t)r * inner);
    }
    const uint64_t sb = (w.o * nblk + w.kb) * inner + w.col;      // of [outer, nblk, inner]
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        uint32_t a = 0u;
#pragma unroll
        for (int r = 0; r < 32; ++r) a = max(a, v[r].b[j] & 0x7FFFFFFFu);
        bool nan;
        int se0, se1;
        mx_candidates<ELEM>(a, nan, se0, se1);
        dpl_mx::TreeSum t0, t1;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const double d = dpl_mx::f32_bits_to_f64(v[r].b[j]);
            t0.push(dpl_mx::elem_sq_err<ELEM>(v[r].b[j], d, se0), (uint32_t)r);
            t1.push(dpl_mx::elem_sq_err<ELEM>(v[r].b[j], d, se1), (uint32_t)r);
        }
        mx_store_choice(scales, err, sb + (uint32_t)j, mx_choose(nan, se0, t0.level[5], t1.level[5]));
    }
}

template <int ELEM>
int mx_scale_search_launch(const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales, double* d_err, dpl_stream_t s) {
    const uint32_t K = (uint32_t)k, nblk = (K + 31u) / 32u;
    const bool aligned = ((uintptr_t)d_x & 15u) == 0u;
    if (inner == 1) {
        const uint64_t n_groups = outer * nblk;
        const bool vec = aligned && (K & 3u) == 0u;
        const uint64_t per_wg = (uint64_t)kMxRowsIter * kBlock * (vec ? 4 : 1) / 32;
        const uint64_t blocks = (n_groups + per_wg - 1) / per_wg;
        if (blocks > 0x7FFFFFFFull) return fail_msg("dpl_mx_scale_search: tensor too large");
        if (vec)
            hipLaunchKernelGGL((k_mx_scale_search_rows<ELEM, 4>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, n_groups, K, nblk,
                               d_scales, d_err);
        else
            hipLaunchKernelGGL((k_mx_scale_search_rows<ELEM, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, n_groups, K, nblk,
                               d_scales, d_err);
        DPL_LAUNCH_CHECK("k_mx_scale_search_rows");
        return 0;
    }
    const bool vec = aligned && (inner & 3u) == 0u;
    const uint32_t cs = (uint32_t)(vec ? inner / 4 : inner);
    const uint64_t n_slots = outer * nblk * cs;
    const uint64_t blocks = (n_slots + kMxColsBlock - 1) / kMxColsBlock;
    if (blocks > 0x7FFFFFFFull) return fail_msg("dpl_mx_scale_search: tensor too large");
    if (vec)
        hipLaunchKernelGGL((k_mx_scale_search_cols<ELEM, 4>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, n_slots, K, nblk,
                           (uint32_t)inner, cs, d_scales, d_err);
    else
        hipLaunchKernelGGL((k_mx_scale_search_cols<ELEM, 1>), dim3((unsigned)blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, n_slots, K, nblk,
                           (uint32_t)inner, cs, d_scales, d_err);
    DPL_LAUNCH_CHECK("k_mx_scale_search_cols");
    return 0;
}

}  // namespace

extern "C" int dpl_mx_scale_search(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales,
                                   double* d_err_or_null, dpl_stream_t s) {
    if (elem != DPL_MX_E4M3 && elem != DPL_MX_E2M1) return fail_msg("dpl_mx_scale_search: elem must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (outer == 0 || k == 0 || inner == 0) return 0;
    if (d_x == nullptr || d_scales == nullptr) return fail_msg("dpl_mx_scale_search: d_x and d_scales must not be null");
    if (k > 0x7FFFFFFFull || inner > 0x7FFFFFFFull) return fail_msg("dpl_mx_scale_search: k and inner must be in [1, 2^31)");
    if (outer > (0x7FFFFFFFFFFFFFFFull / k) / inner) return fail_msg("dpl_mx_scale_search: tensor too large");
    return elem == DPL_MX_E4M3 ? mx_scale_search_launch<DPL_MX_E4M3>(d_x, outer, k, inner, d_scales, d_err_or_null, s)
                               : mx_scale_search_launch<DPL_MX_E2M1>(d_x, outer, k, inner, d_scales, d_err_or_null, s);
}
