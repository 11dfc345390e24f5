// K7c: `--mx_scale_search` — per block of a constant MX operand, whichever of the floor-rule shared exponent se0 and se0 + 1 gives
// the smaller squared Q/DQ error (tests/mx_scale_model.py is the definition; mx_search.hpp the arithmetic, which also compiles for
// the host; mx_block.hpp the block walk — MxRowsLoad, MxColsLoad — and the block maximum shared with the Q/DQ pair; mx_plan.hpp
// the argument check, the launch plan and the dispatch).  The tensor is fp32
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
// (a lane past a short block's end holds +0.0: it adds 0 to either sum)
template <int ELEM, int VEC>
__global__ __launch_bounds__(kBlock) void k_mx_scale_search_rows(const float* x, uint64_t n_groups, uint32_t K, uint32_t nblk, uint8_t* scales,
                                                                 double* err) {
    MxRowsLoad<VEC> in(n_groups, K, nblk);
    in.load(x);
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t a = mx_group_max<VEC>(in.v[i]);
        bool nan;
        int se0, se1;
        mx_candidates<ELEM>(a, nan, se0, se1);
        double t0[VEC], t1[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double d = dpl_mx::f32_bits_to_f64(in.v[i].b[j]);
            t0[j] = dpl_mx::elem_sq_err<ELEM>(in.v[i].b[j], d, se0);
            t1[j] = dpl_mx::elem_sq_err<ELEM>(in.v[i].b[j], d, se1);
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
        if (in.first(i)) mx_store_choice(scales, err, in.group(i), mx_choose(nan, se0, e0, e1));
    }
}

// ---------------------------------------------------------------------------------------------- inner > 1
template <int ELEM, int VEC>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_mx_scale_search_cols(const float* x, uint64_t n_slots, uint32_t K, uint32_t nblk, uint32_t inner,
                                                                       uint32_t cs, uint8_t* scales, double* err) {
    const MxColsAt<VEC> w(n_slots, nblk, cs);
    if (!w.live) return;
    MxColsLoad<VEC> in(w, K, inner);
    in.load(x);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        bool nan;
        int se0, se1;
        mx_candidates<ELEM>(MX_COL_MAX(in, j), nan, se0, se1);
        dpl_mx::TreeSum t0, t1;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const double d = dpl_mx::f32_bits_to_f64(in.v[r].b[j]);
            t0.push(dpl_mx::elem_sq_err<ELEM>(in.v[r].b[j], d, se0), (uint32_t)r);
            t1.push(dpl_mx::elem_sq_err<ELEM>(in.v[r].b[j], d, se1), (uint32_t)r);
        }
        mx_store_choice(scales, err, w.block(nblk, inner, j), mx_choose(nan, se0, t0.level[5], t1.level[5]));
    }
}

}  // namespace

extern "C" int dpl_mx_scale_search(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_scales,
                                   double* d_err_or_null, dpl_stream_t s) {
    const char* who = "dpl_mx_scale_search";
    int rc;
    if (mx_check(rc, who, elem, "d_x and d_scales", {d_x, d_scales}, outer, k, inner, false, nullptr)) return rc;
    MxPlan p;
    if ((rc = mx_plan(p, who, (uintptr_t)d_x, outer, k, inner, false)) != 0) return rc;
    return mx_dispatch_all(elem, inner == 1, p.vec, [&](auto E, auto ROWS, auto VEC) {
        if constexpr (ROWS) {
            hipLaunchKernelGGL((k_mx_scale_search_rows<E, VEC>), dim3((unsigned)p.blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, p.n, p.K, p.nblk,
                               d_scales, d_err_or_null);
            DPL_LAUNCH_CHECK("k_mx_scale_search_rows");
        } else {
            hipLaunchKernelGGL((k_mx_scale_search_cols<E, VEC>), dim3((unsigned)p.blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, p.n, p.K, p.nblk,
                               (uint32_t)inner, p.cs, d_scales, d_err_or_null);
            DPL_LAUNCH_CHECK("k_mx_scale_search_cols");
        }
        return 0;
    });
}
