// K7c: `--mx_verify` — the product of two packed MX operands on CDNA4's block-scaled matrix instruction (tests/mx_gemm_model.py is
// the definition; DESIGN.md §3o the lane map as confirmed on the hardware and the measurements).  Both operands are K-INNERMOST,
// exactly as dpl_mx_encode writes them: A codes [batch, m, Kp * bits / 8] and scales [batch, m, Kp / 32], B codes
// [batch or 1, n, Kp * bits / 8] and scales [.., n, Kp / 32], Kp = 32 * ceil(k / 32);  C[b, i, j] = sum over kk < Kp of
// a[b, i, kk] * b[b or 0, j, kk], fp32 [batch, m, n].  The pad codes take part in the sum (the encoder writes 0).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16 x 128 by a 128 x 16 tile; which lane supplies what is mx_mfma.hpp's comment.
// A lane's fragment is one (E2M1) or two (E4M3, 64 bytes apart) 16-byte loads, or three 8-byte ones (E2M3 / E3M2: a 24-byte block),
// straight from the file's order, and the four lanes of a row read one run of 64 or 96 bytes, or two of 64.  k_mx_gemm is instantiated
// for all sixteen pairs of the four formats (mx_pair_dispatch_all), k_mx_gemm_err for the four of E4M3 / E2M1 (--mx_mixed's).
//
//   k_mx_gemm<EA, EB>  mx_mfma_tile with plain K-innermost rows on both sides: 256 threads, a 64 x 64 tile of C per workgroup; each
//                      wave owns 32 x 32 of it as 2 x 2 instruction tiles, four accumulators.  Operands come straight from global
//                      memory (L2), no LDS.  Rows >= m, columns >= n and the K-blocks past Kp / 32 of the last step are masked:
//                      nothing is loaded or stored outside the arrays, a masked lane supplies a zero fragment and scale byte 127.
// The NaN rule is the kernel's own, whatever the instruction does with such bytes: a lane notes a 0xFF scale byte or an E4M3 NaN
// code (0x7F, 0xFF) in what it loads, the four lanes of a row combine their notes after the K loop, and every C of that row of A
// (column of C for B) is stored as NaN.  No atomics, 64-bit indices.
//
// K7e: `--mx_mixed` — the same product held against a reference without ever being written (tests/mx_mixed_model.py
// gemm_err_partials is the definition; DESIGN.md §3u the summation order and the measurements).
//   k_mx_gemm_err<EA, EB>  k_mx_gemm's tile with another epilogue: per live element v of C, d = (v + bias[col]) - ref in fp32 (two
//                      roundings; no bias: v - ref), and the tile's sums of (double)d * d and (double)ref * ref — both squares
//                      exact in fp64 — go to part fp64 [batch * tiles_m * tiles_n, 2] in the grid's own tile order.  The order of
//                      the additions is fixed: a lane adds its 16 terms in the tile body's order (i, reg, j), a masked term being
//                      +0.0 (rows >= m and columns >= n of ref are not read); the 64 lane sums fold by xor-shuffles 1, 2, 4, 8, 16,
//                      32; the four wave sums go through LDS, and threads 0 and 1 store (w0 + w1) + (w2 + w3) of the first resp.
//                      the second sum.  Plain stores, no atomics: every workgroup writes its own row of part.
#include "mx_mfma.hpp"      // the fragment of an operand tile and the tile body: mx_frag_load, mx_mfma_tile

namespace {

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_gemm(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                    float* c, uint32_t m, uint32_t n, uint32_t nblk, uint32_t tiles_m, uint32_t tiles_n,
                                                    uint32_t b_batched) {
    mx_mfma_tile<EA, EB>(a_codes, a_scales, b_codes, b_scales, m, n, nblk, tiles_m, tiles_n, b_batched != 0u,
                         [=](uint32_t bi, uint64_t r) { return MxRowBlocks{((uint64_t)bi * m + r) * nblk, nblk, r < m}; }, MxStoreC{c, m, n});
}

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_gemm_err(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                        const float* ref, const float* bias, double* part, uint32_t m, uint32_t n, uint32_t nblk,
                                                        uint32_t tiles_m, uint32_t tiles_n, uint32_t b_batched) {
    double sum_d = 0.0, sum_r = 0.0;
    mx_mfma_tile<EA, EB>(a_codes, a_scales, b_codes, b_scales, m, n, nblk, tiles_m, tiles_n, b_batched != 0u,
                         [=](uint32_t bi, uint64_t r) { return MxRowBlocks{((uint64_t)bi * m + r) * nblk, nblk, r < m}; },
                         [&](uint32_t bi, uint64_t r, uint64_t cc, bool live, float v) {
                             double dd = 0.0, rr = 0.0;
                             if (live) {
                                 const float rf = ref[((uint64_t)bi * m + r) * n + cc];
                                 const float d = __fsub_rn(bias != nullptr ? __fadd_rn(v, bias[cc]) : v, rf);
                                 dd = (double)d * (double)d, rr = (double)rf * (double)rf;
                             }
                             sum_d += dd, sum_r += rr;
                         });
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        sum_d += __shfl_xor(sum_d, o, kWave);
        sum_r += __shfl_xor(sum_r, o, kWave);
    }
    __shared__ double waves[kBlock / kWave][2];
    if ((threadIdx.x & (kWave - 1)) == 0) waves[threadIdx.x / kWave][0] = sum_d, waves[threadIdx.x / kWave][1] = sum_r;
    __syncthreads();
    const uint32_t t = threadIdx.x;      // threads 0 and 1: the tile's two sums
    if (t < 2) part[2ull * blockIdx.x + t] = (waves[0][t] + waves[1][t]) + (waves[2][t] + waves[3][t]);
}

}  // namespace

extern "C" int dpl_mx_gemm_err(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                               const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, const float* d_ref,
                               const float* d_bias_or_null, double* d_part, dpl_stream_t s) {
    const MxPair o = {elem_a, elem_b, d_a_codes, d_a_scales, d_b_codes, d_b_scales, nullptr};
    int rc;
    MxTiles t;
    if (mx_gemm_err_check(rc, t, o, d_ref, d_part, batch, m, n, k)) return rc;
    return mx_pair_dispatch(o, [&](auto EA, auto EB) {
        hipLaunchKernelGGL((k_mx_gemm_err<EA, EB>), dim3((unsigned)t.blocks), dim3(kBlock), 0, (hipStream_t)s, o.a_codes, o.a_scales, o.b_codes, o.b_scales,
                           d_ref, d_bias_or_null, d_part, (uint32_t)m, (uint32_t)n, (uint32_t)((k + 31u) / 32u), t.tiles_m, t.tiles_n,
                           (uint32_t)(b_batched != 0));
        DPL_LAUNCH_CHECK("k_mx_gemm_err");
        return 0;
    });
}

extern "C" int dpl_mx_gemm(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                           const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, float* d_c,
                           dpl_stream_t s) {
    const MxPair o = {elem_a, elem_b, d_a_codes, d_a_scales, d_b_codes, d_b_scales, d_c};
    int rc;
    MxTiles t;
    if (mx_gemm_check(rc, t, o, batch, m, n, k)) return rc;
    return mx_pair_dispatch_all(o, [&](auto EA, auto EB) {
        hipLaunchKernelGGL((k_mx_gemm<EA, EB>), dim3((unsigned)t.blocks), dim3(kBlock), 0, (hipStream_t)s, o.a_codes, o.a_scales, o.b_codes, o.b_scales,
                           o.c, (uint32_t)m, (uint32_t)n, (uint32_t)((k + 31u) / 32u), t.tiles_m, t.tiles_n, (uint32_t)(b_batched != 0));
        DPL_LAUNCH_CHECK("k_mx_gemm");
        return 0;
    });
}
