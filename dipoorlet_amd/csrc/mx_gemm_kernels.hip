// K7c: `--mx_verify` — the product of two packed MX operands on CDNA4's block-scaled matrix instruction (tests/mx_gemm_model.py is
// the definition; DESIGN.md §3o the lane map as confirmed on the hardware and the measurements).  Both operands are K-INNERMOST,
// exactly as dpl_mx_encode writes them: A codes [batch, m, Kp * bits / 8] and scales [batch, m, Kp / 32], B codes
// [batch or 1, n, Kp * bits / 8] and scales [.., n, Kp / 32], Kp = 32 * ceil(k / 32);  C[b, i, j] = sum over kk < Kp of
// a[b, i, kk] * b[b or 0, j, kk], fp32 [batch, m, n].  The pad codes take part in the sum (the encoder writes 0).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16 x 128 by a 128 x 16 tile; which lane supplies what is mx_mfma.hpp's comment.
// A lane's fragment is one (E2M1) or two (E4M3, 64 bytes apart) 16-byte loads straight from the file's order, and the four lanes
// of a row read one run of 64 bytes or two.
//
//   k_mx_gemm<EA, EB>  mx_mfma_tile with plain K-innermost rows on both sides: 256 threads, a 64 x 64 tile of C per workgroup; each
//                      wave owns 32 x 32 of it as 2 x 2 instruction tiles, four accumulators.  Operands come straight from global
//                      memory (L2), no LDS.  Rows >= m, columns >= n and the K-blocks past Kp / 32 of the last step are masked:
//                      nothing is loaded or stored outside the arrays, a masked lane supplies a zero fragment and scale byte 127.
// The NaN rule is the kernel's own, whatever the instruction does with such bytes: a lane notes a 0xFF scale byte or an E4M3 NaN
// code (0x7F, 0xFF) in what it loads, the four lanes of a row combine their notes after the K loop, and every C of that row of A
// (column of C for B) is stored as NaN.  No atomics, 64-bit indices.
#include "mx_mfma.hpp"      // the fragment of an operand tile and the tile body: mx_frag_load, mx_mfma_tile

namespace {

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_gemm(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                    float* c, uint32_t m, uint32_t n, uint32_t nblk, uint32_t tiles_m, uint32_t tiles_n,
                                                    uint32_t b_batched) {
    mx_mfma_tile<EA, EB>(a_codes, a_scales, b_codes, b_scales, c, m, n, nblk, tiles_m, tiles_n, b_batched != 0u,
                         [=](uint32_t bi, uint64_t r) { return MxRowBlocks{((uint64_t)bi * m + r) * nblk, nblk, r < m}; });
}

}  // namespace

extern "C" int dpl_mx_gemm(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                           const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, float* d_c,
                           dpl_stream_t s) {
    const MxPair o = {elem_a, elem_b, d_a_codes, d_a_scales, d_b_codes, d_b_scales, d_c};
    int rc;
    MxTiles t;
    if (mx_gemm_check(rc, t, o, batch, m, n, k)) return rc;
    return mx_pair_dispatch(o, [&](auto EA, auto EB) {
        hipLaunchKernelGGL((k_mx_gemm<EA, EB>), dim3((unsigned)t.blocks), dim3(kBlock), 0, (hipStream_t)s, o.a_codes, o.a_scales, o.b_codes, o.b_scales,
                           o.c, (uint32_t)m, (uint32_t)n, (uint32_t)((k + 31u) / 32u), t.tiles_m, t.tiles_n, (uint32_t)(b_batched != 0));
        DPL_LAUNCH_CHECK("k_mx_gemm");
        return 0;
    });
}
