// K7c: `--mx_verify` — the product of two packed MX operands on CDNA4's block-scaled matrix instruction (tests/mx_gemm_model.py is
// the definition; DESIGN.md §3o the lane map as confirmed on the hardware and the measurements).  Both operands are K-INNERMOST,
// exactly as dpl_mx_encode writes them: A codes [batch, m, Kp * bits / 8] and scales [batch, m, Kp / 32], B codes
// [batch or 1, n, Kp * bits / 8] and scales [.., n, Kp / 32], Kp = 32 * ceil(k / 32);  C[b, i, j] = sum over kk < Kp of
// a[b, i, kk] * b[b or 0, j, kk], fp32 [batch, m, n].  The pad codes take part in the sum (the encoder writes 0).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16 x 128 by a 128 x 16 tile.  Lane l supplies, of either operand, row (column)
// l & 15, and as its scale the E8M0 byte of K-block l >> 4 of the 128-wide step.  Its codes (confirmed with exact
// data): E2M1 — the 32 K values of that same block, 16 bytes, byte j holding k = 2j in its low and k = 2j + 1 in its high nibble,
// the file's order; the other four dwords of the operand are 0.  E4M3 — NOT that block: dwords 0 .. 3 are k = 16 (l >> 4) .. + 15
// of the step and dwords 4 .. 7 k = 64 + 16 (l >> 4) .. + 15, byte j of a run being k = j, while a K-block of 32 is still scaled by
// the byte of lane group block-number.  So a lane's fragment is one (E2M1) or two (E4M3, 64 bytes apart) 16-byte loads straight
// from the file's order, and the four lanes of a row read one run of 64 bytes or two.  C/D: lane l holds column l & 15, rows
// 4 * (l >> 4) + reg.
//
//   k_mx_gemm<EA, EB>  256 threads, a 64 x 64 tile of C per workgroup; each wave owns 32 x 32 of it as 2 x 2 instruction tiles,
//                      four accumulators.  Operands come straight from global memory (L2), no LDS.  Rows >= m, columns >= n and
//                      the K-blocks past Kp / 32 of the last step are masked: nothing is loaded or stored outside the arrays, a
//                      masked lane supplies a zero fragment and scale byte 127.
// The NaN rule is the kernel's own, whatever the instruction does with such bytes: a lane notes a 0xFF scale byte or an E4M3 NaN
// code (0x7F, 0xFF) in what it loads, the four lanes of a row combine their notes after the K loop, and every C of that row of A
// (column of C for B) is stored as NaN.  No atomics, 64-bit indices.
#include "mx_mfma.hpp"      // the fragment of an operand tile: GemmFrag, gemm_load

namespace {

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_gemm(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                    float* c, uint32_t m, uint32_t n, uint32_t nblk, uint32_t tiles_m, uint32_t tiles_n,
                                                    uint32_t b_batched) {
#if defined(__HIP_DEVICE_COMPILE__)
    using f4v = __attribute__((ext_vector_type(4))) float;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_batch = tiles_m * tiles_n;                       // (the grid is below 2^31)
    const uint32_t bi = blockIdx.x / per_batch, t = blockIdx.x - bi * per_batch;
    const uint32_t tm = t / tiles_n, tn = t - tm * tiles_n;
    const uint64_t row0 = (uint64_t)tm * kMxGemmTile + (wave >> 1) * 32u, col0 = (uint64_t)tn * kMxGemmTile + (wave & 1u) * 32u;
    const uint32_t r16 = lane & 15u, q = lane >> 4;

    uint64_t a_row[2], b_row[2];
    bool a_live[2], b_live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint64_t r = row0 + 16u * i + r16, cc = col0 + 16u * i + r16;
        a_live[i] = r < m;
        b_live[i] = cc < n;
        a_row[i] = (uint64_t)bi * m + r;
        b_row[i] = (b_batched ? (uint64_t)bi * n : 0ull) + cc;
    }
    f4v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t a_bad[2] = {0u, 0u}, b_bad[2] = {0u, 0u};

    for (uint32_t kb0 = 0; kb0 < nblk; kb0 += 4u) {
        GemmFrag fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = gemm_load<EA>(a_codes, a_scales, a_row[i], nblk, kb0, q, a_live[i], a_bad[i]);
            fb[i] = gemm_load<EB>(b_codes, b_scales, b_row[i], nblk, kb0, q, b_live[i], b_bad[i]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i].v, fb[j].v, acc[i][j], GemmOperand<EA>::fmt, GemmOperand<EB>::fmt, 0,
                                                                             fa[i].scale, 0, fb[j].scale);
    }

    // the notes of the four lanes of a row (column); every lane of the wave is here
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        a_bad[i] |= (uint32_t)__shfl_xor((int)a_bad[i], 16, kWave);
        a_bad[i] |= (uint32_t)__shfl_xor((int)a_bad[i], 32, kWave);
        b_bad[i] |= (uint32_t)__shfl_xor((int)b_bad[i], 16, kWave);
        b_bad[i] |= (uint32_t)__shfl_xor((int)b_bad[i], 32, kWave);
    }
    // C/D: lane l holds column l & 15 and rows 4 * (l >> 4) + reg of its 16 x 16 tile; row r's note sits in lanes r, r + 16, ...
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint32_t rr = 4u * q + (uint32_t)reg;
            const uint32_t row_bad = (uint32_t)__shfl((int)a_bad[i], (int)rr, kWave);
            const uint64_t r = row0 + 16u * i + rr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint64_t cc = col0 + 16u * j + r16;
                if (r < m && cc < n) {
                    const float v = (row_bad | b_bad[j]) ? __uint_as_float(0x7FC00000u) : acc[i][j][reg];
                    ((gptr_f32g)c)[((uint64_t)bi * m + r) * n + cc] = v;
                }
            }
        }
    }
#endif
}

template <int EA, int EB>
int mx_gemm_launch(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales, uint64_t batch, uint64_t m,
                   uint64_t n, uint64_t k, int32_t b_batched, float* c, dpl_stream_t s) {
    const uint64_t tiles_m = (m + kMxGemmTile - 1) / kMxGemmTile, tiles_n = (n + kMxGemmTile - 1) / kMxGemmTile;
    if (tiles_m * tiles_n > 0x7FFFFFFFull || batch > 0x7FFFFFFFull / (tiles_m * tiles_n)) return fail_msg("dpl_mx_gemm: tensor too large");
    const uint32_t nblk = (uint32_t)((k + 31u) / 32u);
    hipLaunchKernelGGL((k_mx_gemm<EA, EB>), dim3((unsigned)(batch * tiles_m * tiles_n)), dim3(kBlock), 0, (hipStream_t)s, a_codes, a_scales, b_codes,
                       b_scales, c, (uint32_t)m, (uint32_t)n, nblk, (uint32_t)tiles_m, (uint32_t)tiles_n, (uint32_t)(b_batched != 0));
    DPL_LAUNCH_CHECK("k_mx_gemm");
    return 0;
}

}  // namespace

extern "C" int dpl_mx_gemm(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                           const uint8_t* d_b_scales, uint64_t batch, uint64_t m, uint64_t n, uint64_t k, int32_t b_batched, float* d_c,
                           dpl_stream_t s) {
    if ((elem_a != DPL_MX_E4M3 && elem_a != DPL_MX_E2M1) || (elem_b != DPL_MX_E4M3 && elem_b != DPL_MX_E2M1))
        return fail_msg("dpl_mx_gemm: elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (batch == 0 || m == 0 || n == 0 || k == 0) return 0;
    if (d_a_codes == nullptr || d_a_scales == nullptr || d_b_codes == nullptr || d_b_scales == nullptr || d_c == nullptr)
        return fail_msg("dpl_mx_gemm: the codes, the scales and d_c must not be null");
    if (m > 0x7FFFFFFFull || n > 0x7FFFFFFFull || k > 0x7FFFFFFFull) return fail_msg("dpl_mx_gemm: m, n and k must be in [1, 2^31)");
    // (the padded operands, 32 * ceil(k / 32) <= k + 31 codes a row, and C must be indexable)
    const uint64_t kp = 32ull * ((k + 31u) / 32u), big = m > n ? m : n;
    if (batch > (0x7FFFFFFFFFFFFFFFull / kp) / big || batch > (0x7FFFFFFFFFFFFFFFull / m) / n) return fail_msg("dpl_mx_gemm: tensor too large");
    if ((((uintptr_t)d_a_codes | (uintptr_t)d_b_codes) & 15u) != 0u)
        return fail_msg("dpl_mx_gemm: d_a_codes and d_b_codes must be 16-byte aligned (a block's codes are loaded as 16-byte vectors)");
    const int pair = (elem_a == DPL_MX_E2M1 ? 2 : 0) | (elem_b == DPL_MX_E2M1 ? 1 : 0);
    switch (pair) {
    case 0: return mx_gemm_launch<DPL_MX_E4M3, DPL_MX_E4M3>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, batch, m, n, k, b_batched, d_c, s);
    case 1: return mx_gemm_launch<DPL_MX_E4M3, DPL_MX_E2M1>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, batch, m, n, k, b_batched, d_c, s);
    case 2: return mx_gemm_launch<DPL_MX_E2M1, DPL_MX_E4M3>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, batch, m, n, k, b_batched, d_c, s);
    default: return mx_gemm_launch<DPL_MX_E2M1, DPL_MX_E2M1>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, batch, m, n, k, b_batched, d_c, s);
    }
}
