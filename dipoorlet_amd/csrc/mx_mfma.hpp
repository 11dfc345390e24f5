// The kernels on v_mfma_scale_f32_16x16x128_f8f6f4 (mx_gemm_kernels.hip: k_mx_gemm, k_mx_gemm_err; mx_conv_kernels.hip: k_mx_conv),
// defined once: a lane's fragment of a packed MX operand as dpl_mx_encode writes it (mx_frag_load) and the 64 x 64 tile of C a
// workgroup computes (mx_mfma_tile).  The kernels differ in how K-block kb of a row of A resolves to a block of the operand and in
// what becomes of a finished element of C (the epilogue: MxStoreC writes it, k_mx_gemm_err adds its error up), and state only that; the
// host side — argument checks, tile grid, dispatch — is mx_plan.hpp.  The lane map (confirmed with exact data): lane
// l supplies row (column) l & 15 and, as its scale, the E8M0 byte of K-block l >> 4 of the 128-wide step.  Codes: E2M1 — the 32 K
// values of that same block, 16 bytes, byte j holding k = 2j in its low and k = 2j + 1 in its high nibble, the other four dwords 0.
// E4M3 — NOT that block: dwords 0 .. 3 are k = 16 (l >> 4) .. + 15 of the step and dwords 4 .. 7 k = 64 + 16 (l >> 4) .. + 15, byte
// j of a run being k = j.  C/D: lane l holds column l & 15, rows 4 * (l >> 4) + reg.
// E2M3 / E3M2 (format codes 2 / 3; DESIGN.md §3v, confirmed with one-product outputs that use every bit of the codes) — as E2M1, the
// 32 K values of block l >> 4 under that block's scale byte: dwords 0 .. 5 are the block's 24 bytes as the file holds them, ONE
// little-endian string of 192 bits with k = i in bits [6 i, 6 i + 6), the other two dwords 0.  No repack: the file's order is the
// instruction's.  A 24-byte block lies at a multiple of 8 bytes, so it is loaded as three 8-byte vectors.
#pragma once
#include "common.hpp"
#include "mx_format.hpp"
#include "mx_plan.hpp"

namespace {

using i8v = __attribute__((ext_vector_type(8))) int;
using u4g = __attribute__((ext_vector_type(4))) uint32_t;
typedef const __attribute__((address_space(1))) u4g* gptr_u4g;
using u2g = __attribute__((ext_vector_type(2))) uint32_t;
typedef const __attribute__((address_space(1))) u2g* gptr_u2g;
typedef const __attribute__((address_space(1))) uint8_t* gptr_u8g;
typedef __attribute__((address_space(1))) float* gptr_f32g;

template <int ELEM>
struct GemmOperand {
    static constexpr uint32_t block_bytes = 4u * dpl_mx::Fmt<ELEM>::bits;          // of one K-block's codes in the file: 32, 16 or 24
    static constexpr int fmt = dpl_mx::Fmt<ELEM>::mfma;                            // the instruction's format code (cbsz / blgp)
};

// Does a dword hold an E4M3 NaN byte (0x7F or 0xFF)?  (t's bytes are at most 0x7F: adding 1 carries into bit 7 only from 0x7F.)
__device__ __forceinline__ uint32_t e4m3_nan_in(uint32_t w) {
    return (((w & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u);
}

// One lane's fragment of one operand tile.
struct GemmFrag {
    i8v v;
    int scale;
};

// A row resolves its K-blocks: at(kb, blk) -> is K-block kb of the row there?  blk: its index among the operand's blocks.
// This one is the plain K-innermost row (B in both kernels, A of the GEMM): blk0 = row * nblk, the row already offset by the batch.
struct MxRowBlocks {
    uint64_t blk0;
    uint32_t nblk;
    bool live;                                // the row exists
    __device__ __forceinline__ bool operator()(uint32_t kb, uint64_t& blk) const {
        blk = blk0 + kb;
        return live && kb < nblk;
    }
};

// kb0: the first K-block of the 128-wide step; q = lane >> 4.  By the map above: the scale byte of block kb0 + q; E2M1 — the 16
// bytes of that block; E2M3 / E3M2 — its 24 bytes; E4M3 — half q & 1 of block kb0 + (q >> 1) into the low four dwords and the same half of block
// kb0 + 2 + (q >> 1) into the high four.  A block that is not there leaves zeros (scale byte 127), and nothing is loaded for it.
// bad: the lane's NaN notes, a 0xFF scale byte or an E4M3 NaN code in what it loaded (an FP6 or E2M1 code is never one).
template <int ELEM, class At>
__device__ __forceinline__ GemmFrag mx_frag_load(const uint8_t* codes, const uint8_t* scales, const At& at, uint32_t kb0, uint32_t q, uint32_t& bad) {
    GemmFrag f;
    f.v = i8v{0, 0, 0, 0, 0, 0, 0, 0};
    f.scale = 127;
    uint64_t blk;
    if constexpr (ELEM == DPL_MX_E4M3) {
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
            if (at(kb0 + 2u * hi + (q >> 1), blk)) {
                const u4g w = *(gptr_u4g)(codes + blk * GemmOperand<ELEM>::block_bytes + (q & 1u) * 16u);
                f.v[4 * hi] = (int)w.x, f.v[4 * hi + 1] = (int)w.y, f.v[4 * hi + 2] = (int)w.z, f.v[4 * hi + 3] = (int)w.w;
                bad |= e4m3_nan_in(w.x) | e4m3_nan_in(w.y) | e4m3_nan_in(w.z) | e4m3_nan_in(w.w);
            }
    } else if constexpr (GemmOperand<ELEM>::block_bytes == 24u) {
        // (a 24-byte block lies at a multiple of 8, and the last one of an odd number ends 8 bytes short of a 16-byte boundary:
        // three 8-byte loads, nothing read past the block)
        if (at(kb0 + q, blk)) {
            gptr_u2g src = (gptr_u2g)(codes + blk * 24u);
            const u2g w0 = src[0], w1 = src[1], w2 = src[2];
            f.v[0] = (int)w0.x, f.v[1] = (int)w0.y, f.v[2] = (int)w1.x, f.v[3] = (int)w1.y, f.v[4] = (int)w2.x, f.v[5] = (int)w2.y;
        }
    } else if (at(kb0 + q, blk)) {
        const u4g w = *(gptr_u4g)(codes + blk * GemmOperand<ELEM>::block_bytes);
        f.v[0] = (int)w.x, f.v[1] = (int)w.y, f.v[2] = (int)w.z, f.v[3] = (int)w.w;
    }
    if (at(kb0 + q, blk)) {
        const uint32_t sc = ((gptr_u8g)scales)[blk];
        bad |= sc == 0xFFu ? 1u : 0u;
        f.scale = (int)sc;
    }
    return f;
}

// The epilogue that stores C fp32 [batch, m, n].
struct MxStoreC {
    float* c;
    uint32_t m, n;
    __device__ __forceinline__ void operator()(uint32_t bi, uint64_t r, uint64_t cc, bool live, float v) const {
        if (live) ((gptr_f32g)c)[((uint64_t)bi * m + r) * n + cc] = v;
    }
};

// A workgroup's 64 x 64 tile of C fp32 [batch, m, n] = A [batch, m, nblk blocks] x B [batch or 1, n, nblk blocks]: 256 threads, each
// wave 32 x 32 as 2 x 2 instruction tiles, four accumulators, operands straight from global memory (L2), no LDS.  row_a(bi, r) ->
// the resolver of row r (which may be >= m: it is then not live) of A in batch bi.  Rows >= m, columns >= n and the K-blocks past
// nblk of the last step are masked.  The NaN rule is the kernels' own, whatever the instruction does with such bytes: the four
// lanes of a row combine their notes after the K loop, and every C of that row of A (column of C for B) is NaN.
// epi(bi, r, cc, live, v): the epilogue, called by every lane for each of its 16 elements in the order (i, reg, j) — row r =
// 16 i + 4 (lane >> 4) + reg and column cc = 16 j + (lane & 15) of the wave's quadrant —, live: r < m and cc < n, v: the element.
template <int EA, int EB, class RowA, class Epi>
__device__ __forceinline__ void mx_mfma_tile(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                             uint32_t m, uint32_t n, uint32_t nblk, uint32_t tiles_m, uint32_t tiles_n, bool b_batched, RowA row_a,
                                             Epi&& epi) {
#if defined(__HIP_DEVICE_COMPILE__)
    using f4v = __attribute__((ext_vector_type(4))) float;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_batch = tiles_m * tiles_n;                       // (the grid is below 2^31)
    const uint32_t bi = blockIdx.x / per_batch, t = blockIdx.x - bi * per_batch;
    const uint32_t tm = t / tiles_n, tn = t - tm * tiles_n;
    const uint64_t row0 = (uint64_t)tm * kMxGemmTile + (wave >> 1) * 32u, col0 = (uint64_t)tn * kMxGemmTile + (wave & 1u) * 32u;
    const uint32_t r16 = lane & 15u, q = lane >> 4;

    const uint64_t r_lo = row0 + r16, c_lo = col0 + r16, b0 = b_batched ? (uint64_t)bi * n : 0ull;
    const decltype(row_a(bi, r_lo)) a_at[2] = {row_a(bi, r_lo), row_a(bi, r_lo + 16u)};
    const MxRowBlocks b_at[2] = {{(b0 + c_lo) * nblk, nblk, c_lo < n}, {(b0 + c_lo + 16u) * nblk, nblk, c_lo + 16u < n}};
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
            fa[i] = mx_frag_load<EA>(a_codes, a_scales, a_at[i], kb0, q, a_bad[i]);
            fb[i] = mx_frag_load<EB>(b_codes, b_scales, b_at[i], kb0, q, b_bad[i]);
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
                epi(bi, r, cc, r < m && cc < n, (row_bad | b_bad[j]) ? __uint_as_float(0x7FC00000u) : acc[i][j][reg]);
            }
        }
    }
#endif
}

}  // namespace
