// K7d: `--mx_conv` — a convolution of two packed MX operands on CDNA4's block-scaled matrix instruction, as an implicit GEMM
// (tests/mx_conv_model.py is the definition; DESIGN.md §3r the tap addressing and the measurements; §3o the lane map).  Both operands
// are what dpl_mx_encode writes along axis 1: the activation [n, c, h, w] as NHWC codes [n, h, w, Cb * bb] with scales [n, h, w, Cb],
// the weight [cout, c, kh, kw] as [cout, kh, kw, Cb * bb] with scales [cout, kh, kw, Cb]; Cb = ceil(c / 32), bb = 32 (E4M3) or 16
// (E2M1) bytes a block.  C fp32 [n, oh, ow, cout]:
//   C[b, oy, ox, co] = sum over ky, kx and ch < 32 Cb of a[b, oy sh - pt + ky dh, ox sw - pl + kx dw, ch] * b[co, ky, kx, ch]
// a tap outside the image contributing nothing.  That is k_mx_gemm's product with m = oh * ow rows per image and K = the kh * kw * Cb
// K-blocks of a weight row in its memory order (ky, kx, cb): B is a plain K-innermost row (gemm_load), and K-block kb of A's row
// (oy, ox) is channel block kb % Cb of the pixel that tap kb / Cb reaches.
//
//   k_mx_conv<EA, EB>  k_mx_gemm's shape: 256 threads, 64 output pixels of one image x 64 output channels per workgroup, each wave
//                      32 x 32 as 2 x 2 instruction tiles, four accumulators, operands straight from global memory (L2), no LDS —
//                      the un-staged form: a pixel's blocks are read again for every tap that reaches it.  Every K-block a lane
//                      touches in a step — one (E2M1) or up to three (E4M3: two for codes, one for the scale) — is resolved and
//                      masked on its own: a row >= oh * ow, a tap outside the image or a block past the end supplies zero dwords
//                      resp. scale byte 127, and nothing is loaded for it.
// The NaN rule is k_mx_gemm's, on what is loaded: an output is NaN if a block of A inside one of its in-image taps, or any block of
// row co of B, holds a 0xFF scale byte or an E4M3 NaN code.  A bad pixel no tap of an output reaches leaves that output finite.
// No atomics, 64-bit indices.
#include "mx_mfma.hpp"

namespace {

struct ConvGeom {
    uint32_t h, w, cb, cout, kw, oh, ow;      // cb: channel blocks of 32
    uint32_t sh, sw, pt, pl, dh, dw;
    uint32_t nblk;                            // kh * kw * cb: the K-blocks of a weight row
    uint32_t tiles_m, tiles_n;
};

// K-block kb of the A operand: the offset of its tap from an output's first tap, and its channel block.
struct ConvTap {
    int64_t dy, dx;
    uint32_t cb;
    bool live;                                // kb < nblk
};

__device__ __forceinline__ ConvTap conv_tap(const ConvGeom& g, uint32_t kb) {
    ConvTap t;
    const uint32_t tap = kb / g.cb, ky = tap / g.kw, kx = tap - ky * g.kw;
    t.live = kb < g.nblk;
    t.cb = kb - tap * g.cb;
    t.dy = (int64_t)ky * g.dh;
    t.dx = (int64_t)kx * g.dw;
    return t;
}

// One output pixel as a row of A: its image, and the pixel its tap (0, 0) reaches (may lie outside the image).
struct ConvRow {
    uint64_t img;
    int64_t iy0, ix0;
    bool live;                                // row < oh * ow
};

// -> does block t of row r exist in the image?  blk: its index among the [n, h, w, Cb] blocks.
__device__ __forceinline__ bool conv_block(const ConvGeom& g, const ConvRow& r, const ConvTap& t, uint64_t& blk) {
    const int64_t iy = r.iy0 + t.dy, ix = r.ix0 + t.dx;
    if (!(r.live && t.live && iy >= 0 && iy < (int64_t)g.h && ix >= 0 && ix < (int64_t)g.w)) return false;
    blk = ((r.img * g.h + (uint64_t)iy) * g.w + (uint64_t)ix) * g.cb + t.cb;
    return true;
}

// gemm_load for the A operand: ts is the block whose scale byte (and, E2M1, whose codes) this lane supplies, t_lo / t_hi (E4M3
// only) the two blocks it supplies half q & 1 of.
template <int ELEM>
__device__ __forceinline__ GemmFrag conv_load_a(const uint8_t* codes, const uint8_t* scales, const ConvGeom& g, const ConvRow& r, const ConvTap& ts,
                                                const ConvTap& t_lo, const ConvTap& t_hi, uint32_t q, uint32_t& bad) {
    GemmFrag f;
    f.v = i8v{0, 0, 0, 0, 0, 0, 0, 0};
    f.scale = 127;
    uint64_t blk;
    if constexpr (ELEM == DPL_MX_E4M3) {
        const uint32_t half = (q & 1u) * 16u;
        if (conv_block(g, r, t_lo, blk)) {
            const u4g lo = *(gptr_u4g)(codes + blk * GemmOperand<ELEM>::block_bytes + half);
            f.v[0] = (int)lo.x, f.v[1] = (int)lo.y, f.v[2] = (int)lo.z, f.v[3] = (int)lo.w;
            bad |= e4m3_nan_in(lo.x) | e4m3_nan_in(lo.y) | e4m3_nan_in(lo.z) | e4m3_nan_in(lo.w);
        }
        if (conv_block(g, r, t_hi, blk)) {
            const u4g hi = *(gptr_u4g)(codes + blk * GemmOperand<ELEM>::block_bytes + half);
            f.v[4] = (int)hi.x, f.v[5] = (int)hi.y, f.v[6] = (int)hi.z, f.v[7] = (int)hi.w;
            bad |= e4m3_nan_in(hi.x) | e4m3_nan_in(hi.y) | e4m3_nan_in(hi.z) | e4m3_nan_in(hi.w);
        }
    } else {
        if (conv_block(g, r, ts, blk)) {
            const u4g lo = *(gptr_u4g)(codes + blk * GemmOperand<ELEM>::block_bytes);
            f.v[0] = (int)lo.x, f.v[1] = (int)lo.y, f.v[2] = (int)lo.z, f.v[3] = (int)lo.w;
        }
    }
    if (conv_block(g, r, ts, blk)) {
        const uint32_t sc = ((gptr_u8g)scales)[blk];
        bad |= sc == 0xFFu ? 1u : 0u;
        f.scale = (int)sc;
    }
    return f;
}

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_conv(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                    float* c, ConvGeom g) {
#if defined(__HIP_DEVICE_COMPILE__)
    using f4v = __attribute__((ext_vector_type(4))) float;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_image = g.tiles_m * g.tiles_n;                   // (the grid is below 2^31)
    const uint32_t bi = blockIdx.x / per_image, t = blockIdx.x - bi * per_image;
    const uint32_t tm = t / g.tiles_n, tn = t - tm * g.tiles_n;
    const uint32_t m = g.oh * g.ow;                                     // (below 2^31)
    const uint64_t row0 = (uint64_t)tm * kMxGemmTile + (wave >> 1) * 32u, col0 = (uint64_t)tn * kMxGemmTile + (wave & 1u) * 32u;
    const uint32_t r16 = lane & 15u, q = lane >> 4;

    ConvRow a_row[2];
    uint64_t b_row[2];
    bool b_live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint64_t r = row0 + 16u * i + r16, cc = col0 + 16u * i + r16;
        const uint32_t rr = r < m ? (uint32_t)r : 0u, oy = rr / g.ow, ox = rr - oy * g.ow;
        a_row[i].live = r < m;
        a_row[i].img = bi;
        a_row[i].iy0 = (int64_t)oy * g.sh - (int64_t)g.pt;
        a_row[i].ix0 = (int64_t)ox * g.sw - (int64_t)g.pl;
        b_live[i] = cc < g.cout;
        b_row[i] = cc;
    }
    f4v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t a_bad[2] = {0u, 0u}, b_bad[2] = {0u, 0u};

    for (uint32_t kb0 = 0; kb0 < g.nblk; kb0 += 4u) {
        // the blocks this lane touches in this step: the same for both of its rows
        const ConvTap ts = conv_tap(g, kb0 + q);
        ConvTap t_lo = ts, t_hi = ts;
        if constexpr (EA == DPL_MX_E4M3) {
            t_lo = conv_tap(g, kb0 + (q >> 1));
            t_hi = conv_tap(g, kb0 + 2u + (q >> 1));
        }
        GemmFrag fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = conv_load_a<EA>(a_codes, a_scales, g, a_row[i], ts, t_lo, t_hi, q, a_bad[i]);
            fb[i] = gemm_load<EB>(b_codes, b_scales, b_row[i], g.nblk, kb0, q, b_live[i], b_bad[i]);
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
                if (r < m && cc < g.cout) {
                    const float v = (row_bad | b_bad[j]) ? __uint_as_float(0x7FC00000u) : acc[i][j][reg];
                    ((gptr_f32g)c)[((uint64_t)bi * m + r) * g.cout + cc] = v;
                }
            }
        }
    }
#endif
}

template <int EA, int EB>
int mx_conv_launch(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales, uint64_t n, const ConvGeom& g,
                   float* c, dpl_stream_t s) {
    hipLaunchKernelGGL((k_mx_conv<EA, EB>), dim3((unsigned)(n * g.tiles_m * g.tiles_n)), dim3(kBlock), 0, (hipStream_t)s, a_codes, a_scales, b_codes,
                       b_scales, c, g);
    DPL_LAUNCH_CHECK("k_mx_conv");
    return 0;
}

// acc *= f unless that passes limit
bool conv_mul(uint64_t& acc, uint64_t f, uint64_t limit) {
    if (f != 0 && acc > limit / f) return false;
    acc *= f;
    return true;
}

}  // namespace

extern "C" int dpl_mx_conv(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                           const uint8_t* d_b_scales, int64_t n, int64_t h, int64_t w, int64_t c, int64_t cout, int64_t kh, int64_t kw,
                           int64_t stride_h, int64_t stride_w, int64_t pad_top, int64_t pad_left, int64_t dil_h, int64_t dil_w, int64_t oh, int64_t ow,
                           float* d_c, dpl_stream_t s) {
    if ((elem_a != DPL_MX_E4M3 && elem_a != DPL_MX_E2M1) || (elem_b != DPL_MX_E4M3 && elem_b != DPL_MX_E2M1))
        return fail_msg("dpl_mx_conv: elem_a and elem_b must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (kh < 1 || kw < 1 || stride_h < 1 || stride_w < 1 || dil_h < 1 || dil_w < 1)
        return fail_msg("dpl_mx_conv: kh, kw, the strides and the dilations must be at least 1");
    if (pad_top < 0 || pad_left < 0) return fail_msg("dpl_mx_conv: pad_top and pad_left must not be negative");
    for (int64_t d : {n, h, w, c, cout, kh, kw, stride_h, stride_w, pad_top, pad_left, dil_h, dil_w, oh, ow})
        if (d < 0 || d > 0x7FFFFFFFll) return fail_msg("dpl_mx_conv: every dimension, stride, pad and dilation must be in [0, 2^31)");
    if (n == 0 || h == 0 || w == 0 || c == 0 || cout == 0 || oh == 0 || ow == 0) return 0;
    if (d_a_codes == nullptr || d_a_scales == nullptr || d_b_codes == nullptr || d_b_scales == nullptr || d_c == nullptr)
        return fail_msg("dpl_mx_conv: the codes, the scales and d_c must not be null");
    // (the K-blocks of a weight row and the output pixels of an image are 32-bit in the kernel; both operands' codes, at most 32
    // bytes a block, and C must be indexable)
    const uint64_t cb = ((uint64_t)c + 31u) / 32u, big = 0x7FFFFFFFFFFFFFFFull;
    uint64_t nblk = (uint64_t)kh, m = (uint64_t)oh, a_bytes = 32u, b_bytes = 32u, c_bytes = 4u;
    const bool fits = conv_mul(nblk, (uint64_t)kw, 0x7FFFFFFFull) && conv_mul(nblk, cb, 0x7FFFFFFFull) && conv_mul(m, (uint64_t)ow, 0x7FFFFFFFull) &&
                      conv_mul(a_bytes, (uint64_t)n, big) && conv_mul(a_bytes, (uint64_t)h, big) && conv_mul(a_bytes, (uint64_t)w, big) &&
                      conv_mul(a_bytes, cb, big) && conv_mul(b_bytes, (uint64_t)cout, big) && conv_mul(b_bytes, nblk, big) &&
                      conv_mul(c_bytes, (uint64_t)n, big) && conv_mul(c_bytes, m, big) && conv_mul(c_bytes, (uint64_t)cout, big);
    if (!fits) return fail_msg("dpl_mx_conv: tensor too large");
    const uint64_t tiles_m = (m + kMxGemmTile - 1) / kMxGemmTile, tiles_n = ((uint64_t)cout + kMxGemmTile - 1) / kMxGemmTile;
    if (tiles_m * tiles_n > 0x7FFFFFFFull || (uint64_t)n > 0x7FFFFFFFull / (tiles_m * tiles_n)) return fail_msg("dpl_mx_conv: tensor too large (the grid)");
    if ((((uintptr_t)d_a_codes | (uintptr_t)d_b_codes) & 15u) != 0u)
        return fail_msg("dpl_mx_conv: d_a_codes and d_b_codes must be 16-byte aligned (a block's codes are loaded as 16-byte vectors)");
    ConvGeom g;
    g.h = (uint32_t)h, g.w = (uint32_t)w, g.cb = (uint32_t)cb, g.cout = (uint32_t)cout, g.kw = (uint32_t)kw, g.oh = (uint32_t)oh, g.ow = (uint32_t)ow;
    g.sh = (uint32_t)stride_h, g.sw = (uint32_t)stride_w, g.pt = (uint32_t)pad_top, g.pl = (uint32_t)pad_left, g.dh = (uint32_t)dil_h, g.dw = (uint32_t)dil_w;
    g.nblk = (uint32_t)nblk, g.tiles_m = (uint32_t)tiles_m, g.tiles_n = (uint32_t)tiles_n;
    const int pair = (elem_a == DPL_MX_E2M1 ? 2 : 0) | (elem_b == DPL_MX_E2M1 ? 1 : 0);
    switch (pair) {
    case 0: return mx_conv_launch<DPL_MX_E4M3, DPL_MX_E4M3>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, (uint64_t)n, g, d_c, s);
    case 1: return mx_conv_launch<DPL_MX_E4M3, DPL_MX_E2M1>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, (uint64_t)n, g, d_c, s);
    case 2: return mx_conv_launch<DPL_MX_E2M1, DPL_MX_E4M3>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, (uint64_t)n, g, d_c, s);
    default: return mx_conv_launch<DPL_MX_E2M1, DPL_MX_E2M1>(d_a_codes, d_a_scales, d_b_codes, d_b_scales, (uint64_t)n, g, d_c, s);
    }
}
