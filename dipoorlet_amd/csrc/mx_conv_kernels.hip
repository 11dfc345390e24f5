// K7d: `--mx_conv` — a convolution of two packed MX operands on CDNA4's block-scaled matrix instruction, as an implicit GEMM
// (tests/mx_conv_model.py is the definition; DESIGN.md §3r the tap addressing and the measurements; §3o the lane map).  Both operands
// are what dpl_mx_encode writes along axis 1: the activation [n, c, h, w] as NHWC codes [n, h, w, Cb * bb] with scales [n, h, w, Cb],
// the weight [cout, c, kh, kw] as [cout, kh, kw, Cb * bb] with scales [cout, kh, kw, Cb]; Cb = ceil(c / 32), bb = 32 (E4M3), 24 (E2M3 / E3M2) or 16
// (E2M1) bytes a block.  C fp32 [n, oh, ow, cout]:
//   C[b, oy, ox, co] = sum over ky, kx and ch < 32 Cb of a[b, oy sh - pt + ky dh, ox sw - pl + kx dw, ch] * b[co, ky, kx, ch]
// a tap outside the image contributing nothing.  That is k_mx_gemm's product with m = oh * ow rows per image and K = the kh * kw * Cb
// K-blocks of a weight row in its memory order (ky, kx, cb): B is a plain K-innermost row (MxRowBlocks), and K-block kb of A's row
// (oy, ox) is channel block kb % Cb of the pixel that tap kb / Cb reaches (ConvRowBlocks).
//
//   k_mx_conv<EA, EB>  k_mx_gemm's tile (mx_mfma.hpp: mx_mfma_tile), 64 output pixels of one image x 64 output channels per
//                      workgroup — the un-staged form: a pixel's blocks are read again for every tap that reaches it.  Every
//                      K-block a lane touches in a step — one (E2M1) or up to three (E4M3: two for codes, one for the scale) — is
//                      resolved and masked on its own: a row >= oh * ow, a tap outside the image or a block past the end supplies
//                      zero dwords resp. scale byte 127, and nothing is loaded for it.
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

// One output pixel as a row of A: its image, and the pixel its tap (0, 0) reaches (may lie outside the image).
struct ConvRowBlocks {
    const ConvGeom& g;
    uint64_t img;
    int64_t iy0, ix0;
    bool live;                                // row < oh * ow
    // -> does K-block kb of the row exist in the image?  blk: its index among the [n, h, w, Cb] blocks.  (The tap is kb's alone: a
    // lane asks the same kb of both of its rows in a step, and the divisions are done once for the two.  The tests are joined with
    // &, not &&: one mask per block, as for a plain row, where && makes the compiler branch on each test — DESIGN.md §3t.)
    __device__ __forceinline__ bool operator()(uint32_t kb, uint64_t& blk) const {
        const uint32_t tap = kb / g.cb, ky = tap / g.kw, kx = tap - ky * g.kw;
        const int64_t iy = iy0 + (int64_t)ky * g.dh, ix = ix0 + (int64_t)kx * g.dw;
        blk = ((img * g.h + (uint64_t)iy) * g.w + (uint64_t)ix) * g.cb + (kb - tap * g.cb);
        return live & (kb < g.nblk) & (iy >= 0) & (iy < (int64_t)g.h) & (ix >= 0) & (ix < (int64_t)g.w);
    }
};

template <int EA, int EB>
__global__ __launch_bounds__(kBlock) void k_mx_conv(const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes, const uint8_t* b_scales,
                                                    float* c, ConvGeom g) {
    const uint32_t m = g.oh * g.ow;                                     // (below 2^31)
    mx_mfma_tile<EA, EB>(a_codes, a_scales, b_codes, b_scales, m, g.cout, g.nblk, g.tiles_m, g.tiles_n, false, [&](uint32_t bi, uint64_t r) {
        const uint32_t rr = r < m ? (uint32_t)r : 0u, oy = rr / g.ow, ox = rr - oy * g.ow;
        return ConvRowBlocks{g, bi, (int64_t)oy * g.sh - (int64_t)g.pt, (int64_t)ox * g.sw - (int64_t)g.pl, r < m};
    }, MxStoreC{c, m, g.cout});
}

}  // namespace

extern "C" int dpl_mx_conv(int32_t elem_a, int32_t elem_b, const uint8_t* d_a_codes, const uint8_t* d_a_scales, const uint8_t* d_b_codes,
                           const uint8_t* d_b_scales, int64_t n, int64_t h, int64_t w, int64_t c, int64_t cout, int64_t kh, int64_t kw,
                           int64_t stride_h, int64_t stride_w, int64_t pad_top, int64_t pad_left, int64_t dil_h, int64_t dil_w, int64_t oh, int64_t ow,
                           float* d_c, dpl_stream_t s) {
    const MxPair o = {elem_a, elem_b, d_a_codes, d_a_scales, d_b_codes, d_b_scales, d_c};
    int rc;
    MxConvPlan p;
    if (mx_conv_check(rc, p, o, {n, h, w, c, cout, kh, kw, stride_h, stride_w, pad_top, pad_left, dil_h, dil_w, oh, ow})) return rc;
    ConvGeom g;
    g.h = (uint32_t)h, g.w = (uint32_t)w, g.cb = (uint32_t)p.cb, g.cout = (uint32_t)cout, g.kw = (uint32_t)kw, g.oh = (uint32_t)oh, g.ow = (uint32_t)ow;
    g.sh = (uint32_t)stride_h, g.sw = (uint32_t)stride_w, g.pt = (uint32_t)pad_top, g.pl = (uint32_t)pad_left, g.dh = (uint32_t)dil_h, g.dw = (uint32_t)dil_w;
    g.nblk = (uint32_t)p.nblk, g.tiles_m = p.t.tiles_m, g.tiles_n = p.t.tiles_n;
    return mx_pair_dispatch_all(o, [&](auto EA, auto EB) {
        hipLaunchKernelGGL((k_mx_conv<EA, EB>), dim3((unsigned)p.t.blocks), dim3(kBlock), 0, (hipStream_t)s, o.a_codes, o.a_scales, o.b_codes, o.b_scales,
                           o.c, g);
        DPL_LAUNCH_CHECK("k_mx_conv");
        return 0;
    });
}
