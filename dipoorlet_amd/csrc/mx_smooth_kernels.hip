// K7f: `--smooth_search` — the MX error of a LayerNorm site's product under MANY candidate smoothing vectors in one launch
// (tests/mx_smooth_model.py is the definition; DESIGN.md §3y the design and the measurements; added under 37).  For candidate c:
//   A = the MX encoding (dpl_mx_encode's floor rule, blocks of 32 along k, a short last block) of fl32(x[i, kk] / s[c, kk]),
//   B = that of fl32(w[j, kk] * s[c, kk]),  C = dpl_mx_gemm's product of those bytes, NaN rule included,
//   part[(c * tiles_m + tm) * tiles_n + tn] = dpl_mx_gemm_err's two sums of the tile against ref, no bias, in its order of additions
// — bit for bit what dpl_mx_encode on the two scaled tensors and dpl_mx_gemm_err write, without the scaled tensors, the codes or C
// ever reaching memory.  x fp32 [m, k], w fp32 [n, k], s fp32 [n_cand, k], ref fp32 [m, n].
//
//   k_mx_smooth_err<ELEM, VEC4>  256 threads, one 64 x 64 tile of one candidate's C per workgroup, the candidate being the tile grid's
//       batch (workgroup b writes row b of part, as k_mx_gemm_err does); k_mx_gemm's wave split and lane map.  A K step of 128 is 64
//       rows x 4 blocks = 256 blocks per operand: thread t owns block t & 3 of row t >> 2 of BOTH operand tiles.  It loads the 32
//       scale values of its K-block once, the 32 fp32 of its row of x and of w (eight 16-byte loads each, or 32 single ones where
//       k % 4 != 0 or a base is not 16-byte aligned), divides resp. multiplies — one IEEE operation each, the file is built without
//       contraction —, takes the block maximum in its own registers (no cross-lane traffic), the shared exponent and the codes from
//       mx_block.hpp / mx_format.hpp (mx_block_se, mx_code: the encoder's own), packs the 32 codes into 8 (E4M3) or 4 (E2M1) dwords and
//       writes them and the scale byte to LDS in the order a lane's fragment is read (below).  One barrier; the four waves read their
//       fragments — one (E2M1) or two (E4M3) 16-byte LDS reads and a byte — and issue 2 x 2 v_mfma_scale_f32_16x16x128_f8f6f4.  The
//       LDS tiles are double-buffered, so a step has ONE barrier: a thread that writes buffer p of step s + 2 has passed the barrier
//       of step s + 1, which every thread reaches only after its reads of step s.  Elements at kk >= k are absent (+0.0 to the
//       maximum, code 0), blocks past the last and rows >= m / columns >= n are not read: zero codes under scale byte 127.  The
//       accumulators stay in registers; the end is mx_mfma_finish and MxErrSums (mx_mfma.hpp), k_mx_gemm_err's own.  Plain stores.
//   LDS order.  E2M1: block b of row r is the 16 bytes at u4 index 4 r + b: lane (r16, q) reads index 4 row + q, a wave 1 KiB
//       contiguous.  E4M3: a lane wants half q & 1 of block q >> 1 and the same half of block 2 + (q >> 1); half h of block b of row
//       r lies at index 256 (b >> 1) + 4 r + 2 (b & 1) + h, so both reads are index 4 row + q again, 256 apart, and the writer's two
//       halves are 32 contiguous bytes.  The scale byte of (r, b) is byte 4 r + b.  No bank conflicts on either side.
#include "mx_block.hpp"
#include "mx_mfma.hpp"

namespace {

// The 32 values at p[0 .. have) (have <= 32; p 16-byte aligned and have a multiple of 4 under VEC4), +0.0 where there is none.
template <bool VEC4>
__device__ __forceinline__ void smooth_load32(const float* p, uint32_t have, float (&v)[32]) {
    if constexpr (VEC4) {
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            f4 t = {0.f, 0.f, 0.f, 0.f};
            if (4u * j < have) t = ((gptr_f4)p)[j];
            v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 32u; ++j) v[j] = j < have ? ((gptr_f32)p)[j] : 0.f;
    }
}

// One block of `have` values (the rest absent) -> its dwords of codes and its scale byte, as dpl_mx_encode writes them.
template <int ELEM>
__device__ __forceinline__ uint32_t smooth_encode(const float (&v)[32], uint32_t have, uint32_t (&wd)[GemmOperand<ELEM>::block_bytes / 4u]) {
    constexpr uint32_t BITS = dpl_mx::Fmt<ELEM>::bits;
    uint32_t a = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 32u; ++j) a = max(a, j < have ? __float_as_uint(v[j]) & 0x7FFFFFFFu : 0u);
    bool nan;
    const int se = mx_block_se<ELEM>(a, nan);
#pragma unroll
    for (uint32_t d = 0; d < GemmOperand<ELEM>::block_bytes / 4u; ++d) wd[d] = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 32u; ++j) wd[j * BITS / 32u] |= mx_code<ELEM>(__float_as_uint(v[j]), se, nan, j < have) << (j * BITS % 32u);
    return mx_scale_byte(se, nan);
}

template <int ELEM>
struct SmoothLds {
    static constexpr uint32_t U4 = kMxGemmTile * 4u * GemmOperand<ELEM>::block_bytes / 16u;      // 16-byte units of an operand tile: 512 or 256
    u4g codes[2][2][U4];                      // [buffer][A, B]
    uint8_t scales[2][2][kMxGemmTile * 4u];
};

// Thread t's block of an operand tile into LDS (the file's comment: LDS order).
template <int ELEM>
__device__ __forceinline__ void smooth_put(u4g* codes, uint8_t* scales, uint32_t t, const uint32_t (&wd)[GemmOperand<ELEM>::block_bytes / 4u], uint32_t byte) {
    if constexpr (ELEM == DPL_MX_E4M3) {
        const uint32_t at = 256u * ((t & 3u) >> 1) + 4u * (t >> 2) + 2u * (t & 1u);
        codes[at] = u4g{wd[0], wd[1], wd[2], wd[3]};
        codes[at + 1u] = u4g{wd[4], wd[5], wd[6], wd[7]};
    } else {
        codes[t] = u4g{wd[0], wd[1], wd[2], wd[3]};
    }
    scales[t] = (uint8_t)byte;
}

// A lane's fragment of tile row `row` (0 .. 63) for K-block quarter q, and its NaN note: a 0xFF scale byte (the encoder writes an
// E4M3 NaN code into such blocks only).
template <int ELEM>
__device__ __forceinline__ GemmFrag smooth_frag(const u4g* codes, const uint8_t* scales, uint32_t row, uint32_t q, uint32_t& bad) {
    GemmFrag f;
    const u4g lo = codes[4u * row + q];
    f.v = i8v{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, 0, 0, 0, 0};
    if constexpr (ELEM == DPL_MX_E4M3) {
        const u4g hi = codes[256u + 4u * row + q];
        f.v[4] = (int)hi.x, f.v[5] = (int)hi.y, f.v[6] = (int)hi.z, f.v[7] = (int)hi.w;
    }
    const uint32_t sc = scales[4u * row + q];
    bad |= sc == 0xFFu ? 1u : 0u;
    f.scale = (int)sc;
    return f;
}

template <int ELEM, bool VEC4>
__global__ __launch_bounds__(kBlock) void k_mx_smooth_err(const float* x, const float* w, const float* sv, const float* ref, double* part, uint32_t m,
                                                          uint32_t n, uint32_t K, uint32_t nblk, uint32_t tiles_m, uint32_t tiles_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr uint32_t NW = GemmOperand<ELEM>::block_bytes / 4u;
    __shared__ SmoothLds<ELEM> lds;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t per_cand = tiles_m * tiles_n;                        // (the grid is below 2^31)
    const uint32_t cand = blockIdx.x / per_cand, tile = blockIdx.x - cand * per_cand;
    const uint32_t tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const uint32_t r16 = lane & 15u, q = lane >> 4;
    const uint32_t wr = (wave >> 1) * 32u, wc = (wave & 1u) * 32u;      // the wave's quadrant of the tile

    // the encoder's side: block eb of tile row er of both operands
    const uint32_t er = t >> 2, eb = t & 3u;
    const uint64_t a_row = (uint64_t)tm * kMxGemmTile + er, b_row = (uint64_t)tn * kMxGemmTile + er;
    const float* xs = x + a_row * K;                                    // (formed, not read, for a row that is not there)
    const float* ws = w + b_row * K;
    const float* ss = sv + (uint64_t)cand * K;

    f4v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t a_bad[2] = {0u, 0u}, b_bad[2] = {0u, 0u};

    uint32_t buf = 0u;
    for (uint32_t kb0 = 0; kb0 < nblk; kb0 += 4u, buf ^= 1u) {
        const uint32_t kb = kb0 + eb, k0 = kb * 32u;
        const uint32_t have = kb < nblk ? min(32u, K - k0) : 0u;        // elements of the thread's K-block that exist
        const uint32_t have_a = a_row < m ? have : 0u, have_b = b_row < n ? have : 0u;
        float s[32], v[32];
        uint32_t wd[NW];
        smooth_load32<VEC4>(ss + k0, (have_a | have_b) ? have : 0u, s);
        smooth_load32<VEC4>(xs + k0, have_a, v);
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = __fdiv_rn(v[j], s[j]);
        uint32_t byte = smooth_encode<ELEM>(v, have_a, wd);
        smooth_put<ELEM>(lds.codes[buf][0], lds.scales[buf][0], t, wd, have_a ? byte : 127u);
        smooth_load32<VEC4>(ws + k0, have_b, v);
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = __fmul_rn(v[j], s[j]);
        byte = smooth_encode<ELEM>(v, have_b, wd);
        smooth_put<ELEM>(lds.codes[buf][1], lds.scales[buf][1], t, wd, have_b ? byte : 127u);
        __syncthreads();

        GemmFrag fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fa[i] = smooth_frag<ELEM>(lds.codes[buf][0], lds.scales[buf][0], wr + 16u * i + r16, q, a_bad[i]);
            fb[i] = smooth_frag<ELEM>(lds.codes[buf][1], lds.scales[buf][1], wc + 16u * i + r16, q, b_bad[i]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa[i].v, fb[j].v, acc[i][j], GemmOperand<ELEM>::fmt, GemmOperand<ELEM>::fmt, 0,
                                                                             fa[i].scale, 0, fb[j].scale);
    }

    MxErrSums sums;
    mx_mfma_finish(acc, a_bad, b_bad, cand, (uint64_t)tm * kMxGemmTile + wr, (uint64_t)tn * kMxGemmTile + wc, q, r16, m, n,
                   [&](uint32_t, uint64_t r, uint64_t cc, bool live, float c) { sums.add(ref, nullptr, r * n + cc, cc, live, c); });
    sums.store(part, blockIdx.x);
#endif
}

// out[c][j] = part[c * tiles + 0][j] + part[c * tiles + 1][j] + ..., one thread per (c, j), the tiles in ascending order: a fixed
// order of fp64 additions, the same on every rank.  (The loads do not depend on the sum; the additions are the chain.)
__global__ __launch_bounds__(2 * (int)kMxSmoothMaxCand) void k_mx_smooth_sum(const double* part, uint32_t n_cand, uint64_t tiles, double* out) {
    const uint32_t c = threadIdx.x >> 1, j = threadIdx.x & 1u;
    if (c >= n_cand) return;
    const double* p = part + 2ull * c * tiles + j;
    double acc = 0.0;
    for (uint64_t t = 0; t < tiles; ++t) acc += p[2ull * t];
    out[2u * c + j] = acc;
}

}  // namespace

extern "C" int dpl_mx_smooth_sum(const double* d_part, uint64_t n_cand, uint64_t tiles, double* d_sums, dpl_stream_t s) {
    if (n_cand == 0) return 0;
    if (d_part == nullptr || d_sums == nullptr) return mx_fail("dpl_mx_smooth_sum", "d_part and d_sums must not be null");
    if (n_cand > kMxSmoothMaxCand) return mx_fail("dpl_mx_smooth_sum", "n_cand must be in [1, 64]");
    if (tiles > 0x7FFFFFFFull) return mx_fail("dpl_mx_smooth_sum", "tiles must be below 2^31");
    hipLaunchKernelGGL(k_mx_smooth_sum, dim3(1), dim3(2 * (unsigned)kMxSmoothMaxCand), 0, (hipStream_t)s, d_part, (uint32_t)n_cand, tiles, d_sums);
    DPL_LAUNCH_CHECK("k_mx_smooth_sum");
    return 0;
}

extern "C" int dpl_mx_smooth_err(int32_t elem, const float* d_x, const float* d_w, const float* d_s, uint64_t n_cand, uint64_t m, uint64_t n,
                                 uint64_t k, const float* d_ref, double* d_part, dpl_stream_t s) {
    int rc;
    MxTiles t;
    bool vec = false;
    if (mx_smooth_check(rc, t, vec, elem, d_x, d_w, d_s, n_cand, m, n, k, d_ref, d_part)) return rc;
    return mx_dispatch(elem, true, vec, [&](auto E, auto, auto VEC) {
        hipLaunchKernelGGL((k_mx_smooth_err<E, VEC == 4>), dim3((unsigned)t.blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_w, d_s, d_ref, d_part,
                           (uint32_t)m, (uint32_t)n, (uint32_t)k, (uint32_t)((k + 31u) / 32u), t.tiles_m, t.tiles_n);
        DPL_LAUNCH_CHECK("k_mx_smooth_err");
        return 0;
    });
}
