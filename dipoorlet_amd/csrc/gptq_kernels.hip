// K12: GPTQ's sequential quantise-and-compensate step over one block of weight columns (--gptq, --mx_gptq; Frantar et al., 2022) and
// its C ABI.  A row (output channel) is a dependent chain of nb <= 128 steps — round column j, divide its error by U[j, j], subtract
// e * U[j, k] from every column k > j of the block — and rows do not talk to each other.  One wave owns one row: its columns live
// in registers, two per lane (column l and column 64 + l); step j fetches column j from the lane that owns it with a readlane (j
// is wave-uniform), every lane computes the same Q and e, and updates its own two columns from row j of U in LDS (consecutive
// lanes, consecutive words: conflict-free).  The upper triangle of the nb x nb block of U is staged once per workgroup, in nb * nb
// words of dynamic LDS.  No atomics, no traffic between waves: every value is produced by the same single fp32
// operations in the same order whatever the launch geometry, which is why tests/gptq_model.py gptq_block is matched bit for bit.  (The inter-block update W -= Err @ U is a GEMM and
// is left to the BLAS library: ops.gptq_quantize.)
//
// Two kernels share the step (gptq_step) and the staging (gptq_stage_u) and differ in where q comes from:
//   k_gptq_block<FMT>      a static grid: fq_elem<FMT> under the row's scale (and zero point);
//   k_gptq_mx_block<ELEM>  an MX block-scaled grid (tests/mx_gptq_model.py gptq_mx_block): at every column that is a multiple of 32
//                          the 32 lanes that hold the block reduce |w| as bit patterns to its maximum (five xor-shuffles inside a
//                          32-lane half: c0 is a multiple of 32, so a block never straddles the two register columns), which fixes
//                          the block's shared exponent; its columns are rounded under it on their bit patterns (mx_format.hpp:
//                          integer arithmetic, independent of the code object's denormal mode; E4M3 with keep_top_closed, which
//                          keeps the finished block a fixed point of the floor-rule Q/DQ).
#include "common.hpp"
#include "fq_elem.hpp"
#include "mx_block.hpp"

namespace {

constexpr int kGptqMaxBlock = DPL_GPTQ_MAX_BLOCK;   // columns per call: two per lane of a wave
constexpr int kGptqRows = kBlock / kWave;           // rows per workgroup: one per wave
static_assert(kGptqMaxBlock == 2 * kWave, "a lane holds two columns of the block");

__device__ __forceinline__ float lane_value(float v, int lane) {   // lane: wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One step of the chain for the wave's row.  `wj`: the row's value in column j, `q`: its rounded value (both uniform over the
// wave); u_row: row j of the staged block.  Lane l holds columns l (w0) and 64 + l (w1) and the errors of steps l (e0) and 64 + l (e1).
__device__ __forceinline__ void gptq_step(int j, float wj, float q, const float* __restrict__ u_row, int lane, int nb, float& w0, float& w1,
                                          float& e0, float& e1) {
    const float e = __fdiv_rn(__fsub_rn(wj, q), u_row[j]);
    const int k0 = lane, k1 = lane + kWave;
    if (k0 == j) {
        w0 = q;
        e0 = e;
    } else if (k0 > j && k0 < nb) {
        w0 = __fsub_rn(w0, __fmul_rn(e, u_row[k0]));
    }
    if (k1 == j) {
        w1 = q;
        e1 = e;
    } else if (k1 > j && k1 < nb) {
        w1 = __fsub_rn(w1, __fmul_rn(e, u_row[k1]));
    }
}

// The block of U, row j at word j * nb: nb * nb * 4 bytes of dynamic LDS (64 KB at nb = 128, 4 KB at 32: a small block leaves the
// CU's LDS to more workgroups).  Wave v stages rows v, v + 4, ...; only the upper triangle is ever read, so only it is loaded.
__device__ __forceinline__ void gptq_stage_u(float* __restrict__ u_lds, const float* __restrict__ u, uint64_t ldu, uint64_t c0, int nb, int lane) {
    for (int j = threadIdx.x >> 6; j < nb; j += kGptqRows) {
        const float* __restrict__ u_row = u + (c0 + j) * ldu + c0;
        for (int k = j + lane; k < nb; k += kWave) u_lds[j * nb + k] = u_row[k];
    }
    __syncthreads();
}

template <int FMT>
__global__ __launch_bounds__(kBlock) void k_gptq_block(float* __restrict__ w, uint32_t rows, uint64_t ldw, uint64_t c0, int nb,
                                                        const float* __restrict__ u, uint64_t ldu, const float* __restrict__ scale_p,
                                                        const int32_t* __restrict__ zp_p, uint32_t n_channels, float qlo, float qhi,
                                                        float* __restrict__ err) {
    extern __shared__ float u_lds[];
    const int lane = threadIdx.x & (kWave - 1);
    gptq_stage_u(u_lds, u, ldu, c0, nb, lane);
    const uint32_t r = blockIdx.x * kGptqRows + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint32_t ch = n_channels == 1u ? 0u : r;
    const float scale = scale_p[ch], zp = fq_zp<FMT>(zp_p, ch);
    float* wr = w + (uint64_t)r * ldw + c0;
    const bool has0 = lane < nb, has1 = lane + kWave < nb;
    float w0 = has0 ? wr[lane] : 0.f, w1 = has1 ? wr[lane + kWave] : 0.f, e0 = 0.f, e1 = 0.f;
    const int n0 = nb < kWave ? nb : kWave;
    for (int j = 0; j < n0; ++j) {
        const float wj = lane_value(w0, j);
        gptq_step(j, wj, fq_elem<FMT>(wj, scale, zp, qlo, qhi), u_lds + j * nb, lane, nb, w0, w1, e0, e1);
    }
    for (int j = kWave; j < nb; ++j) {
        const float wj = lane_value(w1, j - kWave);
        gptq_step(j, wj, fq_elem<FMT>(wj, scale, zp, qlo, qhi), u_lds + j * nb, lane, nb, w0, w1, e0, e1);
    }
    float* er = err + (uint64_t)r * (uint32_t)nb;
    if (has0) {
        wr[lane] = w0;
        er[lane] = e0;
    }
    if (has1) {
        wr[lane + kWave] = w1;
        er[lane + kWave] = e1;
    }
}

// The same chain on an MX grid.  The call's columns are whole MX blocks (c0 and nb are multiples of 32; the last block of the
// matrix may be short, and the registers past nb hold +0.0, which adds nothing to a maximum), so local column b0 = 0, 32, 64, 96
// enters a block held by lanes b0 % 64 .. b0 % 64 + 31 of one register column.  Everything about a block — its maximum, se, the NaN
// flag — is uniform over the wave; the lane that holds the block's first column stores its E8M0 byte.
template <int ELEM>
__global__ __launch_bounds__(kBlock) void k_gptq_mx_block(float* __restrict__ w, uint32_t rows, uint64_t ldw, uint64_t c0, int nb,
                                                           const float* __restrict__ u, uint64_t ldu, float* __restrict__ err,
                                                           uint8_t* __restrict__ scales, uint64_t ld_scales) {
    extern __shared__ float u_lds[];
    const int lane = threadIdx.x & (kWave - 1);
    gptq_stage_u(u_lds, u, ldu, c0, nb, lane);
    const uint32_t r = blockIdx.x * kGptqRows + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* wr = w + (uint64_t)r * ldw + c0;
    uint8_t* sr = scales + (uint64_t)r * ld_scales + c0 / dpl_mx::kBlock32;
    const bool has0 = lane < nb, has1 = lane + kWave < nb;
    float w0 = has0 ? wr[lane] : 0.f, w1 = has1 ? wr[lane + kWave] : 0.f, e0 = 0.f, e1 = 0.f;
    for (int b0 = 0; b0 < nb; b0 += dpl_mx::kBlock32) {
        const bool upper = b0 >= kWave;                       // which register column holds the block
        const int l0 = b0 & (kWave - 1);
        uint32_t a = __float_as_uint(upper ? w1 : w0) & 0x7FFFFFFFu;
#pragma unroll
        for (int o = 1; o < dpl_mx::kBlock32; o <<= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, kWave));
        a = (uint32_t)__builtin_amdgcn_readlane((int)a, l0);
        bool nan;
        const int se = mx_block_se<ELEM>(a, nan);
        if (lane == l0) sr[b0 / dpl_mx::kBlock32] = nan ? (uint8_t)0xFF : (uint8_t)(se + 127);
        const int j_end = b0 + dpl_mx::kBlock32 < nb ? b0 + dpl_mx::kBlock32 : nb;
        uint32_t m = 0u;                                      // the largest |q| pattern the block has been given so far (E4M3's rule)
        for (int j = b0; j < j_end; ++j) {
            const float wj = lane_value(upper ? w1 : w0, j & (kWave - 1));
            const uint32_t wb = __float_as_uint(wj), b = wb & 0x7FFFFFFFu;
            const uint32_t y = dpl_mx::keep_top_closed<ELEM>(b, dpl_mx::round_bits<ELEM>(b, se), m);
            m = max(m, y);
            const float q = __uint_as_float(nan ? kQuietNaN : (wb & 0x80000000u) | y);
            gptq_step(j, wj, q, u_lds + j * nb, lane, nb, w0, w1, e0, e1);
        }
    }
    float* er = err + (uint64_t)r * (uint32_t)nb;
    if (has0) {
        wr[lane] = w0;
        er[lane] = e0;
    }
    if (has1) {
        wr[lane + kWave] = w1;
        er[lane + kWave] = e1;
    }
}

}  // namespace

extern "C" {

int dpl_gptq_mx_block(int32_t elem, float* d_w, int64_t rows, int64_t ldw, int64_t k, int64_t c0, int64_t nb, const float* d_u, int64_t ldu,
                      float* d_err, uint8_t* d_scales, int64_t ld_scales, dpl_stream_t s) {
    if (elem != DPL_MX_E4M3 && elem != DPL_MX_E2M1) return fail_msg("dpl_gptq_mx_block: elem must be DPL_MX_E4M3 or DPL_MX_E2M1");
    if (d_w == nullptr || d_u == nullptr || d_err == nullptr || d_scales == nullptr) return fail_msg("dpl_gptq_mx_block: null pointer");
    if (nb < 1 || nb > kGptqMaxBlock) return fail_msg("dpl_gptq_mx_block: nb must be in [1, 128]");
    if (c0 < 0 || c0 % dpl_mx::kBlock32 != 0) return fail_msg("dpl_gptq_mx_block: c0 must be a non-negative multiple of 32");
    if (k < 1 || ldw < 1 || ldu < 1 || k > ldw || c0 > k - nb || c0 > ldu - nb)
        return fail_msg("dpl_gptq_mx_block: columns [c0, c0 + nb) must lie inside k <= ldw and inside ldu");
    if (nb % dpl_mx::kBlock32 != 0 && c0 + nb != k)
        return fail_msg("dpl_gptq_mx_block: nb must be a multiple of 32 unless the call ends at column k (whole MX blocks only)");
    if (ld_scales < (k + dpl_mx::kBlock32 - 1) / dpl_mx::kBlock32) return fail_msg("dpl_gptq_mx_block: ld_scales must be at least ceil(k / 32)");
    if (rows <= 0) return 0;
    if (rows > 0x7FFFFFFFll) return fail_msg("dpl_gptq_mx_block: too many rows");
    const unsigned blocks = (unsigned)((rows + kGptqRows - 1) / kGptqRows);
#define DPL_GPTQ_MX_LAUNCH(ELEM)                                                                                                        \
    hipLaunchKernelGGL((k_gptq_mx_block<ELEM>), dim3(blocks), dim3(kBlock), (size_t)(nb * nb) * sizeof(float), (hipStream_t)s, d_w, \
                       (uint32_t)rows, (uint64_t)ldw, (uint64_t)c0, (int)nb, d_u, (uint64_t)ldu, d_err, d_scales, (uint64_t)ld_scales)
    if (elem == DPL_MX_E4M3) DPL_GPTQ_MX_LAUNCH(0);
    else DPL_GPTQ_MX_LAUNCH(1);
#undef DPL_GPTQ_MX_LAUNCH
    DPL_LAUNCH_CHECK("k_gptq_mx_block");
    return 0;
}

int dpl_gptq_block(float* d_w, int64_t rows, int64_t ldw, int64_t c0, int64_t nb, const float* d_u, int64_t ldu, const float* d_scale,
                   const int32_t* d_zero_point, int64_t n_channels, int32_t qlo, int32_t qhi, int32_t fmt, float* d_err, dpl_stream_t s) {
    if (fmt != DPL_GRID_UNIFORM && fmt != DPL_GRID_E4M3) return fail_msg("dpl_gptq_block: fmt must be DPL_GRID_UNIFORM or DPL_GRID_E4M3");
    if (d_w == nullptr || d_u == nullptr || d_scale == nullptr || d_err == nullptr || (fmt == DPL_GRID_UNIFORM && d_zero_point == nullptr))
        return fail_msg("dpl_gptq_block: null pointer (d_zero_point may be null for DPL_GRID_E4M3 only)");
    if (nb < 1 || nb > kGptqMaxBlock) return fail_msg("dpl_gptq_block: nb must be in [1, 128]");
    if (c0 < 0 || ldw < 1 || ldu < 1 || c0 > ldw - nb || c0 > ldu - nb)
        return fail_msg("dpl_gptq_block: columns [c0, c0 + nb) must lie inside ldw and ldu");
    if (rows <= 0) return 0;
    if (rows > 0x7FFFFFFFll) return fail_msg("dpl_gptq_block: too many rows");
    if (n_channels != 1 && n_channels != rows) return fail_msg("dpl_gptq_block: n_channels must be 1 or rows");
    if (fmt == DPL_GRID_UNIFORM && qlo >= qhi) return fail_msg("dpl_gptq_block: the integer grid needs qlo < qhi");
    const unsigned blocks = (unsigned)((rows + kGptqRows - 1) / kGptqRows);
#define DPL_GPTQ_LAUNCH(FMT)                                                                                                      \
    hipLaunchKernelGGL((k_gptq_block<FMT>), dim3(blocks), dim3(kBlock), (size_t)(nb * nb) * sizeof(float), (hipStream_t)s, d_w, \
                       (uint32_t)rows, (uint64_t)ldw, (uint64_t)c0, (int)nb, d_u, (uint64_t)ldu, d_scale, d_zero_point, (uint32_t)n_channels, (float)qlo, (float)qhi, \
                       d_err)
    if (fmt == DPL_GRID_E4M3) DPL_GPTQ_LAUNCH(kFqFmtE4M3);
    else DPL_GPTQ_LAUNCH(kFqFmtInt);
#undef DPL_GPTQ_LAUNCH
    DPL_LAUNCH_CHECK("k_gptq_block");
    return 0;
}

}  // extern "C"
