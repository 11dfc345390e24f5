// The 64 x 64 fp64 tile product of GPTQ's device kernels, defined once: the factorisation (gptq_factor_kernels.hip) and the layer
// Hessian (gptq_hessian_kernels.hip) differ in how they stage the two operands, not in what follows.
//
// Four waves in 2 x 2, each 32 x 32 of C as 2 x 2 v_mfma_f64_16x16x4_f64 accumulators, the two operands staged through LDS 32
// values of the reduction index at a time as [k][64 + 16] doubles (the 16 put k and k + 1 in different halves of the banks: a
// wave's fragment read is conflict-free).
//
// The lane map of v_mfma_f64_16x16x4_f64 (D = A[16 x 4] . B[4 x 16] + C), confirmed on an MI355X with random integer operands in
// [-15, 15] (every product and sum exact, all 256 outputs compared): lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; its
// four accumulator doubles r = 0 .. 3 are D[(l >> 4) + 4 r][l & 15] — rows interleaved by four, unlike the fp32 16 x 16 instructions.
#pragma once
#include "common.hpp"
#include "gptq_factor_plan.hpp"

namespace {

constexpr int kGfKc = 32;                      // reduction values staged per pass
constexpr int kGfLd = kGfB + 16;               // doubles per staged row
using d4 = __attribute__((ext_vector_type(4))) double;

struct GfTileLds {
    double a[kGfKc][kGfLd];
    double b[kGfKc][kGfLd];
};

// 32 staged k onto the wave's 2 x 2 accumulators: a[k][m], b[k][n] (the same panel twice for a tile on the diagonal of X^T X).
__device__ __forceinline__ void gf_mma_pass(const double (*a)[kGfLd], const double (*b)[kGfLd], d4 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = (wave >> 1) * 32 + (lane & 15), n0 = (wave & 1) * 32 + (lane & 15), kq = lane >> 4;
#pragma unroll
    for (int k = 0; k < kGfKc; k += 4) {
        const double a0 = a[k + kq][m0], a1 = a[k + kq][m0 + 16];
        const double b0 = b[k + kq][n0], b1 = b[k + kq][n0 + 16];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}
__device__ __forceinline__ void gf_mma_pass(const GfTileLds& s, d4 (&acc)[2][2]) { gf_mma_pass(s.a, s.b, acc); }

// Every element the lane holds, by the lane map above: f(row, column, value) within the 64 x 64 tile.
template <class F>
__device__ __forceinline__ void gf_for_each(const d4 (&acc)[2][2], F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                f((wave >> 1) * 32 + x * 16 + (lane >> 4) + 4 * r, (wave & 1) * 32 + y * 16 + (lane & 15), acc[x][y][r]);
}

__device__ __forceinline__ void gf_zero(d4 (&acc)[2][2]) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
}

// Block t of a launch over the tiles on and below the diagonal of an m x m tile matrix -> (i, j <= i), rows first.
__device__ __forceinline__ void gf_lower_tile(uint32_t t, uint32_t& i, uint32_t& j) {
    uint32_t r = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((uint64_t)r * (r + 1) / 2 > t) --r;
    while ((uint64_t)(r + 1) * (r + 2) / 2 <= t) ++r;
    i = r;
    j = t - (uint32_t)((uint64_t)r * (r + 1) / 2);
}

}  // namespace
