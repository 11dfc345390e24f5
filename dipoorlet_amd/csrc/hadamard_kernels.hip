// K13: the block-Hadamard rotation of `--mx_rotate` — y = x . blockdiag(H32) along the contiguous last axis of [rows, k], k % 32 == 0,
// H32[i][j] = (-1)^popcount(i & j) (Sylvester, natural order, symmetric, H32 . H32 = 32 I; no normalisation here: the weight side
// carries the 2^-5, tests/mx_rotate_model.py is the definition).  Five butterfly stages h = 1, 2, 4, 8, 16 per run of 32 elements:
// for every i with (i & h) == 0, (v[i], v[i | h]) <- (v[i] + v[i | h], v[i] - v[i | h]), each a single fp32 operation — the pairs
// of a stage are independent, so the result does not depend on the lane mapping and the kernel is held to the model bit for bit.
// Because k % 32 == 0 the rows fall away: the tensor is rows * k / 32 consecutive blocks.  The layout is k_fake_quant_mx_rows'
// (mx_kernels.hip): a group of 32 / VEC lanes holds one block, VEC elements per lane — 16-byte non-temporal vectors (VEC = 4, 8
// lanes per block: stages 1 and 2 inside the lane, 4, 8 and 16 as xor steps over the 8 lanes) when both bases are 16-byte aligned,
// else element by element (VEC = 1, 32 lanes, five xor steps).  In a cross-lane step the lane whose bit is clear keeps own + other,
// the lane whose bit is set other - own.  One read and one write per element (8 B); no LDS, no atomics, no scratch; 64-bit element
// indices.  A group holds its whole block before it stores, so y may be x.
#include "common.hpp"

namespace {

typedef __attribute__((address_space(1))) float* gptr_f32w;
typedef __attribute__((address_space(1))) f4* gptr_f4w;

constexpr int kHadIter = 4;           // blocks per lane group (all loads issued before the first use)

template <int VEC>
struct HadVec {
    float v[VEC];
};

template <int VEC>
__device__ __forceinline__ HadVec<VEC> had_load(const float* p) {
    HadVec<VEC> r;
    if constexpr (VEC == 4) {
        const f4 q = __builtin_nontemporal_load((gptr_f4)p);
        r.v[0] = q.x;
        r.v[1] = q.y;
        r.v[2] = q.z;
        r.v[3] = q.w;
    } else {
        r.v[0] = __builtin_nontemporal_load((gptr_f32)p);
    }
    return r;
}

template <int VEC>
__device__ __forceinline__ void had_store(float* p, const HadVec<VEC>& r) {
    if constexpr (VEC == 4) {
        const f4 q = {r.v[0], r.v[1], r.v[2], r.v[3]};
        __builtin_nontemporal_store(q, (gptr_f4w)p);
    } else {
        __builtin_nontemporal_store(r.v[0], (gptr_f32w)p);
    }
}

// Block g of the launch is elements [32 g, 32 g + 32); a workgroup owns kHadIter * 256 * VEC / 32 consecutive blocks.  Every lane
// takes every cross-lane step (a lane past the last block holds zeros, reads nothing and writes nothing).
template <int VEC>
__global__ __launch_bounds__(kBlock) void k_hadamard32(const float* x, float* y, uint64_t n_groups) {
    constexpr uint32_t LPG = 32 / VEC;                 // lanes per group
    constexpr uint32_t GPI = kBlock / LPG;             // groups per iteration of the workgroup
    const uint32_t tid = threadIdx.x, lane = tid % LPG;
    const uint64_t g0 = (uint64_t)blockIdx.x * (GPI * kHadIter) + tid / LPG;
    HadVec<VEC> v[kHadIter];
    uint64_t at[kHadIter];
    bool live[kHadIter];
#pragma unroll
    for (int i = 0; i < kHadIter; ++i) {
        const uint64_t g = g0 + (uint32_t)i * GPI;
        live[i] = g < n_groups;
        at[i] = g * 32u + lane * VEC;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[i].v[j] = 0.0f;
        if (live[i]) v[i] = had_load<VEC>(x + at[i]);
    }
#pragma unroll
    for (int i = 0; i < kHadIter; ++i) {
        if constexpr (VEC == 4) {
            const float a0 = v[i].v[0] + v[i].v[1], a1 = v[i].v[0] - v[i].v[1];       // h = 1
            const float a2 = v[i].v[2] + v[i].v[3], a3 = v[i].v[2] - v[i].v[3];
            v[i].v[0] = a0 + a2;                                                      // h = 2
            v[i].v[1] = a1 + a3;
            v[i].v[2] = a0 - a2;
            v[i].v[3] = a1 - a3;
        }
#pragma unroll
        for (uint32_t o = 1; o < LPG; o <<= 1) {                                      // h = o * VEC
            const bool hi = (lane & o) != 0u;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float own = v[i].v[j], other = __shfl_xor(own, (int)o, kWave);
                v[i].v[j] = hi ? other - own : own + other;
            }
        }
        if (live[i]) had_store<VEC>(y + at[i], v[i]);
    }
}

}  // namespace

extern "C" int dpl_hadamard32(const float* d_x, float* d_y, uint64_t rows, uint64_t k, dpl_stream_t s) {
    if (rows == 0 || k == 0) return 0;
    if (d_x == nullptr || d_y == nullptr) return fail_msg("dpl_hadamard32: d_x and d_y must not be null");
    if (k > 0x7FFFFFFFull) return fail_msg("dpl_hadamard32: k must be in [1, 2^31)");
    if ((k & 31u) != 0u) return fail_msg("dpl_hadamard32: k must be a multiple of 32");
    if (rows > 0x7FFFFFFFFFFFFFFFull / k) return fail_msg("dpl_hadamard32: tensor too large");
    const uint64_t n_groups = rows * (k / 32u);
    const bool vec = ((((uintptr_t)d_x | (uintptr_t)d_y) & 15u) == 0u);
    const uint64_t per_wg = (uint64_t)kHadIter * kBlock * (vec ? 4 : 1) / 32;
    const uint64_t blocks = (n_groups + per_wg - 1) / per_wg;
    if (blocks > 0x7FFFFFFFull) return fail_msg("dpl_hadamard32: tensor too large");
    if (vec)
        hipLaunchKernelGGL((k_hadamard32<4>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups);
    else
        hipLaunchKernelGGL((k_hadamard32<1>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_y, n_groups);
    DPL_LAUNCH_CHECK("k_hadamard32");
    return 0;
}
