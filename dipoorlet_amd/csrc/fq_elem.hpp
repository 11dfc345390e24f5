// The element quantisers of the library, one definition: the Q/DQ of ONE fp32 value on an integer grid (fq_one) or on the OCP
// FP8 E4M3 grid (e4m3_round), and fq_elem<FMT>, which picks between them at compile time.  Included by fake_quant_kernels.hip
// (the streaming Q/DQ pair) and gptq_kernels.hip (the sequential quantise-and-compensate kernel of --gptq), which must round
// exactly as the graph's own Q/DQ node does.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ float fq_one(float x, float scale, float zp, float qlo, float qhi) {
    float q = __fadd_rn(rintf(__fdiv_rn(x, scale)), zp);  // round half to even, then zero point
    q = fminf(fmaxf(q, qlo), qhi);                        // saturate
    return __fmul_rn(__fsub_rn(q, zp), scale);
}

// The OCP FP8 E4M3 ("e4m3fn": bias 7, 3 mantissa bits, subnormal step 2^-9, largest finite 448, no infinities) Q/DQ of one value:
// the nearest e4m3fn value of v as fp32, round half to even (subnormals too), SATURATING (|v| > 448 and +-inf give +-448: ONNX
// QuantizeLinear, saturate = 1), NaN stays NaN, the sign of zero is kept.  In fp32 arithmetic on the value's own exponent bits: a
// value of binade e lies on a grid of step 2^(max(e, -6) - 3); |v| times the inverse step is exact (a power of two), v_rndne
// rounds it half to even, times the step is exact again (a carry into the next binade lands on a value of the format).  Every
// fp32 subnormal rounds to zero whether or not the multiply flushes it.  gfx950's v_cvt_pk_fp8_f32 / v_cvt_f32_fp8 would do the
// same in two instructions; how they round subnormals and what they return above 448 and for NaN has not been measured on this
// hardware (scripts/fp8_cvt_probe.hip measures it), and neither user is bound by these eight operations: the streaming
// Q/DQ kernel by its 8 B per element, the GPTQ kernel by the latency of its dependent chain (two divisions per step).
__device__ __forceinline__ float e4m3_round(float v) {
    const float a = fminf(fabsf(v), 448.f);            // saturate (a NaN comes out finite here: routed below)
    uint32_t e = __float_as_uint(a) >> 23;             // biased exponent: binade e - 127
    e = e < 121u ? 121u : e;                           // below 2^-6 the step stays 2^-9
    const float step = __uint_as_float((e - 3u) << 23), inv = __uint_as_float((257u - e) << 23);      // 2^(e-130), 2^(130-e)
    const float r = copysignf(__fmul_rn(rintf(__fmul_rn(a, inv)), step), v);
    return v != v ? v : r;
}

// The number format of the Q/DQ pair, a compile-time parameter of the kernels that include this header (k_fake_quant<PRE, FMT>,
// k_fake_quant_items<FMT>, k_gptq_block<FMT>): kFqFmtInt the integer
// grid of fq_one (scale, zero point, [qlo, qhi]); kFqFmtE4M3 y = fl32(e4m3_round(fl32(x / scale)) * scale) — the same shape, two
// single fp32 operations around the rounding; zero point / qlo / qhi are not read (zp_p may be null).
enum { kFqFmtInt = 0, kFqFmtE4M3 = 1 };
template <int FMT>
__device__ __forceinline__ float fq_elem(float x, float scale, float zp, float qlo, float qhi) {
    if (FMT == kFqFmtE4M3) return __fmul_rn(e4m3_round(__fdiv_rn(x, scale)), scale);
    return fq_one(x, scale, zp, qlo, qhi);
}
template <int FMT>
__device__ __forceinline__ float fq_zp(const int32_t* __restrict__ zp_p, uint32_t c) {
    return FMT == kFqFmtInt ? (float)zp_p[c] : 0.f;
}

}  // namespace
