// OCP Microscaling (MX) v1.0 arithmetic of one block, on fp32 BIT PATTERNS only (tests/mx_model.py is the definition): the shared
// exponent of a block from its largest |v|, and the Q/DQ of one element, y = round_elem(v / 2^se) * 2^se.  Integer operations
// throughout, so the result does not depend on the code object's fp32 denormal mode: with se down to -127 both an input and an
// output may be fp32 subnormals (a = 2^-120 on E4M3: se = -127, and v = 2^-127 comes out as 1 * 2^-127), which a multiply would
// flush under a flushing mode.  Host and device: the same text is compiled into the host-side check of the rounding.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>   // __forceinline__, __clz
#define DPL_MX_HD __host__ __device__ __forceinline__
#else
#define DPL_MX_HD inline
#endif

namespace dpl_mx {

constexpr int kBlock32 = 32;   // elements per block

// The element formats: emax (the exponent of the largest value), mantissa bits, the exponent of the smallest normal value, and
// the mantissa field of the largest value as fp32 (E4M3: 448 = 1.75 * 2^8; E2M1: 6 = 1.5 * 2^2).
template <int ELEM>
struct Fmt;
template <>
struct Fmt<0> {   // DPL_MX_E4M3
    static constexpr int emax = 8, mbits = 3, emin = -6;
    static constexpr uint32_t top_mant = 0x600000u;
};
template <>
struct Fmt<1> {   // DPL_MX_E2M1
    static constexpr int emax = 2, mbits = 1, emin = 0;
    static constexpr uint32_t top_mant = 0x400000u;
};

DPL_MX_HD int clz32(uint32_t v) {   // 32 for 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)v);
#else
    return v ? __builtin_clz(v) : 32;
#endif
}

// a_bits: the largest |v| of the block as a bit pattern (sign cleared), finite and not 0.  floor(log2 a) is the exponent field,
// or for a subnormal the position of its leading bit; se = max(floor(log2 a) - emax, -127) (the upper clamp, 127, is out of
// reach: floor(log2 a) <= 127 and emax >= 2).
template <int ELEM>
DPL_MX_HD int shared_exponent(uint32_t a_bits) {
    const int field = (int)(a_bits >> 23);
    const int e = field ? field - 127 : (31 - clz32(a_bits)) - 149;
    const int se = e - Fmt<ELEM>::emax;
    return se < -127 ? -127 : se;
}

// b: |v| as a bit pattern, finite.  Returns |y| as a bit pattern.
//   |v| = M * 2^(ex - 150) with ex = max(exponent field, 1) and M the 24-bit significand (no implicit bit for a subnormal).  The
//   grid around |v| has step 2^(max(floor(log2 |v|), se + emin) - mbits): `sh` low bits of M are rounded away, half to even —
//   sh = max(position of M's leading bit - mbits, se + emin - mbits - (ex - 150)), never below 13 (ex = 1 meets se + emin - mbits
//   >= -136) and, at 25 or more, everything (M < 2^24 lies below half a step).  The rounded significand M' is 0, or lies in
//   [2^23, 2^24] for a normal |v| and in (0, 2^23] for a subnormal one, so ((ex - 1) << 23) + M' is the pattern of M' * 2^(ex -
//   150), a carry into the next binade included.  Saturation first: the largest value times 2^se is a normal fp32 (se + emax +
//   127 >= 2), and patterns of finite non-negative values order as the values do.
template <int ELEM>
DPL_MX_HD uint32_t round_bits(uint32_t b, int se) {
    typedef Fmt<ELEM> F;
    const uint32_t top = ((uint32_t)(se + F::emax + 127) << 23) | F::top_mant;
    b = b < top ? b : top;
    const uint32_t field = b >> 23;
    const int ex = field ? (int)field : 1;
    const uint32_t M = (b & 0x7FFFFFu) | (field ? 0x800000u : 0u);
    int sh = 31 - clz32(M) - F::mbits;
    const int sub = se + (F::emin - F::mbits + 150) - ex;
    sh = sh > sub ? sh : sub;
    sh = sh < 25 ? sh : 25;
    const uint32_t q = (M + (1u << (sh - 1)) - 1u + ((M >> sh) & 1u)) >> sh;
    const uint32_t Mr = q << sh;
    return Mr ? ((uint32_t)(ex - 1) << 23) + Mr : 0u;
}

}  // namespace dpl_mx
