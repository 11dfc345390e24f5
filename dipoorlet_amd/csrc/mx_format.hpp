// OCP Microscaling (MX) v1.0 arithmetic of one block, on fp32 BIT PATTERNS only (tests/mx_model.py is the definition): the shared
// exponent of a block from its largest |v|, and the Q/DQ of one element, y = round_elem(v / 2^se) * 2^se.  Integer operations
// throughout, so the result does not depend on the code object's fp32 denormal mode: with se down to -127 both an input and an
// output may be fp32 subnormals (a = 2^-120 on E4M3: se = -127, and v = 2^-127 comes out as 1 * 2^-127), which a multiply would
// flush under a flushing mode.  And, for `--mx_pack`, the step between such a y and its element code, both ways (encode_bits,
// decode_bits; tests/mx_pack_model.py is the definition).  Host and device: the same text is compiled into the host-side checks
// of the rounding and of the codes.
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

// The element formats: emax (the exponent of the largest value), mantissa bits, the exponent of the smallest normal value, the
// exponent bits of the code, and the mantissa field of the largest value as fp32 (E4M3: 448 = 1.75 * 2^8; E2M1: 6 = 1.5 * 2^2;
// E2M3: 7.5 = 1.875 * 2^2; E3M2: 28 = 1.75 * 2^4).  And what the packed form and the block-scaled MFMA key on: the bits a code takes
// in the file (a block of 32 is 4 * bits bytes: 32, 16 or 24), the code of every element of a 0xFF block, and the instruction's
// format code (cbsz / blgp).  The two FP6 formats (tests/mx_fp6_model.py) have no NaN or inf codes, like E2M1.
template <int ELEM>
struct Fmt;
template <>
struct Fmt<0> {   // DPL_MX_E4M3
    static constexpr int emax = 8, mbits = 3, emin = -6, ebits = 4;
    static constexpr uint32_t top_mant = 0x600000u, bits = 8u, nan_code = 0x7Fu;
    static constexpr int mfma = 0;
};
template <>
struct Fmt<1> {   // DPL_MX_E2M1
    static constexpr int emax = 2, mbits = 1, emin = 0, ebits = 2;
    static constexpr uint32_t top_mant = 0x400000u, bits = 4u, nan_code = 0u;
    static constexpr int mfma = 4;
};
template <>
struct Fmt<6> {   // DPL_MX_E2M3
    static constexpr int emax = 2, mbits = 3, emin = 0, ebits = 2;
    static constexpr uint32_t top_mant = 0x700000u, bits = 6u, nan_code = 0u;
    static constexpr int mfma = 2;
};
template <>
struct Fmt<7> {   // DPL_MX_E3M2
    static constexpr int emax = 4, mbits = 2, emin = -2, ebits = 3;
    static constexpr uint32_t top_mant = 0x600000u, bits = 6u, nan_code = 0u;
    static constexpr int mfma = 3;
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

// `--mx_gptq` (tests/mx_gptq_model.py keep_top_closed is the definition): a block rounded under a shared exponent se that is
// HIGHER than its own floor exponent stays a fixed point of the floor-rule Q/DQ only if its largest |y| is within the range of the
// finer grid.  E2M1's largest value ends its binade, so it always is.  E4M3's binade ends with 1.875 * 2^8, which the format does
// not have: a largest |y| of 1.875 * 2^t would be saturated to 1.75 * 2^t.  So a |y| with the significand 1.111b that would become
// the block's largest so far (m: the largest |y| pattern given out before in the block) gives way to the nearer of its two
// neighbours on the grid.  y = 15 u with u the value of its lowest set pattern bit; the neighbours are the patterns y - u and y + u
// (the carry into the exponent field is the next binade's 1.0; fp32 subnormals are contiguous with the normals).
//   b: |v| as a bit pattern; y: round_bits<ELEM>(b, se).  Returns the |y| to use.
template <int ELEM>
DPL_MX_HD uint32_t keep_top_closed(uint32_t b, uint32_t y, uint32_t m) {
    if (ELEM != 0) return y;
    const uint32_t u = y & (0u - y);
    const uint32_t sig = (y >> 23) ? ((y & 0x7FFFFFu) | 0x800000u) : y;
    const bool hit = y != 0u && sig == (u << 4) - u && y > m;
    return hit ? (b > y ? y + u : y - u) : y;
}

// The element codes of `--mx_pack` (tests/mx_pack_model.py is the definition): E4M3 is the OCP FP8 E4M3FN byte S.EEEE.MMM, E2M1 the
// four bits S.EE.M; both have the exponent bias 1 - emin and subnormals m * 2^(emin - mbits) under the exponent field 0.
//
// ybits: sign | round_bits<ELEM>(|v|, se) — a value of the element format times 2^se, finite.  Returns its code.
//   |y| = N * 2^(e - 23) with N the 24-bit significand normalised to [2^23, 2^24) (shifted up for an fp32 subnormal) and e its true
//   exponent; in units of 2^se the exponent is d = e - se, in [emin - mbits, emax].  A normal element (d >= emin) has the field
//   d - emin + 1 over the mbits bits below N's leading bit, which is ((d - emin) << mbits) + (N >> (23 - mbits)): the leading bit
//   carries the + 1.  A subnormal one is m = N >> (23 - mbits + emin - d).  Both in one expression; the shift is at most 23 on
//   such a ybits and is held to 31 on any other.
template <int ELEM>
DPL_MX_HD uint32_t encode_bits(uint32_t ybits, int se) {
    typedef Fmt<ELEM> F;
    const uint32_t b = ybits & 0x7FFFFFFFu;
    const uint32_t sign = (ybits >> 31) << (F::ebits + F::mbits);
    if (b == 0u) return sign;
    const uint32_t field = b >> 23;
    const int lead = field ? 23 : 31 - clz32(b);
    const uint32_t N = field ? ((b & 0x7FFFFFu) | 0x800000u) : b << (23 - lead);
    const int d = (field ? (int)field - 127 : lead - 149) - se - F::emin;      // the exponent above the smallest normal element's
    const int up = d > 0 ? d : 0;
    int sh = 23 - F::mbits + (up - d);
    sh = sh < 31 ? sh : 31;
    return sign | (((uint32_t)up << F::mbits) + (N >> sh));
}

// round_bits and encode_bits in one: the code of round_elem(|v| / 2^se) from b = |v| as a bit pattern, finite — what the encode
// kernels run per element (encode_bits(round_bits(b, se), se) without the way through y; tests/mx_codes_host.cpp holds the two to
// each other on every input it sees).  With round_bits' names: the rounded significand q counts steps of 2^(ex - 150 + sh), which
// in units of 2^se is the exponent (emin - mbits) + (sh - sub).  Where the subnormal step won (sh == sub, or everything rounded
// away), q itself is the code: m below 2^mbits, the exponent field 1 from its bit mbits on, 2 after a carry.  Where |v|'s own
// binade set the step (sh > sub), q lies in [2^mbits, 2^(mbits + 1)] and the code is ((sh - sub) << mbits) + q — its leading bit
// carries the field's + 1, a carry out of the mantissa the next field.
template <int ELEM>
DPL_MX_HD uint32_t round_code(uint32_t b, int se) {
    typedef Fmt<ELEM> F;
    const uint32_t top = ((uint32_t)(se + F::emax + 127) << 23) | F::top_mant;
    b = b < top ? b : top;
    const uint32_t field = b >> 23;
    const int ex = field ? (int)field : 1;
    const uint32_t M = (b & 0x7FFFFFu) | (field ? 0x800000u : 0u);
    const int lead_sh = 31 - clz32(M) - F::mbits;
    const int sub = se + (F::emin - F::mbits + 150) - ex;
    const int up = lead_sh > sub ? lead_sh - sub : 0;
    int sh = lead_sh > sub ? lead_sh : sub;
    sh = sh < 25 ? sh : 25;
    const uint32_t q = (M + (1u << (sh - 1)) - 1u + ((M >> sh) & 1u)) >> sh;
    return ((uint32_t)up << F::mbits) + q;
}

// code: any byte (E2M1: the low four bits are read); se in [-127, 127].  Returns the fp32 pattern of +-value * 2^se: exact — the
// smallest product, 2^(emin - mbits - 127) >= 2^-136, is an fp32 subnormal whose significand needs no rounding —, +-inf above
// fp32's range (se > 127 - emax only: never a pair the encoder emits), and the quiet NaN 0x7FC00000 for the two E4M3 NaN codes.
// (A scale byte of 0xFF makes the whole block NaN: the caller's.)
template <int ELEM>
DPL_MX_HD uint32_t decode_bits(uint32_t code, int se) {
    typedef Fmt<ELEM> F;
    const uint32_t sign = ((code >> (F::ebits + F::mbits)) & 1u) << 31;
    const uint32_t field = (code >> F::mbits) & ((1u << F::ebits) - 1u), m = code & ((1u << F::mbits) - 1u);
    if (ELEM == 0 && field == 15u && m == 7u) return 0x7FC00000u;
    if (field == 0u && m == 0u) return sign;
    const int lead = field ? F::mbits : 31 - clz32(m);                         // of (1.m) or (0.m) as an integer of mbits + 1 bits
    const uint32_t N = ((field ? (1u << F::mbits) : 0u) | m) << (23 - lead);  // [2^23, 2^24)
    const int e = (field ? (int)field : 1) + (F::emin - 1) + (lead - F::mbits) + se;
    if (e > 127) return sign | 0x7F800000u;
    if (e >= -126) return sign | ((uint32_t)(e + 127) << 23) | (N & 0x7FFFFFu);
    return sign | (N >> (-126 - e));                                           // (-126 - e <= 10; N's lowest set bit is at 20 or above)
}

}  // namespace dpl_mx
