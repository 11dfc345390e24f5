// `--mx_scale_search`: the arithmetic of one block's choice between the floor-rule shared exponent se0 and se0 + 1
// (tests/mx_scale_model.py is the definition), on fp32 BIT PATTERNS as mx_format.hpp's: the two roundings (round_bits), the squared
// Q/DQ error of an element as an fp64 built from the patterns, the balanced tree that sums 32 of them, and the choice.  Host and
// device: the same text is compiled into tests/mx_search_host.cpp.
//   Exactness: v and y = round_elem(v / 2^se) * 2^se are fp32 values of one sign whose difference is a multiple of v's last place
//   and no larger than |v| (or y = 0): at most 25 significant bits, so v - y is exact in fp64 and so is its square (2^-298 .. 2^256:
//   normal fp64 values).  The sum is 31 fp64 additions in a fixed order; it must be compiled without contraction or reassociation
//   (-ffp-contract=off, no fast-math).
//   Denormal mode: an fp32 value becomes an fp64 as (fp64)(its integer significand) * 2^(its exponent), an integer conversion and a
//   product of normal fp64 values — no fp32 operation sees a subnormal.
#pragma once
#include "mx_format.hpp"

namespace dpl_mx {

DPL_MX_HD double f64_from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }

constexpr uint64_t kF64InfBits = 0x7FF0000000000000ull;

// bits: any finite fp32 pattern.  Its value as an fp64, exactly.
DPL_MX_HD double f32_bits_to_f64(uint32_t bits) {
    const uint32_t field = (bits >> 23) & 0xFFu;
    const int32_t M = (int32_t)((bits & 0x7FFFFFu) | (field ? 0x800000u : 0u));
    const int ex = field ? (int)field : 1;                                     // M * 2^(ex - 150)
    const double p = f64_from_bits((uint64_t)(ex - 150 + 1023) << 52);         // (ex - 150 >= -149: a normal fp64)
    const double r = (double)M * p;
    return (bits >> 31) ? -r : r;
}

// The highest shared exponent a block of this format may take: the largest element times 2^se must be an fp32 value.
template <int ELEM>
DPL_MX_HD int se_limit() {
    return 127 - Fmt<ELEM>::emax;
}

// The second candidate of a block whose floor-rule exponent is se0: se0 + 1, or se0 again where se0 + 1 is out of range — the two
// errors are then equal and the floor stays, which is the rule.
template <int ELEM>
DPL_MX_HD int upper_candidate(int se0) {
    return se0 < se_limit<ELEM>() ? se0 + 1 : se0;
}

// (v - Q/DQ(v))^2 under the shared exponent se; vbits finite.
template <int ELEM>
DPL_MX_HD double elem_sq_err(uint32_t vbits, double v, int se) {
    const uint32_t y = (vbits & 0x80000000u) | round_bits<ELEM>(vbits & 0x7FFFFFFFu, se);
    const double d = v - f32_bits_to_f64(y);
    return d * d;
}

// The sum of 32 (or any power of two of) values pushed in index order, as the balanced tree e = e[0::2] + e[1::2] repeated: level l
// holds the sum of a finished run of 2^l values until its right-hand neighbour arrives.  With the loop around push() unrolled every
// index is a constant.
struct TreeSum {
    double level[6];
    DPL_MX_HD void push(double t, uint32_t index) {
        int l = 0;
        for (uint32_t m = index; m & 1u; m >>= 1) t = level[l++] + t;
        level[l] = t;
    }
};

// One whole block on one thread (the host's form, and a column of the cols kernel's): v[32] patterns with +0.0 past a short block's
// end, a = the largest |v| pattern.  Returns the E8M0 byte; err[0] = the error at the floor, err[1] = at the chosen byte.
template <int ELEM>
DPL_MX_HD uint32_t search_block(const uint32_t* v, uint32_t a, double* err) {
    if (a >= 0x7F800000u) {
        err[0] = err[1] = f64_from_bits(kF64InfBits);
        return 0xFFu;
    }
    const int se0 = a == 0u ? -127 : shared_exponent<ELEM>(a), se1 = upper_candidate<ELEM>(se0);
    TreeSum t0, t1;
    for (uint32_t i = 0; i < 32u; ++i) {
        const double d = f32_bits_to_f64(v[i]);
        t0.push(elem_sq_err<ELEM>(v[i], d, se0), i);
        t1.push(elem_sq_err<ELEM>(v[i], d, se1), i);
    }
    const double e0 = t0.level[5], e1 = t1.level[5];
    const bool up = e1 < e0;
    err[0] = e0;
    err[1] = up ? e1 : e0;
    return (uint32_t)(se0 + 127) + (up ? 1u : 0u);
}

// A given scale byte: is the block a 0xFF block whatever its data (0xFF itself, or an exponent above the format's limit)?
template <int ELEM>
DPL_MX_HD bool given_byte_is_nan(uint32_t byte) {
    return byte > (uint32_t)(se_limit<ELEM>() + 127);
}

}  // namespace dpl_mx
