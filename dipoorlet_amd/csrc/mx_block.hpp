// What the MX kernels share (mx_kernels.hip: the Q/DQ pair; mx_pack_kernels.hip: the element codes of --mx_pack;
// mx_search_kernels.hip: the scale search of --mx_scale_search, whose given-scale rule the first two read too): the loads and
// stores of a lane's VEC values as bit patterns, a block's maximum inside its lane group, its shared exponent, one element's Q/DQ,
// and the two decompositions of a launch into blocks — groups of lanes for contiguous blocks, slots for strided ones.
#pragma once
#include "common.hpp"
#include "mx_format.hpp"
#include "mx_search.hpp"

namespace {

typedef __attribute__((address_space(1))) float* gptr_f32w;
typedef __attribute__((address_space(1))) f4* gptr_f4w;
typedef __attribute__((address_space(1))) uint8_t* gptr_u8w;
typedef const __attribute__((address_space(1))) uint8_t* gptr_u8;

constexpr uint32_t kQuietNaN = 0x7FC00000u;
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr int kMxRowsIter = 4;        // groups per lane group of the rows kernels (all loads issued before the first use)
constexpr int kMxColsBlock = 64;      // threads per workgroup of the cols kernels: one wave (no cross-lane traffic)

template <int VEC>
struct MxVec {
    uint32_t b[VEC];
};

template <int VEC>
__device__ __forceinline__ MxVec<VEC> mx_load(const float* p) {
    MxVec<VEC> r;
    if constexpr (VEC == 4) {
        const f4 v = __builtin_nontemporal_load((gptr_f4)p);
        r.b[0] = __float_as_uint(v.x);
        r.b[1] = __float_as_uint(v.y);
        r.b[2] = __float_as_uint(v.z);
        r.b[3] = __float_as_uint(v.w);
    } else {
        r.b[0] = __float_as_uint(__builtin_nontemporal_load((gptr_f32)p));
    }
    return r;
}

template <int VEC>
__device__ __forceinline__ void mx_store(float* p, const MxVec<VEC>& r) {
    if constexpr (VEC == 4) {
        const f4 v = {__uint_as_float(r.b[0]), __uint_as_float(r.b[1]), __uint_as_float(r.b[2]), __uint_as_float(r.b[3])};
        __builtin_nontemporal_store(v, (gptr_f4w)p);
    } else {
        __builtin_nontemporal_store(__uint_as_float(r.b[0]), (gptr_f32w)p);
    }
}

// One element of a block whose largest |v| has the pattern `a` (`nan`: a is NaN or inf — E8M0 0xFF: every element NaN).
template <int ELEM>
__device__ __forceinline__ uint32_t mx_elem(uint32_t vbits, int se, bool nan) {
    const uint32_t y = (vbits & 0x80000000u) | dpl_mx::round_bits<ELEM>(vbits & 0x7FFFFFFFu, se);
    return nan ? kQuietNaN : y;
}

// se and the NaN flag of a block from its maximum pattern; an all-zero block: se = -127 (its zeros come out with their signs)
template <int ELEM>
__device__ __forceinline__ int mx_block_se(uint32_t a, bool& nan) {
    nan = a >= kInfBits;
    return (nan || a == 0u) ? -127 : dpl_mx::shared_exponent<ELEM>(a);
}

// se and the NaN flag of a block under a GIVEN scale byte (--mx_scale_search: tests/mx_scale_model.py): a block that holds a NaN or
// an infinity is a 0xFF block whatever the byte; so is one whose byte is 0xFF or names an exponent above the format's limit.
template <int ELEM>
__device__ __forceinline__ int mx_block_se_given(uint32_t a, uint32_t byte, bool& nan) {
    nan = a >= kInfBits || dpl_mx::given_byte_is_nan<ELEM>(byte);
    return nan ? -127 : (int)byte - 127;
}

// The largest |v| pattern of a block held by a group of 32 / VEC adjacent lanes, VEC values each: in every lane of the group.
template <int VEC>
__device__ __forceinline__ uint32_t mx_group_max(const MxVec<VEC>& v) {
    uint32_t a = 0u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) a = max(a, v.b[j] & 0x7FFFFFFFu);
#pragma unroll
    for (uint32_t o = 1; o < 32u / VEC; o <<= 1) a = max(a, (uint32_t)__shfl_xor((int)a, (int)o, kWave));
    return a;
}

// ---------------------------------------------------------------------------------------------- inner == 1
// Group g of a rows launch is block g % nblk of row g / nblk (nblk = ceil(K / 32)); a workgroup owns kMxRowsIter * 256 * VEC / 32
// consecutive groups.  The workgroup's first (row, block) comes from one 64-bit division on uniform values; a lane's own from a
// 32-bit one per group.
template <int VEC>
struct MxRowsAt {
    static constexpr uint32_t LPG = 32 / VEC;          // lanes per group
    static constexpr uint32_t GPI = kBlock / LPG;      // groups per iteration of the workgroup
    uint64_t g0, row0;
    uint32_t blk0, lane, sub;                          // sub: the lane's group within an iteration
    __device__ __forceinline__ MxRowsAt(uint32_t nblk) {
        g0 = (uint64_t)blockIdx.x * (GPI * kMxRowsIter);
        row0 = g0 / nblk;
        blk0 = (uint32_t)(g0 - row0 * nblk);
        lane = threadIdx.x % LPG;
        sub = threadIdx.x / LPG;
    }
    __device__ __forceinline__ uint64_t group(int i) const { return g0 + (uint32_t)i * GPI + sub; }
    // iteration i: the lane's row and first column (the column may lie past K in a short last block)
    __device__ __forceinline__ void at(int i, uint32_t nblk, uint64_t& row, uint32_t& col) const {
        const uint32_t b = blk0 + (uint32_t)i * GPI + sub, dr = b / nblk;
        row = row0 + dr;
        col = (b - dr * nblk) * 32u + lane * VEC;
    }
};

// ---------------------------------------------------------------------------------------------- inner > 1
// Slot t of a cols launch is column group t % cs (cs = inner / VEC) of block (t / cs) % nblk of outer slice t / (cs * nblk): adjacent
// lanes own adjacent columns of the same rows.  The workgroup's first slot is decomposed once (64-bit, uniform), a lane's own with
// 32-bit divisions.
struct MxColsAt {
    uint64_t o;                                        // outer slice
    uint32_t kb, col;                                  // block along K, first column
    __device__ __forceinline__ MxColsAt(uint32_t nblk, uint32_t cs, uint32_t vec) {
        const uint64_t t0 = (uint64_t)blockIdx.x * kMxColsBlock;
        const uint64_t r0 = t0 / cs;                   // (outer slice, block) of the workgroup's first slot, flattened
        const uint32_t c0 = (uint32_t)(t0 - r0 * cs);
        const uint64_t o0 = r0 / nblk;
        const uint32_t kb0 = (uint32_t)(r0 - o0 * nblk);
        const uint32_t c = c0 + threadIdx.x, dc = c / cs;
        col = (c - dc * cs) * vec;
        const uint32_t kb1 = kb0 + dc, dk = kb1 / nblk;
        kb = kb1 - dk * nblk;
        o = o0 + dk;
    }
};

}  // namespace
