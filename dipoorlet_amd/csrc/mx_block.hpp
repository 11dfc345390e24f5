// What the MX block kernels share (mx_kernels.hip: the Q/DQ pair; mx_pack_kernels.hip: the element codes of --mx_pack;
// mx_search_kernels.hip: the scale search of --mx_scale_search, whose given-scale rule the first two read too), each defined once:
// the loads and stores of a lane's VEC values as bit patterns, a block's maximum inside its lane group, its shared exponent and
// scale byte, one element's Q/DQ, the decompositions of a launch into blocks — groups of lanes for contiguous blocks (MxRowsAt),
// slots or tiles for strided ones (MxColsAt, MxPackColsAt) — and the block walk on top of them: MxRowsLoad and MxColsLoad, the
// prologues that bring a lane's values into registers.  The host side — argument check, launch plan, dispatch — is mx_plan.hpp.
#pragma once
#include "common.hpp"
#include "mx_format.hpp"
#include "mx_plan.hpp"
#include "mx_search.hpp"

namespace {

typedef __attribute__((address_space(1))) float* gptr_f32w;
typedef __attribute__((address_space(1))) f4* gptr_f4w;
typedef __attribute__((address_space(1))) uint8_t* gptr_u8w;
typedef const __attribute__((address_space(1))) uint8_t* gptr_u8;

constexpr uint32_t kQuietNaN = 0x7FC00000u;
constexpr uint32_t kInfBits = 0x7F800000u;
static_assert(kMxRowsBlock == kBlock, "mx_plan.hpp plans the rows kernels for workgroups of kBlock threads");

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

// The E8M0 byte of a block (se, nan).
__device__ __forceinline__ uint8_t mx_scale_byte(int se, bool nan) { return nan ? 0xFFu : (uint8_t)(se + 127); }

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

// The prologue of a rows kernel: where the lane works in each of its kMxRowsIter groups, and — load() — its VEC values of each,
// every load issued before the first use.  A lane past the last group or past K in a short last block is not live: it reads
// nothing, holds +0.0 (0 to the block maximum) and writes nothing to the tensor.
template <int VEC>
struct MxRowsLoad {
    MxRowsAt<VEC> w;
    uint64_t n_groups;
    MxVec<VEC> v[kMxRowsIter];
    uint64_t at[kMxRowsIter];                          // the element offset row * K + col
    bool live[kMxRowsIter];
    __device__ __forceinline__ MxRowsLoad(uint64_t n_groups, uint32_t K, uint32_t nblk) : w(nblk), n_groups(n_groups) {
#pragma unroll
        for (int i = 0; i < kMxRowsIter; ++i) {
            uint64_t row;
            uint32_t col;
            w.at(i, nblk, row, col);
            live[i] = exists(i) && col < K;            // (K % VEC == 0: a vector that starts inside a row ends inside it)
            at[i] = row * K + col;
        }
    }
    __device__ __forceinline__ void load(const float* x) {
#pragma unroll
        for (int i = 0; i < kMxRowsIter; ++i) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[i].b[j] = 0u;
            if (live[i]) v[i] = mx_load<VEC>(x + at[i]);
        }
    }
    __device__ __forceinline__ uint64_t group(int i) const { return w.group(i); }
    __device__ __forceinline__ bool exists(int i) const { return group(i) < n_groups; }
    // lane 0 of a group with any live lane is live (col = blk * 32 < K): the one that stores what the block has one of
    __device__ __forceinline__ bool first(int i) const { return live[i] && w.lane == 0u; }
    // the block's byte of a GIVEN kernel, one per group in group order; 0 where `have` is false or the kernel derives its own
    template <bool GIVEN>
    __device__ __forceinline__ uint32_t given_byte(const uint8_t* bytes, int i, bool have) const {
        if constexpr (GIVEN)
            if (have) return ((gptr_u8)bytes)[group(i)];
        return 0u;
    }
};

// ---------------------------------------------------------------------------------------------- inner > 1
// Slot t of a cols launch is column group t % cs (cs = inner / VEC) of block (t / cs) % nblk of outer slice t / (cs * nblk): adjacent
// lanes own adjacent columns of the same rows.  The workgroup's first slot is decomposed once (64-bit, uniform), a lane's own with
// 32-bit divisions.
struct MxColsPos {
    uint64_t o;                                        // outer slice
    uint32_t kb, col;                                  // block along K, first column
    bool live;                                         // the lane has a block: one that has none returns before it uses the rest
    // the block of column col + j in [outer, nblk, inner] (dpl_fake_quant_mx's scales) and in the K-innermost [outer, inner, nblk]
    __device__ __forceinline__ uint64_t block(uint32_t nblk, uint32_t inner, int j = 0) const { return (o * nblk + kb) * inner + col + (uint32_t)j; }
    __device__ __forceinline__ uint64_t packed_block(uint32_t nblk, uint32_t inner, int j) const { return (o * inner + col + (uint32_t)j) * nblk + kb; }
    // the lane's slot, `vec` columns wide.  (Decomposed for a lane past the last slot too — it touches no memory: skipping it
    // there costs k_fake_quant_mx_cols<ELEM, 4, GIVEN>, which sits at 256 VGPRs, 20 bytes of scratch.)
    __device__ __forceinline__ void slot(uint64_t n_slots, uint32_t nblk, uint32_t cs, uint32_t vec) {
        const uint64_t t0 = (uint64_t)blockIdx.x * kMxColsBlock;
        live = t0 + threadIdx.x < n_slots;
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

template <int VEC>
struct MxColsAt : MxColsPos {
    __device__ __forceinline__ MxColsAt(uint64_t n_slots, uint32_t nblk, uint32_t cs) { slot(n_slots, nblk, cs, VEC); }
};

// Where a lane of a cols kernel of mx_pack_kernels.hip works.  One column to a lane (VEC = 1): the slots above — a wave is one
// K-block of 64 columns.  Four columns to a lane (VEC = 4): a wave is a TILE of four consecutive K-blocks of sixteen column groups,
// lane = 16 * (K-block in the tile) + column group: an fp32 access of the wave is four runs of 256 contiguous bytes (whole lines, as
// many as the slot form touches), and the four lanes that hold the four K-blocks of one column access one run of 128 (64)
// contiguous code bytes instead of four runs Kp bytes apart.  Tiles: [outer, ceil(nblk / 4), ceil(cs / 16)].
template <int VEC>
struct MxPackColsAt : MxColsPos {
    __device__ __forceinline__ MxPackColsAt(uint64_t n_slots, uint32_t nblk, uint32_t cs) {
        if constexpr (VEC == 1) {
            slot(n_slots, nblk, cs, 1);
        } else {
            const uint32_t nct = (cs + 15u) / 16u, nkt = (nblk + 3u) / 4u;
            const uint32_t r = blockIdx.x / nct, ct = blockIdx.x - r * nct;       // (the grid is below 2^31)
            const uint32_t ob = r / nkt, kt = r - ob * nkt;
            const uint32_t cg = ct * 16u + (threadIdx.x & 15u);
            o = ob;
            kb = kt * 4u + (threadIdx.x >> 4);
            col = cg * VEC;
            live = kb < nblk && cg < cs;
        }
    }
};

// The prologue of a cols kernel at either position type: the rows the lane's block has, the offset of its first element, and —
// load() — the block's 32 rows of VEC columns in registers (+0.0 past a short last block), each load coalesced across the lanes.
template <int VEC>
struct MxColsLoad {
    uint32_t rows, inner;
    uint64_t base;
    MxVec<VEC> v[32];
    __device__ __forceinline__ MxColsLoad(const MxColsPos& w, uint32_t K, uint32_t inner)
        : rows(min(32u, K - w.kb * 32u)), inner(inner), base((w.o * K + (uint64_t)w.kb * 32u) * inner + w.col) {}
    __device__ __forceinline__ uint64_t at(int r) const { return base + (uint64_t)r * inner; }      // element offset of row r
    __device__ __forceinline__ bool has(int r) const { return (uint32_t)r < rows; }
    __device__ __forceinline__ void load(const float* x) {
#pragma unroll
        for (int r = 0; r < 32; ++r) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[r].b[j] = 0u;
            if (has(r)) v[r] = mx_load<VEC>(x + at(r));
        }
    }
};

// The largest |v| pattern of column j of a loaded block.  A macro on purpose: taken inside a function, a method of the loader
// included, the compiler folds every maximum into the guarded load before it and waits for each load where it is issued (32 waits
// in place of one in the ISA of the VEC = 1 kernels; occupancy moves with it).
#define MX_COL_MAX(in, j)                                                                                        \
    ({                                                                                                           \
        uint32_t a_ = 0u;                                                                                        \
        _Pragma("unroll") for (int r_ = 0; r_ < 32; ++r_) a_ = max(a_, (in).v[r_].b[j] & 0x7FFFFFFFu);           \
        a_;                                                                                                      \
    })

}  // namespace
