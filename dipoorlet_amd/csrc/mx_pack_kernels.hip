// K7b: `--mx_pack` — an MX tensor as packed element codes and E8M0 scale bytes, and back (tests/mx_pack_model.py is the definition;
// mx_format.hpp round_code / decode_bits the arithmetic; mx_block.hpp what is shared with the Q/DQ pair of mx_kernels.hip: the
// block walk — MxRowsLoad, MxColsLoad over MxPackColsAt —, the block maximum, the shared exponent and its byte; mx_plan.hpp the
// argument check, the launch plan and the dispatch).  The tensor is fp32 [outer, K, inner], blocks of 32 along K.  Codes and scales are K-INNERMOST, the order a block-scaled GEMM reads both operands in: with nblk = ceil(K / 32),
// codes is [outer, inner, nblk * 32] bytes (E4M3), [outer, inner, nblk * 16] (E2M1: two to a byte, the even index along K in the
// low nibble) or [outer, inner, nblk * 24] (E2M3 / E3M2, tests/mx_fp6_model.py: a block's 32 codes are one little-endian string of 192
// bits, code i in bits [6 i, 6 i + 6)), scales [outer, inner, nblk].  For inner > 1 that is a transpose of the element order, and NOT the order of
// dpl_fake_quant_mx's scales ([outer, nblk, inner]).  The elements past K of a short last block get code 0.  A block is 32, 16
// or 24 bytes of codes at a multiple of its size: with a 16-byte aligned base every store and load of a 32- or 16-byte block is 16 bytes
// wide; a 24-byte block lies at a multiple of 8 and goes as three 8-byte vectors (Pack<ELEM>::wide, mx_store_block / mx_load_block).
// No atomics, no LDS, no scratch; 64-bit element indices.
//   k_mx_encode_rows  inner == 1: the lane groups of k_fake_quant_mx_rows (VEC = 4: 8 lanes a block, 16-byte loads; VEC = 1: 32
//                     lanes).  A lane's VEC codes are 32, 16, 8 or 4 bits (FP6: 24 or 6 — the group's first lane gathers eight runs of
//                     24 bits by __shfl_down and stores all 24 bytes); the lanes of a quad exchange them by DPP quad_perm
//                     broadcasts, quads by ds_bpermute (__shfl_xor / __shfl_down), and one lane in 4, 8, 16 or 32 stores 16 bytes.
//   k_mx_encode_cols  inner > 1: a lane owns VEC columns of one block and walks its 32 rows in registers, as k_fake_quant_mx_cols
//                     does; the 32 codes of a column are 8, 4 or 6 dwords, contiguous in the output, stored as 16-byte (FP6: 8-byte) vectors.
//                     The transpose is paid on the code side, 1/4 (1/8) of the bytes; with four columns to a lane a wave is a tile
//                     of four K-blocks, so that four lanes fill one run of a column (MxPackColsAt).
//   k_mx_decode_rows, k_mx_decode_cols  the mirrors: codes and scales in, fp32 [outer, K, inner] out, nothing written past K.
//   GIVEN (--mx_scale_search: dpl_mx_encode_scaled; tests/mx_scale_model.py) the encode kernels read a block's byte from
//   [outer, nblk, inner] instead of deriving it; the block maximum is still taken, for the non-finite rule (mx_block_se_given).
#include "mx_block.hpp"

namespace {

using u4 = __attribute__((ext_vector_type(4))) uint32_t;
typedef __attribute__((address_space(1))) u4* gptr_u4w;
typedef const __attribute__((address_space(1))) u4* gptr_u4;
typedef const __attribute__((address_space(1))) uint32_t* gptr_u32;
typedef const __attribute__((address_space(1))) uint16_t* gptr_u16;
using u2 = __attribute__((ext_vector_type(2))) uint32_t;
typedef __attribute__((address_space(1))) u2* gptr_u2w;
typedef const __attribute__((address_space(1))) u2* gptr_u2;

template <int ELEM>
struct Pack {
    static constexpr uint32_t bits = dpl_mx::Fmt<ELEM>::bits;             // per element: 8, 4 or 6
    static constexpr uint32_t block_bytes = 4u * bits;                    // 32 elements: 32, 16 or 24
    static constexpr uint32_t nan_code = dpl_mx::Fmt<ELEM>::nan_code;     // of every element of a 0xFF block
    static constexpr uint32_t words = block_bytes / 4u;                   // dwords of a block: 8, 4 or 6
    // 24 bytes are no multiple of 16: with a 16-byte aligned base an FP6 block lies at a multiple of 8, and the array of an odd
    // number of blocks ends 8 bytes short of a 16-byte boundary.  Its codes are stored and loaded as three 8-byte vectors.
    static constexpr bool wide = block_bytes % 16u == 0u;
};

// A block's dwords to / from dst / src (a multiple of the block's size past a 16-byte aligned base): 16-byte vectors, or for the
// 24-byte block 8-byte ones.  Nothing outside the block is touched.
template <int ELEM>
__device__ __forceinline__ void mx_store_block(uint8_t* dst, const uint32_t* wd) {
    if constexpr (Pack<ELEM>::wide) {
#pragma unroll
        for (uint32_t d = 0; d < Pack<ELEM>::words; d += 4) __builtin_nontemporal_store(u4{wd[d], wd[d + 1], wd[d + 2], wd[d + 3]}, (gptr_u4w)(dst + 4u * d));
    } else {
#pragma unroll
        for (uint32_t d = 0; d < Pack<ELEM>::words; d += 2) __builtin_nontemporal_store(u2{wd[d], wd[d + 1]}, (gptr_u2w)(dst + 4u * d));
    }
}
template <int ELEM>
__device__ __forceinline__ void mx_load_block(const uint8_t* src, uint32_t* wd) {
    if constexpr (Pack<ELEM>::wide) {
#pragma unroll
        for (uint32_t d = 0; d < Pack<ELEM>::words; d += 4) {
            const u4 t = __builtin_nontemporal_load((gptr_u4)(src + 4u * d));
            wd[d] = t.x, wd[d + 1] = t.y, wd[d + 2] = t.z, wd[d + 3] = t.w;
        }
    } else {
#pragma unroll
        for (uint32_t d = 0; d < Pack<ELEM>::words; d += 2) {
            const u2 t = __builtin_nontemporal_load((gptr_u2)(src + 4u * d));
            wd[d] = t.x, wd[d + 1] = t.y;
        }
    }
}

// Code r of a block (r, and so every shift, is a constant where the loop around it is unrolled) into / out of its dwords: the
// block is one little-endian bit string, a 6-bit code may straddle two dwords.
template <int ELEM>
__device__ __forceinline__ void mx_put_code(uint32_t* wd, uint32_t r, uint32_t c) {
    constexpr uint32_t BITS = Pack<ELEM>::bits;
    const uint32_t at = r * BITS, i = at / 32u, sh = at % 32u;
    wd[i] |= c << sh;
    if (sh + BITS > 32u) wd[i + 1u] |= c >> (32u - sh);
}
template <int ELEM>
__device__ __forceinline__ uint32_t mx_get_code(const uint32_t* wd, uint32_t r) {
    constexpr uint32_t BITS = Pack<ELEM>::bits;
    const uint32_t at = r * BITS, i = at / 32u, sh = at % 32u;
    uint32_t c = wd[i] >> sh;
    if (sh + BITS > 32u) c |= wd[i + 1u] << (32u - sh);
    return c & ((1u << BITS) - 1u);
}

// The code of element v of a block (se, nan); `exists`: false past K.
template <int ELEM>
__device__ __forceinline__ uint32_t mx_code(uint32_t vbits, int se, bool nan, bool exists) {
    const uint32_t c = ((vbits >> 31) << (dpl_mx::Fmt<ELEM>::ebits + dpl_mx::Fmt<ELEM>::mbits)) | dpl_mx::round_code<ELEM>(vbits & 0x7FFFFFFFu, se);
    return exists ? (nan ? Pack<ELEM>::nan_code : c) : 0u;
}

// v of lane J of the caller's quad (lanes 4q .. 4q + 3), in every lane of the quad: one DPP move.  All 64 lanes must be active.
template <int J>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xF, 0xF, true);     // quad_perm [J, J, J, J]
}

// A group of 32 / VEC lanes holds one block's codes, `pay` = the lane's VEC codes in its low VEC * bits bits, lowest index lowest.
// The group's 32 or 16 bytes go to dst as 16-byte stores, its 24 (FP6) as three 8-byte ones.  Called by every lane of the wave (the
// exchange reads lanes that store nothing); `go`: the group exists.
//
// FP6: the block is eight runs of 24 bits — a lane's own (VEC = 4: the group's 8 lanes) or a quad's (VEC = 1: its 8 quads).  The
// group's first lane takes the eight by __shfl_down and stores the block's six dwords.
template <int ELEM, int VEC>
__device__ __forceinline__ void mx_store_group_codes24(uint8_t* dst, uint32_t pay, uint32_t lane, bool go) {
    constexpr int S = VEC == 1 ? 4 : 1;                // lanes between two runs
    uint32_t h = pay;
    if constexpr (VEC == 1) h = quad_bcast<0>(pay) | (quad_bcast<1>(pay) << 6) | (quad_bcast<2>(pay) << 12) | (quad_bcast<3>(pay) << 18);
    uint32_t p[8];
    p[0] = h;
#pragma unroll
    for (int i = 1; i < 8; ++i) p[i] = (uint32_t)__shfl_down((int)h, S * i, kWave);
    uint32_t wd[6];
#pragma unroll
    for (int t = 0; t < 2; ++t) {                      // four runs are three dwords
        wd[3 * t] = p[4 * t] | (p[4 * t + 1] << 24);
        wd[3 * t + 1] = (p[4 * t + 1] >> 8) | (p[4 * t + 2] << 16);
        wd[3 * t + 2] = (p[4 * t + 2] >> 16) | (p[4 * t + 3] << 8);
    }
    if (go && lane == 0u) mx_store_block<ELEM>(dst, wd);
}

template <int ELEM, int VEC>
__device__ __forceinline__ void mx_store_group_codes(uint8_t* dst, uint32_t pay, uint32_t lane, bool go) {
    constexpr uint32_t W = VEC * Pack<ELEM>::bits;     // bits a lane holds: 32, 16, 8, 4 — FP6: 24, 6
    if constexpr (!Pack<ELEM>::wide) {
        mx_store_group_codes24<ELEM, VEC>(dst, pay, lane, go);
    } else {
        const uint32_t q0 = quad_bcast<0>(pay), q1 = quad_bcast<1>(pay), q2 = quad_bcast<2>(pay), q3 = quad_bcast<3>(pay);
        u4 out;
        uint32_t keep, off = 0u;                       // the lanes with lane % keep == 0 store, at byte `off`
        if constexpr (W == 32) {                       // a quad is 16 bytes
            out = u4{q0, q1, q2, q3};
            keep = 4u;
            off = (lane >> 2) * 16u;
        } else if constexpr (W == 16) {                // a quad is 8 bytes, the group's two quads 16
            const uint32_t d0 = q0 | (q1 << 16), d1 = q2 | (q3 << 16);
            out = u4{d0, d1, (uint32_t)__shfl_xor((int)d0, 4, kWave), (uint32_t)__shfl_xor((int)d1, 4, kWave)};
            keep = 8u;
        } else if constexpr (W == 8) {                 // a quad is a dword; four quads 16 bytes, the group's eight 32
            const uint32_t d = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
            out = u4{d, (uint32_t)__shfl_down((int)d, 4, kWave), (uint32_t)__shfl_down((int)d, 8, kWave), (uint32_t)__shfl_down((int)d, 12, kWave)};
            keep = 16u;
            off = (lane >> 4) * 16u;
        } else {                                       // a quad is 16 bits, two quads a dword, the group's eight quads 16 bytes
            const uint32_t h = q0 | (q1 << 4) | (q2 << 8) | (q3 << 12);
            const uint32_t d = h | ((uint32_t)__shfl_down((int)h, 4, kWave) << 16);
            out = u4{d, (uint32_t)__shfl_down((int)d, 8, kWave), (uint32_t)__shfl_down((int)d, 16, kWave), (uint32_t)__shfl_down((int)d, 24, kWave)};
            keep = 32u;
        }
        if (go && lane % keep == 0u) __builtin_nontemporal_store(out, (gptr_u4w)(dst + off));
    }
}

// The bytes a GIVEN encode kernel reads (--mx_scale_search: dpl_mx_encode_scaled), uint8 [outer, nblk, inner] — the order of
// dpl_fake_quant_mx's scales, not the K-innermost one the kernel writes.  The derived form carries nothing.
template <bool GIVEN>
struct MxGivenBytes {
    const uint8_t* p;
    __host__ __device__ const uint8_t* ptr() const { return p; }
};
template <>
struct MxGivenBytes<false> {
    __host__ __device__ const uint8_t* ptr() const { return nullptr; }
};

// ---------------------------------------------------------------------------------------------- encode, inner == 1
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kBlock) void k_mx_encode_rows(const float* x, uint8_t* codes, uint8_t* scales, uint64_t n_groups, uint32_t K,
                                                           uint32_t nblk, MxGivenBytes<GIVEN> given) {
    MxRowsLoad<VEC> in(n_groups, K, nblk);
    in.load(x);
    uint32_t byte[kMxRowsIter];                        // (inner == 1: the two orders are one; read by every lane whose group exists)
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) byte[i] = in.template given_byte<GIVEN>(given.ptr(), i, in.exists(i));
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint32_t a = mx_group_max<VEC>(in.v[i]);
        bool nan;
        const int se = GIVEN ? mx_block_se_given<ELEM>(a, byte[i], nan) : mx_block_se<ELEM>(a, nan);
        uint32_t pay = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) pay |= mx_code<ELEM>(in.v[i].b[j], se, nan, in.live[i]) << (Pack<ELEM>::bits * j);
        const uint64_t g = in.group(i);
        const bool go = in.exists(i);                  // (the pad lanes of a short last block are part of it: code 0)
        mx_store_group_codes<ELEM, VEC>(codes + g * Pack<ELEM>::block_bytes, pay, in.w.lane, go);
        if (go && in.w.lane == 0u) ((gptr_u8w)scales)[g] = mx_scale_byte(se, nan);
    }
}

// ---------------------------------------------------------------------------------------------- encode, inner > 1
template <int ELEM, int VEC, bool GIVEN = false>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_mx_encode_cols(const float* x, uint8_t* codes, uint8_t* scales, uint64_t n_slots, uint32_t K,
                                                                 uint32_t nblk, uint32_t inner, uint32_t cs, MxGivenBytes<GIVEN> given) {
    const MxPackColsAt<VEC> w(n_slots, nblk, cs);
    if (!w.live) return;
    MxColsLoad<VEC> in(w, K, inner);
    in.load(x);
    uint32_t a[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) a[j] = MX_COL_MAX(in, j);
    constexpr uint32_t NW = Pack<ELEM>::words;         // dwords of one column's block: 8, 4 or 6
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        bool nan;
        int se;
        if constexpr (GIVEN)
            se = mx_block_se_given<ELEM>(a[j], ((gptr_u8)given.p)[w.block(nblk, inner, j)], nan);
        else
            se = mx_block_se<ELEM>(a[j], nan);
        uint32_t wd[NW];
#pragma unroll
        for (uint32_t d = 0; d < NW; ++d) wd[d] = 0u;
#pragma unroll
        for (int r = 0; r < 32; ++r) mx_put_code<ELEM>(wd, (uint32_t)r, mx_code<ELEM>(in.v[r].b[j], se, nan, in.has(r)));
        const uint64_t blk = w.packed_block(nblk, inner, j);
        mx_store_block<ELEM>(codes + blk * Pack<ELEM>::block_bytes, wd);
        ((gptr_u8w)scales)[blk] = mx_scale_byte(se, nan);
    }
}

// ---------------------------------------------------------------------------------------------- decode
template <int ELEM>
__device__ __forceinline__ uint32_t mx_decode_code(uint32_t code, uint32_t sc) {
    return sc == 0xFFu ? kQuietNaN : dpl_mx::decode_bits<ELEM>(code, (int)sc - 127);
}

// inner == 1: the groups of the encoder; a lane reads its VEC codes (32 or 16 bits at once for VEC = 4, the byte that holds it for
// VEC = 1; FP6: the dword that holds the first of its 24 or 6 bits and, where they run over, the next one) and its block's scale
// byte, and writes VEC floats.
template <int ELEM, int VEC>
__global__ __launch_bounds__(kBlock) void k_mx_decode_rows(const uint8_t* codes, const uint8_t* scales, float* y, uint64_t n_groups, uint32_t K,
                                                           uint32_t nblk) {
    constexpr uint32_t BITS = Pack<ELEM>::bits;
    const MxRowsLoad<VEC> out(n_groups, K, nblk);      // (where the lane writes: nothing is loaded from the fp32 side)
    uint32_t pay[kMxRowsIter], sc[kMxRowsIter];
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        const uint64_t g = out.group(i);
        pay[i] = sc[i] = 0u;
        if (out.live[i]) {
            const uint8_t* blk = codes + g * Pack<ELEM>::block_bytes;
            if constexpr (BITS == 6) {
                // the lane's 24 or 6 bits start at bit lane * VEC * 6 of the block: the dword that holds the first, and the next
                // one where they run over — which is then inside the block (the last bit is below 192)
                const uint32_t at = out.w.lane * VEC * BITS, sh = at % 32u;
                gptr_u32 dw = (gptr_u32)blk + at / 32u;
                const uint32_t lo = dw[0], hi = sh + VEC * BITS > 32u ? dw[1] : 0u;
                pay[i] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
            } else {
                const uint8_t* src = blk + out.w.lane * VEC * BITS / 8u;
                if constexpr (VEC * BITS == 32)
                    pay[i] = *(gptr_u32)src;
                else if constexpr (VEC * BITS == 16)
                    pay[i] = *(gptr_u16)src;
                else
                    pay[i] = (uint32_t)(*(gptr_u8)src) >> (out.w.lane * BITS % 8u);
            }
            sc[i] = ((gptr_u8)scales)[g];
        }
    }
#pragma unroll
    for (int i = 0; i < kMxRowsIter; ++i) {
        if (out.live[i]) {
            MxVec<VEC> r;
#pragma unroll
            for (int j = 0; j < VEC; ++j) r.b[j] = mx_decode_code<ELEM>((pay[i] >> (BITS * j)) & ((1u << BITS) - 1u), sc[i]);
            mx_store<VEC>(y + out.at[i], r);
        }
    }
}

// inner > 1: the slots of the encoder; a lane reads the blocks of its VEC columns (16-byte loads) and their scale bytes, and writes
// the block's rows that exist, each store coalesced across the lanes.
template <int ELEM, int VEC>
__global__ __launch_bounds__(kMxColsBlock, 2) void k_mx_decode_cols(const uint8_t* codes, const uint8_t* scales, float* y, uint64_t n_slots,
                                                                 uint32_t K, uint32_t nblk, uint32_t inner, uint32_t cs) {
    constexpr uint32_t NW = Pack<ELEM>::words;
    const MxPackColsAt<VEC> w(n_slots, nblk, cs);
    if (!w.live) return;
    const MxColsLoad<VEC> out(w, K, inner);            // (as above)
    uint32_t wd[VEC][NW], sc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const uint64_t blk = w.packed_block(nblk, inner, j);
        mx_load_block<ELEM>(codes + blk * Pack<ELEM>::block_bytes, wd[j]);
        sc[j] = ((gptr_u8)scales)[blk];
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if (out.has(r)) {
            MxVec<VEC> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                o.b[j] = mx_decode_code<ELEM>(mx_get_code<ELEM>(wd[j], (uint32_t)r), sc[j]);
            mx_store<VEC>(y + out.at(r), o);
        }
    }
}

// ---------------------------------------------------------------------------------------------- launches
// (fp: the fp32 side's base, d_x of encode and d_y of decode; the VEC = 4 cols kernels take the tile grid)
template <bool GIVEN>
int mx_encode_launch(const char* who, int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_codes, uint8_t* d_scales,
                     MxGivenBytes<GIVEN> given, dpl_stream_t s) {
    MxPlan p;
    if (const int rc = mx_plan(p, who, (uintptr_t)d_x, outer, k, inner, true)) return rc;
    return mx_dispatch_all(elem, inner == 1, p.vec, [&](auto E, auto ROWS, auto VEC) {
        if constexpr (ROWS) {
            hipLaunchKernelGGL((k_mx_encode_rows<E, VEC, GIVEN>), dim3((unsigned)p.blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_codes, d_scales, p.n,
                               p.K, p.nblk, given);
            DPL_LAUNCH_CHECK("k_mx_encode_rows");
        } else {
            hipLaunchKernelGGL((k_mx_encode_cols<E, VEC, GIVEN>), dim3((unsigned)p.blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_x, d_codes, d_scales,
                               p.n, p.K, p.nblk, (uint32_t)inner, p.cs, given);
            DPL_LAUNCH_CHECK("k_mx_encode_cols");
        }
        return 0;
    });
}

int mx_decode_launch(const char* who, int32_t elem, const uint8_t* d_codes, const uint8_t* d_scales, uint64_t outer, uint64_t k, uint64_t inner,
                     float* d_y, dpl_stream_t s) {
    MxPlan p;
    if (const int rc = mx_plan(p, who, (uintptr_t)d_y, outer, k, inner, true)) return rc;
    return mx_dispatch_all(elem, inner == 1, p.vec, [&](auto E, auto ROWS, auto VEC) {
        if constexpr (ROWS) {
            hipLaunchKernelGGL((k_mx_decode_rows<E, VEC>), dim3((unsigned)p.blocks), dim3(kBlock), 0, (hipStream_t)s, d_codes, d_scales, d_y, p.n, p.K,
                               p.nblk);
            DPL_LAUNCH_CHECK("k_mx_decode_rows");
        } else {
            hipLaunchKernelGGL((k_mx_decode_cols<E, VEC>), dim3((unsigned)p.blocks), dim3(kMxColsBlock), 0, (hipStream_t)s, d_codes, d_scales, d_y, p.n,
                               p.K, p.nblk, (uint32_t)inner, p.cs);
            DPL_LAUNCH_CHECK("k_mx_decode_cols");
        }
        return 0;
    });
}

constexpr const char* kPackPtrs = "the tensor, d_codes and d_scales";

}  // namespace

extern "C" int dpl_mx_encode(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, uint8_t* d_codes, uint8_t* d_scales,
                             dpl_stream_t s) {
    int rc;
    if (mx_check(rc, "dpl_mx_encode", elem, kPackPtrs, {d_x, d_codes, d_scales}, outer, k, inner, true, d_codes)) return rc;
    return mx_encode_launch("dpl_mx_encode", elem, d_x, outer, k, inner, d_codes, d_scales, MxGivenBytes<false>{}, s);
}

extern "C" int dpl_mx_encode_scaled(int32_t elem, const float* d_x, uint64_t outer, uint64_t k, uint64_t inner, const uint8_t* d_scales_in,
                                    uint8_t* d_codes, uint8_t* d_scales_out, dpl_stream_t s) {
    int rc;
    if (mx_check(rc, "dpl_mx_encode_scaled", elem, kPackPtrs, {d_x, d_codes, d_scales_out}, outer, k, inner, true, d_codes)) return rc;
    if (d_scales_in == nullptr) return fail_msg("dpl_mx_encode_scaled: d_scales_in must not be null");
    return mx_encode_launch("dpl_mx_encode_scaled", elem, d_x, outer, k, inner, d_codes, d_scales_out, MxGivenBytes<true>{d_scales_in}, s);
}

extern "C" int dpl_mx_decode(int32_t elem, const uint8_t* d_codes, const uint8_t* d_scales, uint64_t outer, uint64_t k, uint64_t inner,
                             float* d_y, dpl_stream_t s) {
    int rc;
    if (mx_check(rc, "dpl_mx_decode", elem, kPackPtrs, {d_y, d_codes, d_scales}, outer, k, inner, true, d_codes)) return rc;
    return mx_decode_launch("dpl_mx_decode", elem, d_codes, d_scales, outer, k, inner, d_y, s);
}
