// What the two kernels on v_mfma_scale_f32_16x16x128_f8f6f4 share (mx_gemm_kernels.hip: k_mx_gemm; mx_conv_kernels.hip: k_mx_conv):
// a lane's fragment of a K-INNERMOST packed MX operand, as dpl_mx_encode writes it.  The lane map (confirmed with
// exact data): lane l supplies row (column) l & 15 and, as its scale, the E8M0 byte of K-block l >> 4 of the 128-wide step.  Codes:
// E2M1 — the 32 K values of that same block, 16 bytes, byte j holding k = 2j in its low and k = 2j + 1 in its high nibble, the other
// four dwords 0.  E4M3 — NOT that block: dwords 0 .. 3 are k = 16 (l >> 4) .. + 15 of the step and dwords 4 .. 7 k = 64 + 16 (l >> 4)
// .. + 15, byte j of a run being k = j.  C/D: lane l holds column l & 15, rows 4 * (l >> 4) + reg.
#pragma once
#include "common.hpp"

namespace {

using i8v = __attribute__((ext_vector_type(8))) int;
using u4g = __attribute__((ext_vector_type(4))) uint32_t;
typedef const __attribute__((address_space(1))) u4g* gptr_u4g;
typedef const __attribute__((address_space(1))) uint8_t* gptr_u8g;
typedef __attribute__((address_space(1))) float* gptr_f32g;

constexpr uint32_t kMxGemmTile = 64;      // rows and columns of C per workgroup

template <int ELEM>
struct GemmOperand {
    static constexpr uint32_t block_bytes = ELEM == DPL_MX_E4M3 ? 32u : 16u;      // of one K-block's codes in the file
    static constexpr int fmt = ELEM == DPL_MX_E4M3 ? 0 : 4;                        // the instruction's format code (cbsz / blgp)
};

// Does a dword hold an E4M3 NaN byte (0x7F or 0xFF)?  (t's bytes are at most 0x7F: adding 1 carries into bit 7 only from 0x7F.)
__device__ __forceinline__ uint32_t e4m3_nan_in(uint32_t w) {
    return (((w & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u);
}

// One lane's fragment of one operand tile.
struct GemmFrag {
    i8v v;
    int scale;
};

// row: the operand's row this lane reads (already offset by the batch), live: it exists; kb0: the first K-block of the 128-wide
// step; q = lane >> 4.  By the map above: the scale byte of block kb0 + q; E2M1 — the 16 bytes of that block; E4M3 — half q & 1
// of block kb0 + (q >> 1) into the low four dwords and the same half of block kb0 + 2 + (q >> 1) into the high four.  A block past
// Kp / 32 leaves zeros (scale byte 127).
template <int ELEM>
__device__ __forceinline__ GemmFrag gemm_load(const uint8_t* codes, const uint8_t* scales, uint64_t row, uint32_t nblk, uint32_t kb0, uint32_t q,
                                              bool live, uint32_t& bad) {
    GemmFrag f;
    f.v = i8v{0, 0, 0, 0, 0, 0, 0, 0};
    f.scale = 127;
    const uint64_t blk0 = row * nblk;
    if constexpr (ELEM == DPL_MX_E4M3) {
        const uint32_t b_lo = kb0 + (q >> 1), b_hi = b_lo + 2u, half = (q & 1u) * 16u;
        if (live && b_lo < nblk) {
            const u4g lo = *(gptr_u4g)(codes + (blk0 + b_lo) * GemmOperand<ELEM>::block_bytes + half);
            f.v[0] = (int)lo.x, f.v[1] = (int)lo.y, f.v[2] = (int)lo.z, f.v[3] = (int)lo.w;
            bad |= e4m3_nan_in(lo.x) | e4m3_nan_in(lo.y) | e4m3_nan_in(lo.z) | e4m3_nan_in(lo.w);
        }
        if (live && b_hi < nblk) {
            const u4g hi = *(gptr_u4g)(codes + (blk0 + b_hi) * GemmOperand<ELEM>::block_bytes + half);
            f.v[4] = (int)hi.x, f.v[5] = (int)hi.y, f.v[6] = (int)hi.z, f.v[7] = (int)hi.w;
            bad |= e4m3_nan_in(hi.x) | e4m3_nan_in(hi.y) | e4m3_nan_in(hi.z) | e4m3_nan_in(hi.w);
        }
    } else {
        if (live && kb0 + q < nblk) {
            const u4g lo = *(gptr_u4g)(codes + (blk0 + kb0 + q) * GemmOperand<ELEM>::block_bytes);
            f.v[0] = (int)lo.x, f.v[1] = (int)lo.y, f.v[2] = (int)lo.z, f.v[3] = (int)lo.w;
        }
    }
    if (live && kb0 + q < nblk) {
        const uint32_t sc = ((gptr_u8g)scales)[blk0 + kb0 + q];
        bad |= sc == 0xFFu ? 1u : 0u;
        f.scale = (int)sc;
    }
    return f;
}

}  // namespace
