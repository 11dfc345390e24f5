// What the one-read OCTAV kernels (octav_tail.hpp: the streaming kernel and its walk; octav_rescue.hpp: the rescue walk) share
// below the level of a walk: the workgroup's shape and its static LDS block, the wave64 scans and sums by DPP, the suffix
// totals over the histogram's bins, the row loader of a list, and the row a refused pair leaves for its rescue.
#pragma once
#include <type_traits>
#include "common.hpp"
#include "octav_common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kOver = 4;                                         // rows of a list beyond the resident ones streamed per step of an iteration

// The workgroup's STATIC LDS (one struct for all three kernels: with four waves per SIMD its size is part of the occupancy)
struct Shared {
    double red_d[kWaves];
    unsigned long long red_q[kWaves];
    uint32_t red_a[kWaves], red_b[kWaves];
    unsigned long long part_m[2][kWaves];   // walk: the waves' partial (count, mantissa sum), two alternating slots
    uint32_t part_c[2][kWaves];
    float red_mn[kWaves], red_mx[kWaves];
    double low_sum;               // streaming kernel: non-zero values outside the window: their sum, count, a NaN among them
    uint32_t low_cnt, low_nan;
    uint32_t bm[kLogWords];       // rescue walk: the bins of the pair's bracket (their values were gathered)
    uint32_t pub[kLogWords];      // exact-tail walk: the bracket of a refused pair (bracket_marks)
    uint32_t would_list;          // ... and the values its marked bins hold (must fit the pair's region of the rescue list)
    uint32_t cursor;              // streaming kernel: entries of the slice's list region handed out so far
    uint32_t list_cap, region_cap;   // exact-tail form: values this workgroup's list part / the pair's whole list region holds
    uint32_t tail_j;              // exact-tail form (octav_tail.hpp): the bin at and above which values are listed (only ever raised)
    uint32_t jwant;               // ... and the bin this pair asks the tensor's next batches to list from
    // ... wave 0 walks alone; what it hands to the others (and to the pair's state) at the joints of the walk
    float t_s, w_s0, w_ud;
    int w_jb;
    uint32_t w_evals, w_exact, w_path, w_bad, w_route, w_lkn, w_lkc;
    double w_lks;
    uint32_t seg_off[kMaxCluster], seg_len[kMaxCluster];   // merge: the slices' list segments; rescue walk: [0] = the list's length
    OctavStep step;
    int jb;
    uint32_t bad, route;
    float s0, ud, w_s;
    double s_above;
    unsigned long long n_above, n_elems;
};

// The workgroup's range from its waves' (sh.red_mn / red_mx: stream_tail, or k_octav_tail_merge from the pair's state)
struct WgRange {
    float mn, mx;
};
__device__ __forceinline__ WgRange wg_range(const Shared& sh) {
    static_assert(kWaves == 4, "four waves' ranges");
    return {fminf(fminf(sh.red_mn[0], sh.red_mn[1]), fminf(sh.red_mn[2], sh.red_mn[3])),
            fmaxf(fmaxf(sh.red_mx[0], sh.red_mx[1]), fmaxf(sh.red_mx[2], sh.red_mx[3]))};
}

// wave64 inclusive prefix sums by DPP (Hillis-Steele inside each row of 16, then the two row broadcasts): VALU only — the
// ds_bpermute form (__shfl_up) is six dependent trips through the LDS pipeline per value, which inside the streaming kernel is
// full of the other workgroups' histogram atomics
__device__ __forceinline__ uint32_t scan_u32_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    return v;
}
__device__ __forceinline__ double scan_f64_dpp(double v) {
#define DPL_SCAN_STEP(ctrl, rmask, bound)                                                                              \
    {                                                                                                                  \
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);                                      \
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, ctrl, rmask, 0xF, bound);       \
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), ctrl, rmask, 0xF, bound); \
        v += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));                                   \
    }
    DPL_SCAN_STEP(0x111, 0xF, true)
    DPL_SCAN_STEP(0x112, 0xF, true)
    DPL_SCAN_STEP(0x114, 0xF, true)
    DPL_SCAN_STEP(0x118, 0xF, true)
    DPL_SCAN_STEP(0x142, 0xA, false)
    DPL_SCAN_STEP(0x143, 0xC, false)
#undef DPL_SCAN_STEP
    return v;
}
// wave64 sum by DPP (row-local butterflies, then the two row broadcasts): ~6 VALU instead of six dependent ds_bpermute round
// trips; the total arrives in lane 63 and is broadcast from there
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror: every lane holds its row's sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Raw per-bin (count, scaled sum) in n_ge / s_ge -> suffix totals in place (N_ge[j], S_ge[j] = everything in bins >= j).
// Thread t owns the 8 bins below 2047 - 8 t; all 256 threads; the raw values were written by their owners.
__device__ __forceinline__ void suffix_in_place(uint32_t* n_ge, double* s_ge, Shared& sh) {
    constexpr int kPerT = kLogNB / kThreads;
    const int hi = kLogNB - 1 - (int)threadIdx.x * kPerT;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    uint32_t ln = 0;
    double ls = 0.0;
    for (int q = 0; q < kPerT; ++q) {
        ln += n_ge[hi - q];
        ls += s_ge[hi - q];
    }
    const double is = scan_f64_dpp(ls);
    const uint32_t in = scan_u32_dpp(ln);
    if (lane == kWave - 1) {
        sh.red_d[w] = is;
        sh.red_a[w] = in;
    }
    __syncthreads();
    double rs = is - ls;
    uint32_t rn = in - ln;
    for (int q = 0; q < w; ++q) {
        rs += sh.red_d[q];
        rn += sh.red_a[q];
    }
    for (int q = 0; q < kPerT; ++q) {
        const int b = hi - q;
        rn += n_ge[b];
        rs += s_ge[b];
        n_ge[b] = rn;
        s_ge[b] = rs;
    }
    __syncthreads();
}

__device__ __forceinline__ double bin_sum(unsigned long long mant_explicit, uint32_t count, int b) {
    return (double)(mant_explicit + ((unsigned long long)count << 23)) * log_bin_scale(b);   // full 24-bit mantissas
}

// (the dynamic LDS block is addressed through address-space-3 pointers: ds_ instructions with constant offsets)
typedef __attribute__((address_space(3))) unsigned long long* lptr_u64;
typedef __attribute__((address_space(3))) uint32_t* lptr_u32;

// Rows row0 .. row0 + kN - 1 of a list of len values at lp -> dst: 1024 values per ROW, one 16-byte vector per thread.  Buffer
// loads: zero fill past the list's end (one descriptor per row: the range check leaves the SGPR offset out, so the row offset
// goes into the base).
template <int kN>
__device__ __forceinline__ void load_rows(f4 (&dst)[kN], const float* lp, uint32_t row0, uint32_t len) {
    const uint32_t voff = threadIdx.x << 4;
#pragma unroll
    for (int u = 0; u < kN; ++u) {
        const uint32_t e0 = (row0 + (uint32_t)u) << 10;
        const int nbytes = e0 < len ? (int)(min(len - e0, 1024u) << 2) : 0;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(lp + (e0 < len ? e0 : 0u)), 0, nbytes, 0x00020000);
        dst[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
    }
}

// The row of a rescued pair in the job's d_resc (kRescRow 64-bit words, octav_geometry.hpp): fp64 S_ge[kLogNB] | u32 N_ge[kLogNB],
// the suffix totals walk_tail leaves and walk_rescued starts from.  Word: (const) unsigned long long.
struct RescRow {
    template <class Word, class To>
    using like = std::conditional_t<std::is_const<Word>::value, const To, To>;
    template <class Word>
    static __device__ __forceinline__ like<Word, double>* s_ge(Word* resc, uint32_t pair) {
        return reinterpret_cast<like<Word, double>*>(resc + (uint64_t)pair * kRescRow);
    }
    template <class Word>
    static __device__ __forceinline__ like<Word, uint32_t>* n_ge(Word* resc, uint32_t pair) {
        return reinterpret_cast<like<Word, uint32_t>*>(resc + (uint64_t)pair * kRescRow + kLogNB);
    }
    static_assert(kRescRow * sizeof(unsigned long long) == kLogNB * (sizeof(double) + sizeof(uint32_t)), "the row holds both");
};

}  // namespace
