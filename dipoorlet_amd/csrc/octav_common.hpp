// Shared by the OCTAV translation units (octav_kernels.hip: full / compaction / two-read bracket forms and the rescue's
// gather; octav_tail_host.hip: the launchers of the one-read exact-tail form, whose kernels are in octav_tail.hpp and
// octav_rescue.hpp): the fixed-point step, the states a pair is initialised and restarted in, the log-scale histogram
// geometry, the bracket walk over its bin edges, the tile walker, and what the two translation units call of each other.
// The numbers the host planning shares with the kernels (bins, slice and list-region sizes: list_cap_of) are in
// octav_geometry.hpp.
#pragma once
#include "common.hpp"
#include "octav_geometry.hpp"

#pragma clang fp contract(off)

namespace {

// One fixed-point step (forward_net.py:326-330): s' = fl32(sum) / fl32(c/unsigned * cnt_le + cnt_gt) — the python-float
// denominator is cast to float32 for the divide (NEP 50); |s' - s| < 1e-6 stops KEEPING the previous s.
struct OctavStep {
    float s;
    uint32_t iters, done, decreased;
};
__device__ __forceinline__ OctavStep octav_step(double sum, unsigned long long cnt_gt, unsigned long long cnt_le,
                                                float unsigned_div, float s, uint32_t iters, int max_iters) {
    const double c = 1.0 / 65536.0 / 3.0 / (double)unsigned_div;
    const double denom = c * (double)(long long)cnt_le + (double)(long long)cnt_gt;
    const float s1 = __fdiv_rn((float)sum, (float)denom);
    OctavStep r{s, iters, 0u, 0u};
    if (fabsf(__fsub_rn(s1, s)) < 1e-6f) {
        r.done = 1u;
    } else {
        r.decreased = !(s1 >= s) ? 1u : 0u;
        r.s = s1;
        r.iters = iters + 1u;
        if ((int)r.iters >= max_iters || s1 != s1) r.done = 1u;
    }
    return r;
}

// The two states every form writes, each in ONE place.  (Macros over a state `z`, not functions: a local state handed to a
// function by reference stays in memory until the call is inlined, which is after the compiler's first scalarisation, and the
// streaming kernel's last block then comes out in another order than the one it has been measured in.)
//
// The state of a pair (or the control block) no kernel has touched yet, in the histogram forms' mode: what k_octav_init (with
// the mode of the form it serves) and k_octav_tail_init store, and what the one-read walk fills its result into.
#define DPL_OCTAV_FRESH(z)                                                                                           \
    do {                                                                                                             \
        (z).sum = 0.0;                                                                                               \
        (z).cnt_gt = 0;                                                                                              \
        (z).cnt_le = 0;                                                                                              \
        (z).min_enc = 0xFFFFFFFFu; /* (the empty range) */                                                           \
        (z).max_enc = 0u;                                                                                            \
        (z).nan_seen = 0u;                                                                                           \
        (z).done = 0u;                                                                                               \
        (z).s = 0.0f;                                                                                                \
        (z).unsigned_div = 1.0f;                                                                                     \
        (z).iters = 0u;                                                                                              \
        (z).mode = 2u;                                                                                               \
        (z).n_elems = 0ull;                                                                                          \
        (z).len[0] = 0u;                                                                                             \
        (z).len[1] = 0u;                                                                                             \
        (z).cur = 2u; /* (no list yet) */                                                                            \
        (z).reserved = 0u;                                                                                           \
    } while (0)

// A pair that a histogram form could not finish RESTARTS ON THE COMPACTION ROUTE from s_0: list mode, and one more pair in the
// control block's cnt_le (what the route's kernels look at before they do anything).  k_octav_compact_full expects the state
// that k_octav_update<true> leaves: s = s_0, done = iters = 0, both lists empty (len = {0, 0}, cur = 2), the three accumulators
// zero.  `dirty` (a constant): the fields of that state the caller's form has written since — only they are stored, the others
// still hold it.
enum : uint32_t { kDirtyIters = 1u, kDirtyDone = 2u, kDirtyList0 = 4u, kDirtyList1 = 8u };
#define DPL_OCTAV_RESTART_COMPACTION(z, ctl, dirty)                                                                  \
    do {                                                                                                             \
        (z).mode = 1u;                                                                                               \
        if ((dirty) & kDirtyIters) (z).iters = 0u;                                                                   \
        if ((dirty) & kDirtyDone) (z).done = 0u;                                                                     \
        if ((dirty) & kDirtyList0) (z).len[0] = 0u;                                                                  \
        if ((dirty) & kDirtyList1) {                                                                                 \
            (z).len[1] = 0u;                                                                                         \
            (z).cur = 2u;                                                                                            \
        }                                                                                                            \
        atomicAdd(reinterpret_cast<unsigned long long*>(&(ctl)->cnt_le), 1ull);                                      \
    } while (0)

constexpr int kLogShift = 17;                               // 23 - 6: six mantissa bits per bin
constexpr uint32_t kLogKey0 = (uint32_t)(127 - 18) << 6;    // key of 2^-18
constexpr int kBitmapRow = kLogWords + 2;                   // + the gather range [lo, hi) as float bits
constexpr int kLogMaxMarked = 256;
constexpr uint32_t kSmallPair = 16384;                      // pairs this small are gathered whole
constexpr uint32_t kRescueUnit = 16384;                     // elements of a pair one workgroup of k_octav_rescue_gather re-reads
constexpr unsigned kRescueGrid = 512;                       // workgroups of the rescue's persistent kernels (gather and walk)

__device__ __forceinline__ int log_bin(float a) {
    const int b = (int)(__float_as_uint(a) >> kLogShift) - (int)kLogKey0;
    return b < 0 ? 0 : (b > kLogNB - 1 ? kLogNB - 1 : b);
}
__device__ __forceinline__ double log_bin_scale(int b) {   // 2^(e - 150) for the exponent field e of bin b
    const int e = (int)(((uint32_t)b + kLogKey0) >> 6);
    return __longlong_as_double((long long)(e - 150 + 1023) << 52);
}

// One 64-bit LDS atomic per element: the bin word holds the count in bits 43..62 and the mantissa sum in bits
// 0..42 (a sub-span has < 2^20 elements, an explicit mantissa is < 2^23: neither field can overflow into the other).
constexpr int kPackShift = 43;   // count: bits 43..62 (a slice has < 2^20 elements), bit 63 stays free for the gather flag
constexpr unsigned long long kPackMask = (1ull << kPackShift) - 1ull;


__device__ __forceinline__ float log_edge(int b) {  // lower edge of bin b (bin 0 starts at 0)
    return b <= 0 ? 0.0f : __uint_as_float(((uint32_t)b + kLogKey0) << kLogShift);
}


// s_0 and the bracket walk of one pair (one thread).  n_ge[j] / s_ge[j] = exact count / sum of the window values in
// bins >= j (entries 1 .. kLogNB-1 are read); sum_out / nz_out = the directly accumulated nonzero values outside the
// binned window.  Marks in bm[kLogWords] (zeroed by the caller) the bins the true iterates can fall into.
//   route 0: the pair is finished already (NaN iterate, or no iterations asked for)
//   route 2: bracket route — gather the marked bins [jmin, jmax], then walk the exact iteration
//   route 1: compaction route (values >= 2^14 or inf, a bracket that leaves the window or marks too many bins)
struct BracketResult {
    float s0, unsigned_div;
    uint32_t route;
    int jmin, jmax;
};
// The bracket walk proper: from s_0 (finite) over the bin edges, marking in bm[kLogWords] (zeroed by the caller) the bins
// the true iterates can fall into.  Returns route 2 (marks valid, bins [jmin, jmax]) or 1 (the bracket leaves the window
// or marks more than kLogMaxMarked bins: such a pair belongs on the compaction route).
__device__ __forceinline__ BracketResult bracket_marks(const uint32_t* n_ge, const double* s_ge, uint32_t* bm, float s0,
                                                       float ud, unsigned long long n) {
    BracketResult out;
    out.s0 = s0;
    out.unsigned_div = ud;
    out.jmin = kLogNB;
    out.jmax = -1;
    uint32_t r = 2u;
    const double c = 1.0 / 65536.0 / 3.0 / (double)ud;
    double lo = (double)s0, hi = (double)s0;
    int marked = 0;
    for (int itn = 0; itn < 20 && r == 2u; ++itn) {
        const int jl = log_bin((float)lo), jh = log_bin((float)hi);
        if (jl <= 1 || jh >= kLogNB - 2 || !(lo == lo) || !(hi == hi)) {
            r = 1u;
            break;
        }
        // Mark exactly the bins of the bracket, no margin.  Within a bin F(s) moves monotonically between its
        // values at the two edges unless the bin contains F itself (dropping a value v raises F iff v < F),
        // i.e. only at the fixed point, where the excursion beyond the edge values is second order; together
        // with the fp32 rounding of the true iterate that can put an iterate one bin outside the bracket
        // with a probability of order 1e-4 per pair.  The exact walk verifies every iterate and such a pair
        // simply finishes on the compaction route; a margin bin on either side would more than double the
        // values gathered (2.2 % -> 4.9 % on ResNet-50 activations) to avoid that.
        for (int w0 = jl >> 5; w0 <= jh >> 5; ++w0) {   // one LDS read-modify-write per word
            const int lo_b = max(jl, w0 << 5) & 31, hi_b = min(jh, (w0 << 5) + 31) & 31;
            const uint32_t mask = (0xFFFFFFFFu >> (31 - hi_b)) & (0xFFFFFFFFu << lo_b);
            const uint32_t old = bm[w0];
            bm[w0] = old | mask;
            marked += __popc(mask & ~old);
        }
        out.jmin = jl < out.jmin ? jl : out.jmin;
        out.jmax = jh > out.jmax ? jh : out.jmax;
        if (marked > kLogMaxMarked) {
            r = 1u;
            break;
        }
        double nlo = INFINITY, nhi = -INFINITY;
        for (int j = jl; j <= jh + 1; ++j) {  // F with everything in bins >= j counted as "above"
            // An edge above every value of the pair is no bound: no iterate reaches it (F is a mean of the pair's values), and F
            // there — 0 — would drag the bracket down to the bottom of the window.  Seen on erf outputs, whose values pile up
            // just below 1: the iteration ends inside that top bin.  (An iterate that does fall below the marked bins — few
            // values above it — is caught by the exact walk like any other.)
            if (n_ge[j] == 0u) continue;
            const double ng = (double)n_ge[j];
            const double f = s_ge[j] / (c * ((double)(long long)n - ng) + ng);
            nlo = fmin(nlo, f);
            nhi = fmax(nhi, f);
        }
        if (!(nlo <= nhi)) break;           // nothing above the bracket's bins at all
        if (nlo == lo && nhi == hi) break;  // the bracket stopped moving
        lo = nlo;
        hi = nhi;
    }
    out.route = r;
    return out;
}

__device__ __forceinline__ BracketResult bracket_walk(const uint32_t* n_ge, const double* s_ge, uint32_t* bm, float mn,
                                                      float mx, bool nan_seen, double sum_out,
                                                      unsigned long long nz_out, unsigned long long n, int dynamic_sym,
                                                      int max_iters) {
    // forward_net.py:319 — np.abs(data_min - 0) < 1e-6 (float32 compare) and 'dynamic_sym' in qi_params
    const float ud = (dynamic_sym && fabsf(mn) < 1e-6f && !nan_seen) ? 4.0f : 1.0f;
    // forward_net.py:324 — sum(|x|) / count(|x| > 0): exact window totals + the out-of-window part
    const float s0 = nan_seen ? __uint_as_float(0x7FC00000u)
                              : __fdiv_rn((float)(sum_out + s_ge[1]), (float)(long long)(nz_out + n_ge[1]));
    const float max_abs = fmaxf(fabsf(mn), fabsf(mx));
    BracketResult out;
    out.s0 = s0;
    out.unsigned_div = ud;
    out.jmin = kLogNB;
    out.jmax = -1;
    out.route = 2u;
    if (s0 != s0 || max_iters <= 0) {
        out.route = 0u;  // NaN is a fixed point of the iteration
    } else if (!(max_abs < log_edge(kLogNB))) {
        out.route = 1u;  // values at or above 2^14 (or inf): outside the exactly-summed window
    } else if (n <= (unsigned long long)kSmallPair) {
        for (int q = 0; q < kLogWords; ++q) bm[q] = 0xFFFFFFFFu;  // gather the whole (small) pair's window
        out.jmin = 0;
        out.jmax = kLogNB - 1;
    } else {
        out = bracket_marks(n_ge, s_ge, bm, s0, ud, n);
    }
    return out;
}

__device__ __forceinline__ void load_tile(const float* __restrict__ p_generic, uint32_t base, uint32_t n, bool aligned,
                                          f4 (&v)[4]) {
    gptr_f32 p = (gptr_f32)p_generic;
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t idx = base + u * 256 + lane * 4;
        if (aligned && idx + 3 < n) {
            v[u] = __builtin_nontemporal_load((gptr_f4)(p + idx));
        } else {  // zeros never survive (s >= 0)
            v[u].x = idx + 0 < n ? p[idx + 0] : 0.0f;
            v[u].y = idx + 1 < n ? p[idx + 1] : 0.0f;
            v[u].z = idx + 2 < n ? p[idx + 2] : 0.0f;
            v[u].w = idx + 3 < n ? p[idx + 3] : 0.0f;
        }
    }
}

// Tile walker for the compaction-style kernels: wave w of the workgroup takes the 1024-element tiles
// w, w + waves, ... of p[0..n).  Full tiles of an aligned span go through a branch-free, software-pipelined
// loop (two register sets; the next tile's four 16-byte loads are in flight while the current tile is
// consumed); the ragged end (< one workgroup tile) or an unaligned span uses the bounds-checked loader, which
// pads with zeros.  eat(v, tile_base, full): `full` tells the consumer that no element is padding.
template <int kThreads, class Eat>
__device__ __forceinline__ void for_each_tile(const float* __restrict__ p, uint32_t n, Eat&& eat) {
    const uint32_t w = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    constexpr uint32_t kStep = kThreads * 16;
    const bool aligned = (((uintptr_t)p) & 15u) == 0;
    const uint32_t n_main = aligned ? (n / kStep) * kStep : 0u;
    gptr_f4 pv = (gptr_f4)p;
#define DPL_TLOAD(buf, t0)                                                                  \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) buf[u] = __builtin_nontemporal_load(pv + ((t0) >> 2) + u * 64 + lane)
    uint32_t tile = w * 1024;
    if (tile < n_main) {
        f4 A[4], B[4];
        DPL_TLOAD(A, tile);
        for (;;) {
            uint32_t nxt = tile + kStep;
            if (nxt >= n_main) {
                eat(A, tile, true);
                break;
            }
            DPL_TLOAD(B, nxt);
            eat(A, tile, true);
            tile = nxt;
            nxt = tile + kStep;
            if (nxt >= n_main) {
                eat(B, tile, true);
                break;
            }
            DPL_TLOAD(A, nxt);
            eat(B, tile, true);
            tile = nxt;
        }
    }
#undef DPL_TLOAD
    for (uint32_t t2 = n_main + w * 1024; t2 < n; t2 += kStep) {
        f4 v[4];
        load_tile(p, t2, n, aligned, v);
        eat(v, t2, false);
    }
}

}  // namespace

// ---- what octav_kernels.hip defines and octav_tail_host.hip launches as well
extern int g_exact_fail_every, g_rescue_fail_every;   // dpl_test_hook_exact_fail_every / _rescue_fail_every
// the gather pass of the one-read form's rescue (k_octav_rescue_gather)
int dpl_octav_rescue_gather_launch(const uint32_t* d_missed, dpl_octav_state* d_states, int64_t n_pairs, const dpl_span* d_pair_spans,
                                   const float* const* d_seg_ptrs, const uint32_t* d_bm_rows, const uint64_t* d_pair_base,
                                   float* d_list1, hipStream_t st);
// the compaction route on its own, for the pairs whose state says mode 1
int dpl_octav_fallback_route(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                             const float* const* d_seg_ptrs, dpl_octav_state* d_states, int64_t n_pairs,
                             const dpl_span* d_pair_spans, const uint64_t* d_pair_base, const uint32_t* d_pair_order,
                             float* d_list0, float* d_list1, int dynamic_sym, int max_iters, hipStream_t st);
