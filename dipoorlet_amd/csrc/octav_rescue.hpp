// The RESCUE walk of the one-read OCTAV form: a pair whose exact-tail walk (octav_tail.hpp: walk_tail) was refused
// has left its exact bracket and suffix totals behind; k_octav_rescue_gather (octav_kernels.hip) re-reads that pair alone for the
// values of the bracket's bins, and walk_rescued / k_octav_walk_rescue here walk the reference's whole iterate sequence on them,
// every iterate verified.  What even that cannot finish restarts on the compaction route.
#pragma once
#include "common.hpp"
#include "octav_common.hpp"
#include "octav_wave.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kVec = 16;                                        // 16-byte vectors per thread the rescue walk keeps a list in
constexpr int kWalkOcc = 4;                                     // waves per SIMD k_octav_walk_rescue is bounded for

// The RESCUE walk of one pair (one workgroup; phase 2 of rounds 3 - 4's walk_pair, which also served the forms that round 5
// removed): a pair whose exact-tail walk was refused restarts from s_0 and walks the reference's WHOLE iterate sequence
// (forward_net.py:325-330) — totals of the bins above the iterate's bin from the suffix totals the first walk saved (exact
// integers), the values of the iterate's own bin from the list k_octav_rescue_gather collected (integer mantissa sums) —
// verifying that every iterate lands in a bin of the pair's bracket (rescue_bm).  An iterate outside it, or a list longer than
// the pair's region of the rescue list (it was cut), hands the pair to the compaction route.
template <int kVecT>
__device__ __forceinline__ void walk_rescued(
    const uint32_t pair, double* s_ge, uint32_t* n_ge, Shared& sh, dpl_octav_state* __restrict__ st,
    dpl_octav_state* __restrict__ ctl, const uint64_t* __restrict__ pair_base, int max_iters, int fail_every,
    const uint32_t* __restrict__ rescue_bm, const float* __restrict__ list_rescue, const unsigned long long* __restrict__ resc) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (kWave - 1);
    const int w = tid / kWave;
    dpl_octav_state* me = st + pair;
    if (me->mode != 3u || me->done) return;
    if (me->n_elems == 0ull) return;   // an empty pair: nothing was streamed
    const float* lp = list_rescue + pair_base[pair];
    f4 v[kVecT];
    // the list: ONE segment at the start of the pair's region; 1024 values per ROW (load_rows)
    {   // the suffix totals the first walk left for this pair (own bins per thread)
        constexpr int kPerT = kLogNB / kThreads;
        const int hi = kLogNB - 1 - (int)tid * kPerT;
        const double* rs = RescRow::s_ge(resc, pair);
        const uint32_t* rn = RescRow::n_ge(resc, pair);
#pragma unroll
        for (int qq = 0; qq < kPerT; ++qq) {
            n_ge[hi - qq] = rn[hi - qq];
            s_ge[hi - qq] = rs[hi - qq];
        }
    }
    if (tid < (uint32_t)kLogWords) sh.bm[tid] = rescue_bm[(uint64_t)pair * kLogWords + tid];   // the bins whose values were gathered
    if (tid == 0) {   // s_0 and the divisor are in the state since the first walk
        sh.s0 = me->s;
        sh.ud = me->unsigned_div;
        sh.n_elems = me->n_elems;
        sh.seg_len[0] = me->len[0];
        // (more gathered than the pair's region of the rescue list holds: the list is incomplete — the compaction route)
        sh.route = me->len[0] > (uint32_t)(pair_base[pair + 1] - pair_base[pair]) ? 1u : 2u;
    }
    __syncthreads();
    const uint32_t route = __builtin_amdgcn_readfirstlane(sh.route);
    uint32_t bad = route == 1u ? 1u : 0u;
    float s = sh.s0;
    uint32_t iters = 0u;
    if (route == 2u) {
        const float ud = sh.ud;
        const unsigned long long n_elems = sh.n_elems;
        const uint32_t L = __builtin_amdgcn_readfirstlane(sh.seg_len[0]);
        const uint32_t n_rows = (L + 1023u) >> 10;
        // the first kVec rows stay in registers for the whole walk; the rows beyond are streamed kOver at a time in every
        // iteration — requested before the resident rows are scanned, consumed after
        f4 ov[kOver];
        load_rows(v, lp, 0u, L);
        // every wave takes the step itself from the four partial sums (one barrier and two LDS round trips per iteration); the
        // gathered-bin bitmap sits in registers (lane l: word l)
        const uint32_t bm_reg = sh.bm[lane];
        auto marked = [&](int j) {
            return j > 0 && j < kLogNB - 1 && (((uint32_t)__builtin_amdgcn_readlane((int)bm_reg, j >> 5) >> (j & 31)) & 1u);
        };
        int jb = log_bin(s);
        bad = marked(jb) ? 0u : 1u;
        if (fail_every > 0 && pair % (uint32_t)fail_every == 0u) bad = 1u;   // test hook: the compaction route
        unsigned long long n_above = 0ull;
        double s_above = 0.0;
        auto enter = [&](int j) {   // exact totals of the bins above bin j
            n_above = (j + 1 < kLogNB) ? (unsigned long long)n_ge[j + 1] : 0ull;
            s_above = (j + 1 < kLogNB) ? s_ge[j + 1] : 0.0;
        };
        if (!bad) enter(jb);
        uint32_t par = 0u;   // alternating slots: a wave may write iteration k + 1's partials while another still reads k's
        uint32_t done = 0u;
        while (!done && !bad) {
            // values of bin jb above s: bit patterns in (bits(s), lower edge of bin jb + 1), i.e. d = u - bits(s) - 1 below
            // `span` (unsigned: anything at or below s wraps around).  Four VALU instructions per value — the count is a
            // population count of the compare mask on the scalar unit — and the mantissa sum follows from the sum of d.
            const uint32_t lo1 = __float_as_uint(s) + 1u;
            const uint32_t span = (((uint32_t)(jb + 1) + kLogKey0) << kLogShift) - lo1;
            uint32_t c = 0u;   // (wave-uniform)
            unsigned long long dsum = 0ull;
            uint32_t ds = 0u;   // per thread: at most 80 values below 2^17 between two wave sums
            auto in1 = [&](float f) {
                const uint32_t d = __float_as_uint(f) - lo1;
                const bool in = d < span;
                c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
                ds += in ? d : 0u;
            };
            if (n_rows > (uint32_t)kVecT) load_rows(ov, lp, (uint32_t)kVecT, L);
            {
                const uint32_t rows = min(n_rows, (uint32_t)kVecT);
#pragma unroll
                for (int u = 0; u < kVecT; ++u) {
                    if ((uint32_t)u < rows) {   // uniform
                        in1(v[u].x);
                        in1(v[u].y);
                        in1(v[u].z);
                        in1(v[u].w);
                    }
                }
                dsum += (unsigned long long)wave_sum_dpp(ds);   // < 64 * 80 * 2^17
                ds = 0u;
            }
            for (uint32_t r0 = (uint32_t)kVecT; r0 < n_rows; r0 += (uint32_t)kOver) {
#pragma unroll
                for (int u = 0; u < kOver; ++u) {   // (rows past the list's end were loaded as zeros)
                    in1(ov[u].x);
                    in1(ov[u].y);
                    in1(ov[u].z);
                    in1(ov[u].w);
                }
                if (r0 + (uint32_t)kOver < n_rows) load_rows(ov, lp, r0 + (uint32_t)kOver, L);
                dsum += (unsigned long long)wave_sum_dpp(ds);
                ds = 0u;
            }
            if (lane == 0) {
                sh.part_c[par][w] = c;
                sh.part_m[par][w] = dsum + (unsigned long long)c * (unsigned long long)(lo1 & 0x7FFFFFu);   // sum of explicit mantissas
            }
            __syncthreads();
            {
                unsigned long long tc = 0ull, tm = 0ull;
#pragma unroll
                for (int j = 0; j < kWaves; ++j) {
                    tc += sh.part_c[par][j];
                    tm += sh.part_m[par][j];
                }
                par ^= 1u;
                const unsigned long long tg = n_above + tc;
                const double ts = s_above + (double)(tm + (tc << 23)) * log_bin_scale(jb);
                const OctavStep qs = octav_step(ts, tg, n_elems - tg, ud, s, iters, max_iters);
                s = qs.s;
                iters = qs.iters;
                done = qs.done;
                if (!done) {
                    const int jn = log_bin(s);
                    if (!marked(jn)) {
                        bad = 1u;   // a bin that was not gathered (or out of the binned window): the compaction route takes over
                    } else if (jn != jb) {
                        jb = jn;
                        enter(jb);
                    }
                }
            }
        }
    }
    if (tid == 0) {
        if (bad) {
            // s_0 is still in me->s; of the restart state this form has written done and len[0] (the gather's cursor)
            DPL_OCTAV_RESTART_COMPACTION(*me, ctl, kDirtyDone | kDirtyList0);
        } else {
            me->s = s;
            me->iters = iters;
            me->done = 1u;
            me->mode = 2u;
        }
    }
}

// The rescue walk: a small persistent grid over the list of rescued pairs — usually empty, and a launch that has nothing to do
// should not have thousands of workgroups to schedule between those of the next batch's streaming kernel.
__global__ __launch_bounds__(kThreads, kWalkOcc) void k_octav_walk_rescue(
    dpl_octav_state* __restrict__ st, dpl_octav_state* __restrict__ ctl, const uint64_t* __restrict__ pair_base, int max_iters,
    int fail_every, const uint32_t* __restrict__ rescue_bm, const uint32_t* __restrict__ missed,
    const float* __restrict__ list_rescue, const unsigned long long* __restrict__ resc) {
    __shared__ double s_ge[kLogNB];
    __shared__ uint32_t n_ge[kLogNB];
    __shared__ Shared sh;
    const uint32_t n_missed = ctl->len[0];
    for (uint32_t e = blockIdx.x; e < n_missed; e += gridDim.x) {
        walk_rescued<kVec>(missed[3 * e], s_ge, n_ge, sh, st, ctl, pair_base, max_iters, fail_every, rescue_bm, list_rescue, resc);
        __syncthreads();
    }
}

}  // namespace
