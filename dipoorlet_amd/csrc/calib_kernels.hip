// MI355X (gfx950 / CDNA4) activation-calibration kernels + C ABI (include/dipoorlet_hip.h).
//
// Everything here but the entropy search (K4b: fp64 arithmetic on an LDS-resident row) is an HBM-bound streaming
// reduction / scatter-add: no MFMA.  Design rules
// (guides: cdna_hip_programming.md G2/G11/G12/G13, MI355X_MICROARCH.md §LDS/§HBM):
//   * 16 B per lane coalesced loads (global_load_dwordx4), several independent loads in flight,
//     one workgroup per work item (a contiguous chunk of ONE tensor), >> 256 workgroups per launch;
//   * wave64 reductions with DPP/ds_bpermute shuffles, then a tiny LDS combine per workgroup;
//   * histograms privatised in LDS (ds_add_u32), exact zeros counted in registers (ReLU outputs are
//     ~50 % zeros and would otherwise serialise on one LDS address), one flush per workgroup;
//   * order-encoded integer atomics for fp32 min/max, so accumulators persist across launches.
// The tables these kernels index with (work items, block shares) are built on the host by host_plan.hpp.
#include "common.hpp"

// Bit-exact numpy parity needs every fp32 operation rounded on its own: HIP's default
// -ffp-contract=fast would fuse i*step + first into one FMA (__fmul_rn/__fadd_rn are plain * and +
// in this toolchain).  Also passed as a flag by csrc/build.py.
#pragma clang fp contract(off)

namespace {

// ================================================================ K1: running min / max
struct MinMaxOp {
    float mn, mx;
    uint32_t nan;
    __device__ __forceinline__ void operator()(float x) {
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
        nan |= (x != x);
    }
};

// Workgroup reduction of the lanes' MinMaxOp and the three atomics into the slot's accumulators (s_mn / s_mx / s_nan: one word per wave).
__device__ __forceinline__ void minmax_commit(const MinMaxOp& op, uint32_t slot, float* s_mn, float* s_mx, uint32_t* s_nan,
                                              uint32_t* __restrict__ min_enc, uint32_t* __restrict__ max_enc,
                                              uint32_t* __restrict__ nan_flag) {
    float mn = wave_min(op.mn), mx = wave_max(op.mx);
    uint32_t nn = __any(op.nan) ? 1u : 0u;
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_mn[w] = mn;
        s_mx[w] = mx;
        s_nan[w] = nn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < kBlock / kWave; ++j) {
            mn = fminf(mn, s_mn[j]);
            mx = fmaxf(mx, s_mx[j]);
            nn |= s_nan[j];
        }
        if (mn <= mx) {  // false only when the chunk held nothing but NaN
            atomicMin(min_enc + slot, enc_f32(mn));
            atomicMax(max_enc + slot, enc_f32(mx));
        }
        if (nn) atomicOr(nan_flag + slot, 1u);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_minmax(const dpl_work_item* __restrict__ items,
                                                    const uint32_t* __restrict__ bb,
                                                    const float* const* __restrict__ segs,
                                                    uint32_t* __restrict__ min_enc, uint32_t* __restrict__ max_enc,
                                                    uint32_t* __restrict__ nan_flag) {
    __shared__ float s_mn[kBlock / kWave], s_mx[kBlock / kWave];
    __shared__ uint32_t s_nan[kBlock / kWave];
    uint32_t k0, k1;
    block_items(bb, k0, k1);
    for (uint32_t k = k0; k < k1; ++k) {
        const dpl_work_item it = items[k];
        MinMaxOp op{INFINITY, -INFINITY, 0u};
        stream_span(segs[it.seg] + it.offset, it.count, op);
        minmax_commit(op, it.slot, s_mn, s_mx, s_nan, min_enc, max_enc, nan_flag);
    }
}

__global__ void k_minmax_init(uint32_t* mn, uint32_t* mx, uint32_t* nan, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        mn[i] = 0xFFFFFFFFu;
        mx[i] = 0u;
        nan[i] = 0u;
    }
}

// The fp32 range of a slot's accumulators: NaN for both when the slot saw a NaN or no data (shared by k_minmax_finalize and the
// range pass's snapshot, k_hist_snapshot: one piece of device code, so the two cannot disagree in a bit).
__device__ __forceinline__ void minmax_decode(uint32_t mn, uint32_t mx, uint32_t nan, float& omn, float& omx) {
    const bool bad = nan != 0u || mn == 0xFFFFFFFFu;
    omn = bad ? NAN : dec_f32(mn);
    omx = bad ? NAN : dec_f32(mx);
}

__global__ void k_minmax_finalize(const uint32_t* mn, const uint32_t* mx, const uint32_t* nan, int64_t n,
                                  float* omn, float* omx) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) minmax_decode(mn[i], mx[i], nan[i], omn[i], omx[i]);
}

__global__ void k_minmax_encode(const float* mn, const float* mx, int64_t n, uint32_t* emn, uint32_t* emx,
                                uint32_t* nan) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const bool bad = (mn[i] != mn[i]) || (mx[i] != mx[i]);
        emn[i] = bad ? 0xFFFFFFFFu : enc_f32(mn[i]);
        emx[i] = bad ? 0u : enc_f32(mx[i]);
        nan[i] = bad ? 1u : 0u;
    }
}

// ================================================================ K2: |x| histogram, numpy-exact
// numpy's uniform-bin fast path lands every kept value a in the unique bin i with
// edge[i] <= a < edge[i+1] (last bin closed), edge[i] = fl32(fl32(i*step) + first): an index
// estimate followed by one decrement test and one increment test against those edges.  Any estimate
// within +-1 of the true bin gives the same answer, so the estimate here is a multiply by the
// reciprocal (error << 1 bin) unless the range is so small that the reciprocal is not finite.
__device__ __forceinline__ float hist_edge(int i, float step, float first) {
    return __fadd_rn(__fmul_rn((float)i, step), first);  // no FMA contraction: numpy rounds twice
}

// Two bin paths:
//   kFast  (first == 0, reciprocal finite — every non-degenerate range): `inv` carries a +1e-6 relative
//          bias (k_hist_prepare), which dominates the ~3e-7 of accumulated fp32 rounding in the estimate
//          and in the edges, so floor(a*inv) is the true bin or the one above it, never below: ONE
//          decrement test against edge(i) = fl32(i*step) settles it (the bias is < 0.02 bin at 16384 bins).
//   exact  (degenerate (-0.5, 0.5) range of an all-zero tensor, or a range so small that the reciprocal
//          overflows): numpy's own sequence — correctly rounded divide, decrement test, increment test.
// (Measured alternatives that lost and were removed: unconditional ds_add into per-lane dummy slots +2 %;
// ablations: no flush -2.5 %, no LDS atomics -3 % — the kernel is within 5 % of the plain streaming read.)
template <bool kFast>
struct HistOp {
    uint32_t* lds;
    float first, last, step, inv, denom;
    int last_bin;  // bins - 1
    float fbins;
    uint32_t nonzero;  // count of a != 0 (NaN included); exact zeros = elements - nonzero
    __device__ __forceinline__ void operator()(float x) {
        const float a = fabsf(x);
        const bool nz = (a != 0.0f);
        nonzero += nz;
        if (kFast) {
            // (11 vector instructions per element where the form below takes 13 — what matters once the chip runs warm and
            // the shader clock comes down: DESIGN 3e.  No clamp: a <= last gives a * inv <= bins * (1 + 1e-6) + rounding, the
            // estimate is at most `bins`, and counter `bins` — a == last where bins * step rounds to last or below — is folded
            // into the closed last bin at the flush; the byte address in one shift-add.)
            if (nz && (a <= last)) {
                const int i = (int)__fmul_rn(a, inv);      // (v_cvt_i32_f32 maps NaN to 0: dropped by the test above)
                const uint32_t dec = (a < __fmul_rn((float)i, step)) ? 0xFFFFFFFCu : 0u;
                atomicAdd(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds) + (((uint32_t)i << 2) + dec)), 1u);
            }
            return;
        }
        int i;
        if (kFast) {
            i = (int)__fmul_rn(a, inv);  // v_cvt_i32_f32 saturates and maps NaN to 0
            i = i > last_bin ? last_bin : i;
            i -= (a < __fmul_rn((float)i, step)) ? 1 : 0;
        } else {
            i = (int)__fmul_rn(__fdiv_rn(__fsub_rn(a, first), denom), fbins);
            i = i > last_bin ? last_bin : i;
            i = i < 0 ? 0 : i;
            i -= (a < hist_edge(i, step, first)) ? 1 : 0;
            i += (i != last_bin && a >= hist_edge(i + 1, step, first)) ? 1 : 0;
        }
        // exact zeros are counted in a register and added to their bin once per wave (ReLU outputs are ~50 %
        // zeros: they would serialise on one LDS address); out-of-range values and NaN (a <= last false) drop;
        // a >= first always holds since first <= 0 <= a.
        if (nz && (a <= last)) atomicAdd(lds + i, 1u);  // ds_add_u32 (no return)
    }
};

template <bool kFast>
__device__ __forceinline__ void hist_op_init(HistOp<kFast>& op, const dpl_hist_range& r, int bins, uint32_t* lds) {
    op.lds = lds;
    op.first = r.first;
    op.last = r.last;
    op.step = r.step;
    op.inv = r.inv;
    op.denom = __fsub_rn(r.last, r.first);
    op.last_bin = bins - 1;
    op.fbins = (float)bins;
    op.nonzero = 0u;
}

// The workgroup's LDS counters of one item -> the slot's row of `out` (uint64: the accumulated histogram; uint32: a batch's own
// counts in the range pass, where a tensor of fewer than 2^32 elements cannot overflow a counter).
template <class Count>
__device__ __forceinline__ void hist_flush(uint32_t nonzero, const dpl_work_item& it, const dpl_hist_range& r, int bins,
                                           Count* __restrict__ hist, uint32_t* lds, uint32_t* s_nz) {
    const uint32_t nzw = wave_sum(nonzero);
    if ((threadIdx.x & (kWave - 1)) == 0) s_nz[threadIdx.x / kWave] = nzw;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t nzb = 0;
        for (int k = 0; k < kBlock / kWave; ++k) nzb += s_nz[k];
        // |0| is kept iff first <= 0 <= last, which always holds for a finite range
        const uint32_t z = it.count - nzb;
        if (z) atomicAdd(lds + r.zero_bin, z);
        const uint32_t top = lds[bins];        // (estimates of `bins`: values equal to `last`)
        if (top) atomicAdd(lds + bins - 1, top);
    }
    __syncthreads();
    Count* __restrict__ out = hist + (uint64_t)it.slot * (uint64_t)bins;
    for (int b = threadIdx.x; b < bins; b += kBlock) {
        const uint32_t c = lds[b];
        if (c) {
            if constexpr (sizeof(Count) == 8)
                atomicAdd(reinterpret_cast<unsigned long long*>(out + b), (unsigned long long)c);
            else
                atomicAdd(out + b, c);
        }
    }
}

template <bool kFast>
__device__ __forceinline__ void hist_body(const dpl_work_item& it, const float* const* __restrict__ segs,
                                          const dpl_hist_range& r, int bins, uint64_t* __restrict__ hist,
                                          uint32_t* lds, uint32_t* s_nz) {
    HistOp<kFast> op;
    hist_op_init(op, r, bins, lds);
    stream_span(segs[it.seg] + it.offset, it.count, op);
    hist_flush(op.nonzero, it, r, bins, hist, lds, s_nz);
}

__global__ __launch_bounds__(kBlock) void k_abs_hist(const dpl_work_item* __restrict__ items,
                                                      const uint32_t* __restrict__ bb,
                                                      const float* const* __restrict__ segs,
                                                      const dpl_hist_range* __restrict__ ranges, int bins,
                                                      uint64_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // bins + 1 counters + one word per wave
    uint32_t* s_nz = lds + bins + 1;
    uint32_t k0, k1;
    block_items(bb, k0, k1);
    for (uint32_t k = k0; k < k1; ++k) {
        const dpl_work_item it = items[k];
        const dpl_hist_range r = ranges[it.slot];
        if (r.status != 0u) continue;  // reference raises for this tensor; host reports it (uniform branch)
        for (int b = threadIdx.x; b <= bins; b += kBlock) lds[b] = 0u;
        __syncthreads();
        if (r.exact_div)
            hist_body<false>(it, segs, r, bins, hist, lds, s_nz);
        else
            hist_body<true>(it, segs, r, bins, hist, lds, s_nz);
        __syncthreads();
    }
}

__device__ __forceinline__ float py_max(float a, float b) { return (b > a) ? b : a; }  // python max(a, b)
__device__ __forceinline__ float py_min(float a, float b) { return (b < a) ? b : a; }  // python min(a, b)

// The histogram range of a slot from its fp32 min / max.  A histogram depends on the range through this struct alone, so two
// ranges that agree byte for byte bin every value alike: what the range pass's speculation rests on (k_hist_snapshot,
// k_hist_resolve).
__device__ __forceinline__ dpl_hist_range hist_range_of(float gmin, float gmax, int bins) {
    dpl_hist_range r;
    // forward_net.py:266 — data_max = max(np.max(maxlist), -np.min(minlist))
    const float dmax = py_max(gmax, -gmin);
    float first = 0.0f, last = dmax;
    r.dmax = dmax;
    r.status = 0u;
    if (!(fabsf(last) <= 3.402823466e+38f) || last < first) r.status = 1u;  // NaN, inf (or negative) range
    if (first == last) {  // numpy _get_outer_edges: expand an empty range
        first = -0.5f;
        last = 0.5f;
    }
    const float delta = __fsub_rn(last, first);
    const float fb = (float)bins;
    r.first = first;
    r.last = last;
    r.step = __fdiv_rn(delta, fb);
    // +1e-6 relative bias: see HistOp (kFast).  1.000001f = 1 + 8*2^-23 exactly representable enough:
    // the product is rounded once more, still >= (1 + 9e-7) * bins/delta.
    r.inv = __fmul_rn(__fdiv_rn(fb, delta), 1.000001f);
    // linspace must give strictly increasing fp32 edges, else numpy raises "Too many bins"
    if (r.status == 0u) {
        const float e1 = hist_edge(1, r.step, first);
        const float el = hist_edge(bins - 1, r.step, first);
        const float el2 = hist_edge(bins - 2 > 0 ? bins - 2 : 0, r.step, first);
        if (!(r.step > 0.0f) || !(e1 > first) || !(last > el) || (bins > 2 && !(el > el2))) r.status = 2u;
    }
    r.exact_div = (first != 0.0f || !(fabsf(r.inv) <= 3.402823466e+38f) || r.step < 1.0e-30f) ? 1u : 0u;
    // bin of |x| == 0
    {
        const float a = 0.0f;
        float t = __fmul_rn(__fdiv_rn(__fsub_rn(a, first), delta), fb);
        int b = (int)t;
        b = b > bins - 1 ? bins - 1 : b;
        b = b < 0 ? 0 : b;
        if (a < hist_edge(b, r.step, first)) --b;
        if (b != bins - 1 && a >= hist_edge(b + 1, r.step, first)) ++b;
        r.zero_bin = (uint32_t)(b < 0 ? 0 : b);
    }
    return r;
}

__global__ void k_hist_prepare(const float* __restrict__ gmin, const float* __restrict__ gmax, int64_t n, int bins,
                               dpl_hist_range* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = hist_range_of(gmin[i], gmax[i], bins);
}

// ================================================================ K2s: a batch's histogram taken in the RANGE pass
// numpy's bins depend on dmax over the whole shard, known only after the last batch — but on nothing else, and the running
// dmax of a tensor stops moving once the batch that holds its extreme has passed.  The range pass therefore histograms every
// batch against the range its running min / max give (a SNAPSHOT taken before the launch: other workgroups move the live
// accumulators during it) into a per-batch ledger entry; the histogram pass compares the snapshot with the final range byte for
// byte (k_hist_resolve), adds the rows that match and reads only the tensors whose guess was wrong (k_abs_hist_rest).  A wrong
// guess costs what it always cost, so no count can change.  Ledger entry (dpl_hist_spec_entry_bytes):
//   dpl_hist_range snap[n_slots] | uint32 flags[n_slots] | (16-byte aligned) uint32 counts[n_slots, bins]
__host__ __device__ inline uint64_t spec_counts_offset(int64_t n_slots) {
    return (((uint64_t)n_slots * (sizeof(dpl_hist_range) + sizeof(uint32_t))) + 15ull) & ~15ull;
}

// Snapshot of the provisional ranges + the entry's counts zeroed.  A slot with no data yet, a NaN flag or a range numpy would
// refuse comes out with status != 0 ("no guess": the fused kernel takes its min / max only and k_hist_resolve never accepts it).
__global__ __launch_bounds__(kBlock) void k_hist_snapshot(const uint32_t* __restrict__ mn, const uint32_t* __restrict__ mx,
                                                           const uint32_t* __restrict__ nan, int64_t n, int bins,
                                                           dpl_hist_range* __restrict__ snap, uint32_t* __restrict__ flags,
                                                           uint32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (i < n) {
        float gmin, gmax;
        minmax_decode(mn[i], mx[i], nan[i], gmin, gmax);
        snap[i] = hist_range_of(gmin, gmax, bins);
        flags[i] = 0u;
    }
    const int64_t total = n * (int64_t)bins;
    for (int64_t j = i; j < total; j += stride) counts[j] = 0u;
}

template <bool kFast>
struct MinMaxHistOp {
    MinMaxOp m;
    HistOp<kFast> h;
    __device__ __forceinline__ void operator()(float x) {
        m(x);
        h(x);
    }
};

template <bool kFast>
__device__ __forceinline__ void minmax_hist_body(const dpl_work_item& it, const float* const* __restrict__ segs,
                                                 const dpl_hist_range& r, int bins, uint32_t* __restrict__ counts,
                                                 uint32_t* lds, uint32_t* s_nz, MinMaxOp& m) {
    MinMaxHistOp<kFast> op;
    op.m = m;
    hist_op_init(op.h, r, bins, lds);
    stream_span(segs[it.seg] + it.offset, it.count, op);
    m = op.m;
    hist_flush(op.h.nonzero, it, r, bins, counts, lds, s_nz);
}

// k_minmax and k_abs_hist in one read: min / max / NaN into the accumulators as k_minmax does, counts against snap[slot] into the
// ledger entry as k_abs_hist does (same HistOp, same flush).
__global__ __launch_bounds__(kBlock) void k_minmax_hist(const dpl_work_item* __restrict__ items,
                                                         const uint32_t* __restrict__ bb,
                                                         const float* const* __restrict__ segs,
                                                         uint32_t* __restrict__ min_enc, uint32_t* __restrict__ max_enc,
                                                         uint32_t* __restrict__ nan_flag,
                                                         const dpl_hist_range* __restrict__ snap, int bins,
                                                         uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_mh[];  // bins + 1 counters, one word per wave, 3 words per wave
    uint32_t* s_nz = lds_mh + bins + 1;
    float* s_mn = reinterpret_cast<float*>(s_nz + kBlock / kWave);
    float* s_mx = s_mn + kBlock / kWave;
    uint32_t* s_nan = reinterpret_cast<uint32_t*>(s_mx + kBlock / kWave);
    uint32_t k0, k1;
    block_items(bb, k0, k1);
    for (uint32_t k = k0; k < k1; ++k) {
        const dpl_work_item it = items[k];
        const dpl_hist_range r = snap[it.slot];
        MinMaxOp m{INFINITY, -INFINITY, 0u};
        if (r.status != 0u) {  // no guess for this slot (uniform branch)
            stream_span(segs[it.seg] + it.offset, it.count, m);
        } else {
            for (int b = threadIdx.x; b <= bins; b += kBlock) lds_mh[b] = 0u;
            __syncthreads();
            if (r.exact_div)
                minmax_hist_body<false>(it, segs, r, bins, counts, lds_mh, s_nz, m);
            else
                minmax_hist_body<true>(it, segs, r, bins, counts, lds_mh, s_nz, m);
        }
        minmax_commit(m, it.slot, s_mn, s_mx, s_nan, min_enc, max_enc, nan_flag);
    }
}

// One workgroup per slot: the guess was right iff the snapshot equals the final range in all 32 bytes (a sign-of-zero or NaN
// difference falls to the safe side) and numpy accepts the range.  flags[t]: 1 = the entry's row is this batch's histogram and
// has been added; 2 = nothing to count (status != 0: k_abs_hist skips such a tensor too); 0 = to be read.
// stats (may be null) += {pairs, pairs added, elements, elements added}.
__global__ __launch_bounds__(kBlock) void k_hist_resolve(const dpl_hist_range* __restrict__ snap,
                                                          const dpl_hist_range* __restrict__ fin,
                                                          const uint32_t* __restrict__ counts, const uint64_t* __restrict__ elems,
                                                          int bins, uint64_t* __restrict__ hist, uint32_t* __restrict__ flags,
                                                          unsigned long long* __restrict__ stats) {
    const uint32_t t = blockIdx.x;
    const uint32_t* a = reinterpret_cast<const uint32_t*>(snap + t);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(fin + t);
    bool same = true;
#pragma unroll
    for (int w = 0; w < (int)(sizeof(dpl_hist_range) / 4); ++w) same = same && (a[w] == b[w]);
    const uint32_t status = fin[t].status;
    const bool valid = same && status == 0u;
    if (threadIdx.x == 0) {
        flags[t] = valid ? 1u : (status != 0u ? 2u : 0u);
        if (stats) {
            const unsigned long long e = elems[t];
            atomicAdd(stats + 0, 1ull);
            atomicAdd(stats + 2, e);
            if (valid) {
                atomicAdd(stats + 1, 1ull);
                atomicAdd(stats + 3, e);
            }
        }
    }
    if (!valid) return;
    const uint32_t* __restrict__ row = counts + (uint64_t)t * (uint64_t)bins;
    uint64_t* __restrict__ out = hist + (uint64_t)t * (uint64_t)bins;
    for (int j = threadIdx.x; j < bins; j += kBlock) {
        const uint32_t c = row[j];
        if (c) out[j] += (uint64_t)c;  // (this workgroup alone touches row t during the launch)
    }
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, kWave), hi = __shfl_up((uint32_t)(v >> 32), d, kWave);
    return ((uint64_t)hi << 32) | lo;
}

// k_abs_hist over the tensors k_hist_resolve left (flags[t] == 0), BALANCED: the remaining tensors' elements form one stream,
// workgroup b of G owns [cut(b), cut(b + 1)) of it, cut(b) = floor(total * b / G) rounded down to a multiple of 1024 elements
// from the start of the tensor it falls in — the cuts dpl_build_balanced_items makes, in closed form, so every workgroup derives
// its own share from the prefix sums (taken by each workgroup into LDS: T additions) with no list built and no host in between.
// Tensor t is segment t, slot t, offset 0 (the per-tensor spans of a TensorSetPlan); elems[t] < 2^32.
// (k_abs_hist_rest below; rest_prefix and rest_cut are its two steps, shared with the test hook k_hist_spec_cuts.)
//
// Exclusive prefix sums of the remaining tensors' element counts into P[0 .. n_tensors] (LDS), by the whole workgroup.
__device__ __forceinline__ void rest_prefix(const uint64_t* __restrict__ elems, const uint32_t* __restrict__ flags, int n_tensors,
                                            uint64_t* P, uint64_t* s_tot) {
    const int per = (n_tensors + kBlock - 1) / kBlock;  // consecutive tensors per thread
    const int t0 = (int)threadIdx.x * per;
    uint64_t mine = 0;
    for (int j = 0; j < per; ++j) {
        const int t = t0 + j;
        if (t < n_tensors && flags[t] == 0u) mine += elems[t];
    }
    uint64_t incl = mine;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint64_t up = shfl_up_u64(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == kWave - 1) s_tot[wv] = incl;
    __syncthreads();
    uint64_t run = incl - mine;
    for (int w = 0; w < wv; ++w) run += s_tot[w];
    for (int j = 0; j < per; ++j) {
        const int t = t0 + j;
        if (t < n_tensors) {
            P[t] = run;
            if (flags[t] == 0u) run += elems[t];
        }
    }
    if (threadIdx.x == kBlock - 1) P[n_tensors] = run;
    __syncthreads();
}

// Cut b of G (0 <= b <= G) of a stream of P[n_tensors] > 0 elements, and the tensor it falls in (n_tensors for the end).
__device__ __forceinline__ void rest_cut(const uint64_t* P, int n_tensors, uint64_t G, uint64_t b, uint64_t& cut, int& at) {
    const uint64_t total = P[n_tensors], q = total / G, rem = total % G;
    const uint64_t target = (b >= G) ? total : q * b + (rem * b) / G;  // floor(total * b / G) without a 128-bit product
    if (target >= total) {
        cut = total;
        at = n_tensors;
        return;
    }
    int lo = 1, hi = n_tensors;  // first index in [1, T] with P[index] > target (exists: P[T] = total > target)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (P[mid] > target) hi = mid; else lo = mid + 1;
    }
    at = lo - 1;
    cut = P[lo - 1] + ((target - P[lo - 1]) & ~1023ull);
}

__global__ __launch_bounds__(kBlock) void k_abs_hist_rest(const uint64_t* __restrict__ elems, const uint32_t* __restrict__ flags,
                                                           int n_tensors, const float* const* __restrict__ segs,
                                                           const dpl_hist_range* __restrict__ ranges, int bins,
                                                           uint64_t* __restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rest[];
    // layout: uint64 P[n_tensors + 1] | uint64 wave totals [4] | counters [bins + 1] | s_nz [4]
    uint64_t* P = reinterpret_cast<uint64_t*>(lds_rest);
    uint64_t* s_tot = P + n_tensors + 1;
    uint32_t* lds = reinterpret_cast<uint32_t*>(s_tot + kBlock / kWave);
    uint32_t* s_nz = lds + bins + 1;
    rest_prefix(elems, flags, n_tensors, P, s_tot);
    if (P[n_tensors] == 0) return;
    uint64_t cut[2];
    int at[2];
    rest_cut(P, n_tensors, gridDim.x, blockIdx.x, cut[0], at[0]);
    rest_cut(P, n_tensors, gridDim.x, (uint64_t)blockIdx.x + 1, cut[1], at[1]);
    uint64_t pos = cut[0];
    const uint64_t end = cut[1];
    int t = at[0];
    while (pos < end) {  // (pos < end <= P[T], so t + 1 <= T below)
        while (P[t + 1] <= pos) ++t;
        const uint64_t stop = P[t + 1] < end ? P[t + 1] : end;
        dpl_work_item it;
        it.offset = pos - P[t];
        it.count = (uint32_t)(stop - pos);
        it.seg = (uint32_t)t;
        it.slot = (uint32_t)t;
        it.reserved = 0u;
        const dpl_hist_range r = ranges[t];  // (status == 0: k_hist_resolve flagged every other tensor)
        for (int b = threadIdx.x; b <= bins; b += kBlock) lds[b] = 0u;
        __syncthreads();
        if (r.exact_div)
            hist_body<false>(it, segs, r, bins, hist, lds, s_nz);
        else
            hist_body<true>(it, segs, r, bins, hist, lds, s_nz);
        __syncthreads();
        pos = stop;
    }
}

// The cuts k_abs_hist_rest works to, written out (dpl_hist_spec_cuts: what tests hold against tests/hist_spec_model.py).
__global__ __launch_bounds__(kBlock) void k_hist_spec_cuts(const uint64_t* __restrict__ elems, const uint32_t* __restrict__ flags,
                                                            int n_tensors, uint64_t* __restrict__ cuts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cuts[];
    uint64_t* P = reinterpret_cast<uint64_t*>(lds_cuts);
    uint64_t* s_tot = P + n_tensors + 1;
    rest_prefix(elems, flags, n_tensors, P, s_tot);
    if (threadIdx.x != 0) return;
    uint64_t cut = 0;
    int at = 0;
    if (P[n_tensors] != 0) rest_cut(P, n_tensors, gridDim.x, blockIdx.x, cut, at);
    cuts[blockIdx.x] = cut;
    if (blockIdx.x + 1 == gridDim.x) cuts[gridDim.x] = P[n_tensors];
}

// The fp32 clip range of a histogram search that ends on bin `found` (-1: none, the range itself): the centre of that bin,
// basic_algorithm.py:42-53.  Shared by the percentile and the entropy search.
__device__ __forceinline__ void store_bin_clip(int found, float gmin, float gmax, int bins, float* __restrict__ clip) {
    float lo = gmin, hi = gmax;
    if (found >= 0) {
        const float dmax = py_max(-gmin, gmax);  // basic_algorithm.py:42
        const float cv = __fmul_rn((float)found + 0.5f, __fdiv_rn(dmax, (float)bins));
        lo = py_max(-cv, gmin);
        hi = py_min(cv, gmax);
    }
    clip[0] = lo;
    clip[1] = hi;
}

// ================================================================ K4: percentile clip (basic_algorithm.py:40-53)
// One wave per slot.  The cumulative sum is a SEQUENTIAL fp64 accumulation in bin order (the >=
// threshold test is order sensitive), so lanes load 64 bins at a time and the wave walks them in order
// (2048 dependent fp64 additions: ~10 us per launch; through ds_bpermute shuffles and a branch per bin it was 190 us).
__global__ __launch_bounds__(kWave) void k_hist_percentile(const uint64_t* __restrict__ hist,
                                                            const float* __restrict__ gmin_a,
                                                            const float* __restrict__ gmax_a, int bins,
                                                            double threshold, float* __restrict__ clip) {
    const int slot = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t* h = hist + (uint64_t)slot * bins;
    unsigned long long tot = 0;
    for (int b = lane; b < bins; b += kWave) tot += h[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, kWave);
    const double total = (double)(long long)tot;  // int64 -> float64
    const float gmin = gmin_a[slot], gmax = gmax_a[slot];
    double accum = 0.0;
    int found = -1;
    // One chunk of 64 bins per round.  The next chunk's counts are requested BEFORE this chunk is walked (the load's latency
    // sits beside the 64 additions); the lane index of the walk is wave-uniform (v_readlane, not a shuffle through LDS) and the
    // chain of additions carries no branch: the bins that reach the threshold are collected in a mask, its lowest bit is the answer.
    uint64_t raw_next = lane < bins ? h[lane] : 0ull;
    for (int base = 0; base < bins && found < 0; base += kWave) {
        const int b = base + lane;
        // hist.astype(float32) / hist.sum()  -> float64(float32(count)) / float64(total)
        const double hv = (b < bins) ? (double)(float)(long long)raw_next / total : 0.0;
        raw_next = (b + kWave < bins) ? h[b + kWave] : 0ull;
        const int lim = (bins - base) < kWave ? (bins - base) : kWave;
        const int h_lo = __double2loint(hv), h_hi = __double2hiint(hv);
        uint64_t reached = 0;
        if (lim == kWave) {
#pragma unroll
            for (int j = 0; j < kWave; ++j) {
                accum += __hiloint2double(__builtin_amdgcn_readlane(h_hi, j), __builtin_amdgcn_readlane(h_lo, j));
                reached |= (accum >= threshold) ? (1ull << j) : 0ull;
            }
        } else {
            for (int j = 0; j < lim; ++j) {
                accum += __hiloint2double(__builtin_amdgcn_readlane(h_hi, j), __builtin_amdgcn_readlane(h_lo, j));
                reached |= (accum >= threshold) ? (1ull << j) : 0ull;
            }
        }
        if (reached) found = base + __builtin_ctzll(reached);
    }
    if (lane == 0) store_bin_clip(found, gmin, gmax, bins, clip + 2 * slot);
}

// ================================================================ K4b: entropy (KL-divergence) clip — beyond the reference
// The definition is this project's own (tests/kl_model.py): for every candidate i in [levels, bins] — keep bins
// [0, i), outliers folded into bin i - 1 — the divergence between the kept histogram p and its image q on `levels` groups
// (group j = bins [j i / L, (j + 1) i / L), a group's mass WITHOUT the outliers spread over its bins where p != 0), both
// smoothed (zeros -> eps, taken evenly from the non-zeros) and normalised.
//
// grid = (candidate chunk, tensor).  A workgroup holds its tensor's row in LDS as an exclusive prefix sum of the counts (u64;
// a count is the difference of two neighbours) and the non-zero flags as one 64-bit mask and one running count per 64 bins, so
// a group's mass is two LDS reads and its live-bin count two reads and two popcounts, whatever the group's length: 8 B per bin,
// 133 KB with the masks at 16384 bins (one workgroup per CU there; 2048 bins: 19 KB).  One wave per candidate at a time, lanes own bins; the
// group of a bin is ((b + 1) L - 1) / i (the divisors are wave-uniform: their reciprocals leave the loop).  Everything that
// does not depend on the bin is formed analytically per candidate: the number of non-zero bins of p and of q (q has one fewer
// exactly when the last group holds nothing but outliers), the two smoothing amounts, the two sums (sum p' = N - n1 e1 + z eps),
// and the z bins where p is zero, which all contribute the same term.  Counts convert to fp64 exactly (a calibration set stays
// far below 2^53 elements).  A lane adds its bins in order, the 64 partial sums meet in a fixed shuffle tree, one lane stores:
// no floating-point atomics, two calls give the same bits, and a candidate's value does not depend on the launch's geometry.
// Candidates cost in proportion to i: they are dealt round-robin to the chunks and, inside a chunk, to the four waves.
constexpr double kKlEps = 1e-4;

__device__ __forceinline__ uint32_t kl_live_below(const uint64_t* __restrict__ mask, const uint32_t* __restrict__ bcnt, uint32_t x) {
    const uint32_t k = x >> 6;   // bins [0, x) with a non-zero count
    return bcnt[k] + (uint32_t)__popcll(mask[k] & ((1ull << (x & 63u)) - 1ull));
}

__global__ __launch_bounds__(kBlock) void k_hist_kl(const uint64_t* __restrict__ hist, int bins, int levels, int n_chunks,
                                                     double* __restrict__ div) {
    extern __shared__ __attribute__((aligned(16))) uint64_t kl_lds[];
    const uint32_t nblk = ((uint32_t)bins + 63u) >> 6;
    uint64_t* cs = kl_lds;                     // [bins + 1] exclusive prefix sum of the counts
    uint64_t* mask = cs + bins + 1;            // [nblk + 1] bit b & 63 of mask[b >> 6]: count of bin b != 0 (the last entry is 0)
    uint64_t* part = mask + nblk + 1;          // [kBlock] the scan's per-thread sums
    uint32_t* bcnt = reinterpret_cast<uint32_t*>(part + kBlock);   // [nblk + 1] non-zero bins below bin 64 k
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t slot = blockIdx.x / (uint32_t)n_chunks, chunk = blockIdx.x % (uint32_t)n_chunks;
    const uint64_t* __restrict__ h = hist + (uint64_t)slot * (uint64_t)bins;
    double* __restrict__ out = div + (uint64_t)slot * ((uint64_t)bins + 1u);
    const uint32_t L = (uint32_t)levels, C = (uint32_t)n_chunks, nb = (uint32_t)bins;

    // ---- the row: prefix sums (a contiguous run of bins per thread, then the threads' sums) and the non-zero masks
    {
        const uint32_t per = (nb + kBlock - 1) / kBlock;
        const uint32_t b0 = tid * per < nb ? tid * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
        uint64_t s = 0;
        for (uint32_t b = b0; b < b1; ++b) s += h[b];
        part[tid] = s;
        for (uint32_t k = wave; k < nblk; k += kBlock / kWave) {
            const uint32_t b = k * kWave + lane;
            const uint64_t m = __ballot(b < nb && h[b] != 0ull);
            if (lane == 0) mask[k] = m;
        }
        if (tid == 0) mask[nblk] = 0ull;
        __syncthreads();
        uint64_t off = 0;
        for (uint32_t j = 0; j < (uint32_t)kBlock; ++j) off += j < tid ? part[j] : 0ull;   // (one address per step: a broadcast)
        for (uint32_t b = b0; b < b1; ++b) {
            cs[b] = off;
            off += h[b];
        }
        if (tid == kBlock - 1) cs[nb] = off;
        for (uint32_t k = tid; k <= nblk; k += kBlock) {
            uint32_t a = 0;
            for (uint32_t j = 0; j < nblk; ++j) a += j < k ? (uint32_t)__popcll(mask[j]) : 0u;
            bcnt[k] = a;
        }
        __syncthreads();
    }
    // ---- candidates below `levels` are not admissible
    for (uint32_t i = chunk + tid * C; i < L; i += kBlock * C) out[i] = INFINITY;

    const uint64_t N = cs[nb];
    const double dN = (double)(long long)N;
    const uint32_t first = L + (chunk + C - L % C) % C;   // the lowest candidate >= levels of this chunk (i % C == chunk)
    for (uint32_t i = first + wave * C; i <= nb; i += (kBlock / kWave) * C) {
        // per candidate (wave-uniform)
        const uint64_t csi = cs[i];
        const uint64_t outl = N - csi;                      // the outliers, folded into bin i - 1 of p
        const uint32_t s_last = (uint32_t)(((uint64_t)(L - 1u) * i) / L);
        const uint32_t woke = (csi == cs[i - 1] && outl != 0ull) ? 1u : 0u;   // bin i - 1 is empty and live through the outliers alone
        const uint32_t n1p = kl_live_below(mask, bcnt, i) + woke;
        const uint32_t n1q = n1p - ((csi == cs[s_last] && outl != 0ull) ? 1u : 0u);   // (q of that bin is zero: its group holds no mass)
        double res = INFINITY;
        if (n1p != 0u && n1q != 0u) {
            const uint32_t zp = i - n1p, zq = i - n1q;
            const double e1p = kKlEps * (double)zp / (double)n1p;
            const double e1q = kKlEps * (double)zq / (double)n1q;
            if (e1p < 1.0 && e1q < 1.0) {
                const double Sp = dN - (double)n1p * e1p + (double)zp * kKlEps;
                const double Sq = (double)(long long)csi - (double)n1q * e1q + (double)zq * kKlEps;
                double acc = 0.0;
                for (uint32_t b = lane; b < i; b += kWave) {
                    uint64_t pb = cs[b + 1] - cs[b];
                    if (b == i - 1u) pb += outl;
                    if (pb != 0ull) {
                        const uint32_t g = ((b + 1u) * L - 1u) / i;      // (at most 2^28: bins, levels <= 16384)
                        const uint32_t s0 = (g * i) / L, s1 = ((g + 1u) * i) / L;
                        const uint64_t G = cs[s1] - cs[s0];
                        double qs = kKlEps;
                        if (G != 0ull) {
                            const uint32_t live = kl_live_below(mask, bcnt, s1) - kl_live_below(mask, bcnt, s0) + (s1 == i ? woke : 0u);
                            qs = (double)(long long)G / (double)live - e1q;
                        }
                        const double P = ((double)(long long)pb - e1p) / Sp, Q = qs / Sq;
                        acc += P * log(P / Q);
                    }
                }
                acc = wave_sum(acc);
                const double Pz = kKlEps / Sp, Qz = kKlEps / Sq;     // the zp bins where p (and with it q) is zero
                res = acc + (double)zp * (Pz * log(Pz / Qz));
            }
        }
        if (lane == 0) out[i] = res;
    }
}

// One wave per tensor: the lowest candidate with the least divergence (NaN never wins; -1: none is admissible) and its clip.
__global__ __launch_bounds__(kWave) void k_hist_kl_pick(const double* __restrict__ div, const float* __restrict__ gmin_a,
                                                         const float* __restrict__ gmax_a, int bins, int32_t* __restrict__ best,
                                                         float* __restrict__ clip) {
    const int slot = blockIdx.x;
    const int lane = threadIdx.x;
    const double* __restrict__ d = div + (uint64_t)slot * ((uint64_t)bins + 1u);
    double bv = INFINITY;
    int bi = -1;
    for (int i = lane; i <= bins; i += kWave) {
        const double v = d[i];
        if (v < bv) {   // (ascending i: the first of equal values stays)
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, kWave);
        const int oi = __shfl_xor(bi, o, kWave);
        if (ov < bv || (ov == bv && oi >= 0 && (bi < 0 || oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        best[slot] = bi;
        store_bin_clip(bi >= 0 ? bi - 1 : -1, gmin_a[slot], gmax_a[slot], bins, clip + 2 * slot);
    }
}

// ================================================================ K4c: quantisation-MSE clip — beyond the reference
// The definition is this project's own (tests/qmse_model.py), in units of half a bin width: bin b's centre is
// m = 2 b + 1, candidate i in [first, bins] clips at t = 2 i - 1 (the centre of bin i - 1) with scale t / top; u = m top / t,
// Q = the grid point nearest to min(u, top), and out[i] = sum_b h[b] (u - Q)^2 * (t / (2 top))^2 / N.  The grid is a
// compile-time parameter: the integers 0 .. top, or the non-negative finite E4M3 codes (top = 448).
//
// Geometry of k_hist_kl: grid = (candidate chunk, tensor); the tensor's row staged once in LDS, here as fp64 counts (exact:
// < 2^53; 8 B per bin, 128 KB at 16384 bins); one wave per candidate at a time, lanes own bins, bins without a count skipped.
// Per bin everything but the choice of Q is exact in fp64: a = unit m top and Q' t (unit = 1, or 512 on E4M3, whose codes are
// multiples of 2^-9: Q' = 512 Q) are integers below 2^53, so unit (u - Q) t = a - Q' t carries no rounding, whichever Q was
// chosen.  The choice itself, from u = a * fl(1 / t) (the reciprocal is wave-uniform and stays out of the loop), is the right
// one: u is within 3 ulp of the quotient (1e-11 at most, u <= top <= 32767 being all that matters), and no quotient comes
// nearer to a midpoint of the grid than 1 / (2 t) > 1e-5 (uniform) or 1 / (1024 t) > 1e-8 (E4M3), never onto one
// (qmse_model.py).  E4M3 in fp64: the
// exponent field, clamped at the subnormal binade, gives the power-of-two step; rint does the rest.  Saturation (u >= top) is
// the same formula.  Every candidate costs the same: they are dealt round-robin.  A lane adds its bins in ascending order, the
// 64 partial sums meet in the fixed wave_sum tree, one lane stores: no floating-point atomics, two calls give the same bits,
// and a candidate's value does not depend on the launch's geometry.
constexpr int kGridUniform = DPL_GRID_UNIFORM, kGridE4M3 = DPL_GRID_E4M3;

template <int GRID>
__global__ __launch_bounds__(kBlock) void k_hist_qmse(const uint64_t* __restrict__ hist, int bins, int first, int top, int n_chunks,
                                                       double* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double qm_lds[];
    double* hd = qm_lds;                                            // [bins] the counts
    uint64_t* part = reinterpret_cast<uint64_t*>(hd + bins);        // [kBlock / kWave] the waves' totals
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t slot = blockIdx.x / (uint32_t)n_chunks, chunk = blockIdx.x % (uint32_t)n_chunks;
    const uint64_t* __restrict__ h = hist + (uint64_t)slot * (uint64_t)bins;
    double* __restrict__ out = err + (uint64_t)slot * ((uint64_t)bins + 1u);
    const uint32_t F = (uint32_t)first, C = (uint32_t)n_chunks, nb = (uint32_t)bins;

    uint64_t s = 0;
    for (uint32_t b = tid; b < nb; b += kBlock) {
        const uint64_t v = h[b];
        s += v;
        hd[b] = (double)(long long)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);   // (integers: any order)
    if (lane == 0) part[wave] = s;
    __syncthreads();
    uint64_t N = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) N += part[w];

    // ---- candidates below `first` are not searched
    for (uint32_t i = chunk + tid * C; i < F; i += kBlock * C) out[i] = INFINITY;

    constexpr double unit = GRID == kGridE4M3 ? 512.0 : 1.0;
    const double dtop = GRID == kGridE4M3 ? 448.0 : (double)top;
    const double atop = unit * dtop;                                // a = m * atop
    const double norm = (double)(long long)N * (4.0 * atop * atop);
    for (uint32_t i = F + chunk + wave * C; i <= nb; i += (kBlock / kWave) * C) {
        const double t = (double)(2u * i - 1u);
        const double rt = 1.0 / (unit * t);                         // u = a * rt
        double acc = 0.0;
        if (N != 0ull) {
            for (uint32_t b = lane; b < nb; b += kWave) {
                const double hb = hd[b];
                if (hb != 0.0) {
                    const double a = (double)(2u * b + 1u) * atop;
                    const double v = fmin(a * rt, dtop);
                    double q;                                       // unit * Q
                    if (GRID == kGridE4M3) {
                        int e = (int)((__double_as_longlong(v) >> 52) & 0x7FF) - 1023;      // v's binade (v > 0)
                        e = e < -6 ? -6 : e;                        // the subnormal binade's step: 2^-9
                        const double istep = __longlong_as_double((long long)(1023 + 3 - e) << 52);      // 1 / step = 2^(3 - e)
                        const double step512 = __longlong_as_double((long long)(1023 + 9 - 3 + e) << 52);  // 512 step
                        q = rint(v * istep) * step512;
                    } else {
                        q = rint(v);
                    }
                    const double dt = a - q * t;                    // unit * (u - Q) * t, exact
                    acc += hb * (dt * dt);
                }
            }
            acc = wave_sum(acc);
        }
        if (lane == 0) out[i] = N != 0ull ? acc / norm : INFINITY;
    }
}

// ================================================================ K5: per-row min / max of a [rows, cols] matrix
__global__ __launch_bounds__(kBlock) void k_rowwise_minmax(const float* __restrict__ w, int64_t cols,
                                                            float* __restrict__ omn, float* __restrict__ omx) {
    __shared__ float s_mn[kBlock / kWave], s_mx[kBlock / kWave];
    __shared__ uint32_t s_nan[kBlock / kWave];
    const float* p = w + (int64_t)blockIdx.x * cols;
    MinMaxOp op{INFINITY, -INFINITY, 0u};
    // rows can be longer than 2^32 only in theory; weights are at most a few 10^7 elements
    stream_span(p, (uint32_t)cols, op);
    float mn = wave_min(op.mn), mx = wave_max(op.mx);
    uint32_t nn = __any(op.nan) ? 1u : 0u;
    const int wv = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_mn[wv] = mn;
        s_mx[wv] = mx;
        s_nan[wv] = nn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / kWave; ++k) {
            mn = fminf(mn, s_mn[k]);
            mx = fmaxf(mx, s_mx[k]);
            nn |= s_nan[k];
        }
        omn[blockIdx.x] = nn ? NAN : mn;
        omx[blockIdx.x] = nn ? NAN : mx;
    }
}

// ================================================================ K5b: per-column running max |x| of a [rows, cols] matrix
// acc[c] = max(acc[c], max_r |x[r, c]|) as an UNSIGNED-INTEGER maximum on the bit pattern of |x|: non-negative floats order like
// their bits and every NaN pattern lies above +inf, so a NaN in a column (or already in acc) stays a NaN, -0.0 counts as +0.0,
// and the result does not depend on the order in which workgroups arrive (no floating-point atomic).
// Geometry: a workgroup is tw lanes along the columns (tw = 2^k <= 64; a lane owns T = one float, or four with 16-B loads) by
// 256 / tw rows; blockIdx.x picks the column tile, blockIdx.y the rows, grid-strided, kColUnroll independent loads in flight per
// lane.  A lane keeps its columns' maximum in registers over the whole row loop, the 256 / tw lanes that share a column are
// folded in LDS, and lane row 0 issues at most ONE atomicMax per column and workgroup — none where the running value read
// beforehand is not below the candidate (acc only grows, so a stale read can only cause a redundant atomic, never a lost one).
constexpr int kColMaxLanes = 64;     // 64 lanes x 16 B: a wave instruction reads 1 KiB contiguous of one row
constexpr int kColUnroll = 4;
constexpr int kColMaxBlocks = 2048;  // 8 workgroups per CU
using u4 = __attribute__((ext_vector_type(4))) uint32_t;

template <class T>   // uint32_t: one column per lane;  u4: four, cols % 4 == 0 and x 16-byte aligned
__global__ __launch_bounds__(kBlock) void k_colwise_absmax(const T* __restrict__ x_generic, uint64_t rows, uint64_t cv, uint32_t tw,
                                                            uint32_t* __restrict__ acc) {
    __shared__ T s_m[kBlock];
    const __attribute__((address_space(1))) T* x = (const __attribute__((address_space(1))) T*)x_generic;
    const uint32_t tid = threadIdx.x, rp = kBlock / tw;
    const uint64_t c = (uint64_t)blockIdx.x * tw + (tid & (tw - 1));     // this lane's (vector) column; cv of them in a row
    T m = T(0);
    if (c < cv) {
        const uint64_t step = (uint64_t)gridDim.y * rp;
        for (uint64_t r = (uint64_t)blockIdx.y * rp + tid / tw; r < rows; r += kColUnroll * step) {
            T v[kColUnroll];
#pragma unroll
            for (int u = 0; u < kColUnroll; ++u) {
                const uint64_t rr = r + u * step;       // past the end: the last row once more (a branch here would serialise the loads)
                v[u] = __builtin_nontemporal_load(x + (rr < rows ? rr : rows - 1) * cv + c);
            }
#pragma unroll
            for (int u = 0; u < kColUnroll; ++u) m = __builtin_elementwise_max(m, v[u] & T(0x7FFFFFFFu));
        }
    }
    s_m[tid] = m;
    __syncthreads();
    for (uint32_t h = kBlock / 2; h >= tw; h >>= 1) {      // tid and tid + h (h a multiple of tw) share a column
        if (tid < h) s_m[tid] = __builtin_elementwise_max(s_m[tid], s_m[tid + h]);
        __syncthreads();
    }
    if (tid < tw && c < cv) {
        m = s_m[tid];
        if constexpr (sizeof(T) == 16) {
            uint32_t* a = acc + 4 * c;
            const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];     // (acc is only 4-byte aligned: four loads, issued together)
            if (m.x > a0) atomicMax(a + 0, m.x);
            if (m.y > a1) atomicMax(a + 1, m.y);
            if (m.z > a2) atomicMax(a + 2, m.z);
            if (m.w > a3) atomicMax(a + 3, m.w);
        } else {
            if (m > acc[c]) atomicMax(acc + c, m);
        }
    }
}

// ================================================================ K6: fused quantize -> dequantize
__device__ __forceinline__ float fq_one(float x, float scale, float zp, float qlo, float qhi) {
    float q = __fadd_rn(rintf(__fdiv_rn(x, scale)), zp);  // round half to even, then zero point
    q = fminf(fmaxf(q, qlo), qhi);                        // saturate
    return __fmul_rn(__fsub_rn(q, zp), scale);
}

// The OCP FP8 E4M3 ("e4m3fn": bias 7, 3 mantissa bits, subnormal step 2^-9, largest finite 448, no infinities) Q/DQ of one value:
// the nearest e4m3fn value of v as fp32, round half to even (subnormals too), SATURATING (|v| > 448 and +-inf give +-448: ONNX
// QuantizeLinear, saturate = 1), NaN stays NaN, the sign of zero is kept.  In fp32 arithmetic on the value's own exponent bits: a
// value of binade e lies on a grid of step 2^(max(e, -6) - 3); |v| times the inverse step is exact (a power of two), v_rndne
// rounds it half to even, times the step is exact again (a carry into the next binade lands on a value of the format).  Every
// fp32 subnormal rounds to zero whether or not the multiply flushes it.  gfx950's v_cvt_pk_fp8_f32 / v_cvt_f32_fp8 would do the
// same in two instructions; how they round subnormals and what they return above 448 and for NaN has not been measured on this
// hardware (scripts/fp8_cvt_probe.hip measures it), and the kernel is bound by its 8 B per element, not by these
// eight operations.
__device__ __forceinline__ float e4m3_round(float v) {
    const float a = fminf(fabsf(v), 448.f);            // saturate (a NaN comes out finite here: routed below)
    uint32_t e = __float_as_uint(a) >> 23;             // biased exponent: binade e - 127
    e = e < 121u ? 121u : e;                           // below 2^-6 the step stays 2^-9
    const float step = __uint_as_float((e - 3u) << 23), inv = __uint_as_float((257u - e) << 23);      // 2^(e-130), 2^(130-e)
    const float r = copysignf(__fmul_rn(rintf(__fmul_rn(a, inv)), step), v);
    return v != v ? v : r;
}

// The number format of the Q/DQ pair, a compile-time parameter of the streaming skeleton below beside PRE: kFqFmtInt the integer
// grid of fq_one (scale, zero point, [qlo, qhi]); kFqFmtE4M3 y = fl32(e4m3_round(fl32(x / scale)) * scale) — the same shape, two
// single fp32 operations around the rounding; zero point / qlo / qhi are not read (zp_p may be null).
enum { kFqFmtInt = 0, kFqFmtE4M3 = 1 };
template <int FMT>
__device__ __forceinline__ float fq_elem(float x, float scale, float zp, float qlo, float qhi) {
    if (FMT == kFqFmtE4M3) return __fmul_rn(e4m3_round(__fdiv_rn(x, scale)), scale);
    return fq_one(x, scale, zp, qlo, qhi);
}
template <int FMT>
__device__ __forceinline__ float fq_zp(const int32_t* __restrict__ zp_p, uint32_t c) {
    return FMT == kFqFmtInt ? (float)zp_p[c] : 0.f;
}

// What the producer of a fake-quantised tensor would have written, applied on the way in (the reference's merge-ReLU rule puts
// most activation Q/DQ pairs directly behind a ReLU, quantize.py:50-55): kFqPreNone x; kFqPreRelu torch.relu(x) = np.maximum(x, 0)
// (NaN stays NaN; -0 and +0 quantise alike on an integer grid, FP8 keeps the zero's sign); kFqPreAddRelu relu(x + x2), the residual Add of a bottleneck and its ReLU (one fp32
// addition, rounded to nearest, as torch.add).
enum { kFqPreNone = 0, kFqPreRelu = 1, kFqPreAddRelu = 2 };
template <int PRE>
__device__ __forceinline__ float fq_pre(float x, float x2) {
    if (PRE == kFqPreAddRelu) x = __fadd_rn(x, x2);
    if (PRE != kFqPreNone) x = x < 0.f ? 0.f : x;
    return x;
}

// One workgroup fake-quantises elements [e0, e0 + cnt) of a tensor viewed as [outer, n_channels, inner] (n_channels == 1: per
// tensor).  A CONTIGUOUS chunk per workgroup (few large equal shares stream faster from HBM than a grid-stride walk), four
// 16-byte vectors per lane in flight, non-temporal loads and stores (each byte is touched once).  The channel of a vector needs no
// division in the loop: a lane's (column, channel) advance by a constant per step — 1024 elements = (1024 / inner) rows and
// (1024 % inner) columns, both computed once per chunk on the scalar unit — with one conditional wrap each.
template <int PRE, int FMT>
__device__ __forceinline__ void fq_span(const float* __restrict__ x, const float* __restrict__ x2, float* __restrict__ y, uint64_t e0,
                                        uint32_t cnt, const float* __restrict__ scale_p, const int32_t* __restrict__ zp_p,
                                        uint32_t n_channels, uint32_t inner, float qlo, float qhi) {
    typedef __attribute__((address_space(1))) f4* gptr_f4w;
    const uint32_t tid = threadIdx.x;
    const float* xs = x + e0;
    const float* x2s = PRE == kFqPreAddRelu ? x2 + e0 : xs;
    float* ys = y + e0;
    // 16-byte vectors whatever the rows' length: a vector of a row that is no multiple of four long (7 x 7 maps: 49) may straddle two
    // channels — it carries the parameters of both and picks per element (rows shorter than a vector: element by element)
    const bool vec = ((((uintptr_t)xs | (uintptr_t)x2s | (uintptr_t)ys) & 15u) == 0u) && (n_channels == 1u || inner >= 4u);
    if (!vec) {   // unaligned views / rows shorter than a vector: element by element, same bookkeeping
        const uint64_t e = e0 + tid;
        uint32_t col = (uint32_t)(e % inner), c = (uint32_t)((e / inner) % n_channels);
        const uint32_t step_cols = (uint32_t)kBlock % inner, step_ch = ((uint32_t)kBlock / inner) % n_channels;
        for (uint32_t i = tid; i < cnt; i += kBlock) {
            ys[i] = fq_elem<FMT>(fq_pre<PRE>(xs[i], x2s[i]), scale_p[c], fq_zp<FMT>(zp_p, c), qlo, qhi);
            col += step_cols;
            c += step_ch;
            if (col >= inner) {
                col -= inner;
                c += 1u;
            }
            if (c >= n_channels) c -= n_channels;
        }
        return;
    }
    const uint32_t nvec = cnt >> 2;
    gptr_f4 xv = (gptr_f4)xs;
    gptr_f4 x2v = (gptr_f4)x2s;
    gptr_f4w yv = (gptr_f4w)ys;
    // Two register sets in rotation (as stream_span): the NEXT four vectors of a lane — and, per channel, their parameters — are
    // requested before the current four are computed and stored: eight loads in flight per lane, and a parameter look-up never
    // sits between a vector's arrival and its use.
    const bool per_channel = n_channels != 1u;
    uint32_t col = 0u, c = 0u, step_cols = 0u, step_ch = 0u;
    if (per_channel) {   // the lane's first vector: one division; then (col, c) advance by the per-step constants
        const uint64_t e = e0 + 4ull * tid;
        col = (uint32_t)(e % inner);
        c = (uint32_t)((e / inner) % n_channels);
        step_cols = (4u * kBlock) % inner;
        step_ch = ((4u * kBlock) / inner) % n_channels;
    }
    const float sc1 = scale_p[0], zp1 = fq_zp<FMT>(zp_p, 0u);
    const bool straddle = per_channel && (inner & 3u) != 0u;   // (uniform) a vector may end in the next channel's row
    struct Set {
        f4 v[4];
        f4 w[PRE == kFqPreAddRelu ? 4 : 1];   // the second operand of the residual Add
        float sc[4], sc2[4];
        int32_t zp[4], zp2[4];
        uint32_t left[4];   // elements of the vector that still belong to the first channel's row (>= 4: all of them)
    };
    auto load = [&](Set& st, uint32_t i0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            st.v[u] = i0 + u * kBlock < nvec ? __builtin_nontemporal_load(xv + i0 + u * kBlock) : f4{0.f, 0.f, 0.f, 0.f};
            if (PRE == kFqPreAddRelu)
                st.w[PRE == kFqPreAddRelu ? u : 0] =
                    i0 + u * kBlock < nvec ? __builtin_nontemporal_load(x2v + i0 + u * kBlock) : f4{0.f, 0.f, 0.f, 0.f};
            if (per_channel) {   // (uniform)
                st.sc[u] = scale_p[c];
                if (FMT == kFqFmtInt) st.zp[u] = zp_p[c];
                if (straddle) {
                    const uint32_t cn = c + 1u < n_channels ? c + 1u : 0u;
                    st.sc2[u] = scale_p[cn];
                    if (FMT == kFqFmtInt) st.zp2[u] = zp_p[cn];
                    st.left[u] = inner - col;
                }
                col += step_cols;
                c += step_ch;
                if (col >= inner) {
                    col -= inner;
                    c += 1u;
                }
                if (c >= n_channels) c -= n_channels;
            }
        }
    };
    auto eat = [&](Set& st, uint32_t i0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * kBlock < nvec) {
                const float sc = per_channel ? st.sc[u] : sc1, zp = per_channel && FMT == kFqFmtInt ? (float)st.zp[u] : zp1;
                if (PRE != kFqPreNone) {
                    const f4 w = st.w[PRE == kFqPreAddRelu ? u : 0];
                    st.v[u].x = fq_pre<PRE>(st.v[u].x, w.x);
                    st.v[u].y = fq_pre<PRE>(st.v[u].y, w.y);
                    st.v[u].z = fq_pre<PRE>(st.v[u].z, w.z);
                    st.v[u].w = fq_pre<PRE>(st.v[u].w, w.w);
                }
                if (straddle) {   // (uniform)
                    const float scb = st.sc2[u], zpb = FMT == kFqFmtInt ? (float)st.zp2[u] : 0.f;
                    const uint32_t l = st.left[u];
                    st.v[u].x = fq_elem<FMT>(st.v[u].x, sc, zp, qlo, qhi);
                    st.v[u].y = fq_elem<FMT>(st.v[u].y, l > 1u ? sc : scb, l > 1u ? zp : zpb, qlo, qhi);
                    st.v[u].z = fq_elem<FMT>(st.v[u].z, l > 2u ? sc : scb, l > 2u ? zp : zpb, qlo, qhi);
                    st.v[u].w = fq_elem<FMT>(st.v[u].w, l > 3u ? sc : scb, l > 3u ? zp : zpb, qlo, qhi);
                } else {
                    st.v[u].x = fq_elem<FMT>(st.v[u].x, sc, zp, qlo, qhi);
                    st.v[u].y = fq_elem<FMT>(st.v[u].y, sc, zp, qlo, qhi);
                    st.v[u].z = fq_elem<FMT>(st.v[u].z, sc, zp, qlo, qhi);
                    st.v[u].w = fq_elem<FMT>(st.v[u].w, sc, zp, qlo, qhi);
                }
                __builtin_nontemporal_store(st.v[u], yv + i0 + u * kBlock);
            }
        }
    };
    if (tid < nvec) {
        Set A, B;
        uint32_t i0 = tid;
        load(A, i0);
        for (;;) {
            uint32_t nx = i0 + 4 * kBlock;
            const bool hb = nx < nvec;
            if (hb) load(B, nx);
            eat(A, i0);
            if (!hb) break;
            i0 = nx;
            nx = i0 + 4 * kBlock;
            const bool ha = nx < nvec;
            if (ha) load(A, nx);
            eat(B, i0);
            if (!ha) break;
            i0 = nx;
        }
    }
    const uint32_t t = (nvec << 2) + tid;   // (a chunk that is no multiple of four long: the tensor's last elements)
    if (t < cnt) {
        const uint32_t c = n_channels == 1u ? 0u : (uint32_t)(((e0 + t) / inner) % n_channels);
        ys[t] = fq_elem<FMT>(fq_pre<PRE>(xs[t], x2s[t]), scale_p[c], fq_zp<FMT>(zp_p, c), qlo, qhi);
    }
}

// one tensor: workgroup b takes elements [b * chunk, (b + 1) * chunk) (chunk a multiple of 1024)
// (PRE: the producer's ReLU / Add + ReLU on the way in, fq_pre; x2 is read for kFqPreAddRelu only.  FMT: the number format, fq_elem)
template <int PRE, int FMT>
__global__ __launch_bounds__(kBlock) void k_fake_quant(const float* __restrict__ x, const float* __restrict__ x2, float* __restrict__ y,
                                                        uint64_t n, uint64_t chunk, const float* __restrict__ scale_p,
                                                        const int32_t* __restrict__ zp_p, uint32_t n_channels, uint32_t inner, float qlo,
                                                        float qhi) {
    const uint64_t e0 = (uint64_t)blockIdx.x * chunk;
    if (e0 >= n) return;
    const uint64_t cnt = n - e0 < chunk ? n - e0 : chunk;
    fq_span<PRE, FMT>(x, x2, y, e0, (uint32_t)cnt, scale_p, zp_p, n_channels, inner, qlo, qhi);
}

// a whole tensor set in ONE launch: the balanced partition's items (item.seg = tensor, item.offset / count = the elements) over
// the tensors' base pointers and a parameter row per tensor
template <int FMT>
__global__ __launch_bounds__(kBlock) void k_fake_quant_items(const dpl_work_item* __restrict__ items, const uint32_t* __restrict__ bb,
                                                              const float* const* __restrict__ seg_x, float* const* __restrict__ seg_y,
                                                              const dpl_fake_quant_params* __restrict__ prm) {
    uint32_t k0, k1;
    block_items(bb, k0, k1);
    for (uint32_t k = k0; k < k1; ++k) {
        const dpl_work_item it = items[k];
        const dpl_fake_quant_params p = prm[it.seg];
        fq_span<kFqPreNone, FMT>(seg_x[it.seg], nullptr, seg_y[it.seg], it.offset, it.count, p.d_scale, p.d_zero_point, (uint32_t)p.n_channels, (uint32_t)p.inner,
                (float)p.qlo, (float)p.qhi);
    }
}

// ================================================================ N1: cosine-similarity partial sums
__global__ __launch_bounds__(kBlock) void k_cos_acc(const float* __restrict__ a, const float* __restrict__ b,
                                                     int64_t n, double* __restrict__ acc) {
    __shared__ double s_r[3][kBlock / kWave];
    double ab = 0.0, aa = 0.0, bb = 0.0;
    const int64_t nvec = n >> 2;
    const f4* av = reinterpret_cast<const f4*>(a);
    const f4* bv = reinterpret_cast<const f4*>(b);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < nvec; i0 += 4 * stride) {
        f4 p[4], q[4];   // eight 16-byte loads in flight per lane
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            p[u] = i < nvec ? __builtin_nontemporal_load(av + i) : f4{0.f, 0.f, 0.f, 0.f};
            q[u] = i < nvec ? __builtin_nontemporal_load(bv + i) : f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ab += (double)p[u].x * q[u].x + (double)p[u].y * q[u].y + (double)p[u].z * q[u].z + (double)p[u].w * q[u].w;
            aa += (double)p[u].x * p[u].x + (double)p[u].y * p[u].y + (double)p[u].z * p[u].z + (double)p[u].w * p[u].w;
            bb += (double)q[u].x * q[u].x + (double)q[u].y * q[u].y + (double)q[u].z * q[u].z + (double)q[u].w * q[u].w;
        }
    }
    const int64_t t = (nvec << 2) + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) {
        ab += (double)a[t] * b[t];
        aa += (double)a[t] * a[t];
        bb += (double)b[t] * b[t];
    }
    ab = wave_sum(ab);
    aa = wave_sum(aa);
    bb = wave_sum(bb);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_r[0][w] = ab;
        s_r[1][w] = aa;
        s_r[2][w] = bb;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = 0.0;
        for (int k = 0; k < kBlock / kWave; ++k) v += s_r[threadIdx.x][k];
        atomicAdd(acc + threadIdx.x, v);
    }
}

// ================================================================ N2: per-channel sum of (a - b)  (bias correction)
// a, b viewed as [outer, C, inner] (Conv output [n, C, H, W]; Gemm output [n, C] with inner = 1):
// acc[c] += sum over outer and inner of (a - b), in fp64.  One wave per (outer, channel) row, rows round-robin over
// the waves of the launch; 16-byte loads when the rows allow it.
__global__ __launch_bounds__(kBlock) void k_channel_diff_sum(const float* __restrict__ a, const float* __restrict__ b,
                                                              uint64_t rows, uint32_t n_channels, uint32_t inner,
                                                              int vec_ok, double* __restrict__ acc) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
    if (inner == 1) {  // [n, C]: lanes over channels, waves over rows of 64 channels
        const uint64_t chunks = (n_channels + kWave - 1) / kWave;
        for (uint64_t t = wave; t < chunks; t += n_waves) {
            const uint32_t c = (uint32_t)t * kWave + lane;
            if (c >= n_channels) continue;
            double d = 0.0;
            for (uint64_t r = 0; r < rows / n_channels; ++r) d += (double)a[r * n_channels + c] - (double)b[r * n_channels + c];
            atomicAdd(acc + c, d);
        }
        return;
    }
    for (uint64_t r = wave; r < rows; r += n_waves) {
        const float* pa = a + r * inner;
        const float* pb = b + r * inner;
        double d = 0.0;
        uint32_t i = 0;
        if (vec_ok) {  // inner % 4 == 0 and both bases 16-byte aligned: every row starts aligned
            const f4* va = reinterpret_cast<const f4*>(pa);
            const f4* vb = reinterpret_cast<const f4*>(pb);
            const uint32_t nv = inner >> 2;
            for (uint32_t j = lane; j < nv; j += 2 * kWave) {
                const f4 p0 = __builtin_nontemporal_load(va + j), q0 = __builtin_nontemporal_load(vb + j);
                const bool two = j + kWave < nv;
                const f4 p1 = two ? __builtin_nontemporal_load(va + j + kWave) : f4{0.f, 0.f, 0.f, 0.f};
                const f4 q1 = two ? __builtin_nontemporal_load(vb + j + kWave) : f4{0.f, 0.f, 0.f, 0.f};
                d += ((double)p0.x - (double)q0.x) + ((double)p0.y - (double)q0.y) + ((double)p0.z - (double)q0.z) +
                     ((double)p0.w - (double)q0.w);
                d += ((double)p1.x - (double)q1.x) + ((double)p1.y - (double)q1.y) + ((double)p1.z - (double)q1.z) +
                     ((double)p1.w - (double)q1.w);
            }
            i = nv << 2;
        }
        for (uint32_t j = i + lane; j < inner; j += kWave) d += (double)pa[j] - (double)pb[j];
        d = wave_sum(d);
        if (lane == 0) atomicAdd(acc + (uint32_t)(r % n_channels), d);
    }
}

// Per-slot cosine partial sums over work items: slot = (image, tensor) pair for the profiling flow
// (profiling.py:57-64: one cosine per image per quantised layer output).  a and b come from two segment
// tables with identical geometry (fp model vs fake-quantised model).
__global__ __launch_bounds__(kBlock) void k_cos_items(const dpl_work_item* __restrict__ items,
                                                       const uint32_t* __restrict__ bb,
                                                       const float* const* __restrict__ segs_a,
                                                       const float* const* __restrict__ segs_b,
                                                       double* __restrict__ acc) {
    __shared__ double s_r[3][kBlock / kWave];
    uint32_t k0, k1;
    block_items(bb, k0, k1);
    for (uint32_t k = k0; k < k1; ++k) {
        const dpl_work_item it = items[k];
        gptr_f32 a = (gptr_f32)(segs_a[it.seg] + it.offset);
        gptr_f32 b = (gptr_f32)(segs_b[it.seg] + it.offset);
        const uint32_t n = it.count;
        double ab = 0.0, aa = 0.0, bbs = 0.0;
        const bool vec = ((((uintptr_t)(segs_a[it.seg] + it.offset)) | ((uintptr_t)(segs_b[it.seg] + it.offset))) & 15u) == 0;
        uint32_t done = 0;
        if (vec) {
            const uint32_t nvec = n >> 2;
            gptr_f4 av = (gptr_f4)a;
            gptr_f4 bv = (gptr_f4)b;
            // two streams, software pipelined like stream_span: the next 2 + 2 vectors per lane are in flight while
            // the current ones are consumed (ping-pong register sets, no register copy between them)
            constexpr int kU = 2;
            constexpr uint32_t kStride = kU * kBlock;
            auto eat1 = [&](const f4& p, const f4& q) {
                ab += (double)p.x * q.x + (double)p.y * q.y + (double)p.z * q.z + (double)p.w * q.w;
                aa += (double)p.x * p.x + (double)p.y * p.y + (double)p.z * p.z + (double)p.w * p.w;
                bbs += (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w;
            };
#define DPL_CLOAD(P, Q, base)                                      \
    _Pragma("unroll") for (int u = 0; u < kU; ++u) {               \
        P[u] = __builtin_nontemporal_load(av + (base) + u * kBlock); \
        Q[u] = __builtin_nontemporal_load(bv + (base) + u * kBlock); \
    }
#define DPL_CEAT(P, Q) _Pragma("unroll") for (int u = 0; u < kU; ++u) eat1(P[u], Q[u])
            uint32_t i = threadIdx.x;
            if (i + (kU - 1) * kBlock < nvec) {
                f4 PA[kU], QA[kU], PB[kU], QB[kU];
                DPL_CLOAD(PA, QA, i);
                i += kStride;
                for (;;) {
                    if (!(i + (kU - 1) * kBlock < nvec)) {
                        DPL_CEAT(PA, QA);
                        break;
                    }
                    DPL_CLOAD(PB, QB, i);
                    i += kStride;
                    DPL_CEAT(PA, QA);
                    if (!(i + (kU - 1) * kBlock < nvec)) {
                        DPL_CEAT(PB, QB);
                        break;
                    }
                    DPL_CLOAD(PA, QA, i);
                    i += kStride;
                    DPL_CEAT(PB, QB);
                }
            }
#undef DPL_CLOAD
#undef DPL_CEAT
            for (; i < nvec; i += kBlock) eat1(__builtin_nontemporal_load(av + i), __builtin_nontemporal_load(bv + i));
            done = nvec << 2;
        }
        for (uint32_t i = done + threadIdx.x; i < n; i += kBlock) {
            const float p = a[i], q = b[i];
            ab += (double)p * q;
            aa += (double)p * p;
            bbs += (double)q * q;
        }
        ab = wave_sum(ab);
        aa = wave_sum(aa);
        bbs = wave_sum(bbs);
        const int w = threadIdx.x / kWave;
        if ((threadIdx.x & (kWave - 1)) == 0) {
            s_r[0][w] = ab;
            s_r[1][w] = aa;
            s_r[2][w] = bbs;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            double v = 0.0;
            for (int j = 0; j < kBlock / kWave; ++j) v += s_r[threadIdx.x][j];
            atomicAdd(acc + 3 * (uint64_t)it.slot + threadIdx.x, v);
        }
        __syncthreads();
    }
}

// one tensor in either number format (FMT: kFqFmtInt / kFqFmtE4M3; `who`: the entry point's name, for the messages)
template <int FMT>
int fake_quant_launch(const char* who, int32_t pre, const float* d_x, const float* d_x2, float* d_y, int64_t n, const float* d_scale,
                      const int32_t* d_zp, int64_t n_channels, int64_t inner, int32_t qlo, int32_t qhi, dpl_stream_t s) {
    auto bad = [who](const char* what) {
        char m[192];
        snprintf(m, sizeof(m), "%s: %s", who, what);
        return fail_msg(m);
    };
    if (pre != DPL_FQ_PRE_NONE && pre != DPL_FQ_PRE_RELU && pre != DPL_FQ_PRE_ADD_RELU)
        return bad("pre must be DPL_FQ_PRE_NONE, _RELU or _ADD_RELU");
    if (n <= 0) return 0;
    if (pre == DPL_FQ_PRE_ADD_RELU && d_x2 == nullptr) return bad("DPL_FQ_PRE_ADD_RELU needs d_x2");
    if (n_channels < 1 || inner < 1 || n_channels > 0xFFFFFFFFll || inner > 0xFFFFFFFFll)
        return bad("n_channels and inner must be in [1, 2^32)");
    // A contiguous chunk of 3072 elements (12 KiB read + 12 KiB written) per workgroup, whatever the tensor's size (a multiple of
    // 1024 elements: every chunk starts on a 16-byte boundary of an aligned tensor).  Measured on the tensors a fake-quantised
    // ResNet-50 forward at batch 64 runs this on (26 - 205 MB, distinct buffers in rotation), fraction of
    // 8 TB/s by chunk: 1024: 0.61 / 0.52 (205 MB / 26 MB), 2048: 0.72 / 0.57, 3072: 0.76 / 0.56, 4096: 0.75 / 0.54, 8192: 0.78 /
    // 0.54, 12288: 0.72 / 0.43 — and rounds 3 - 4's rule (n / 4096 elements, at least 4096: 50 KB chunks for a 205 MB tensor):
    // 0.70 / 0.54.  The Q/DQ nodes of that forward: 0.61 -> 0.65 of the roofline (bench.py `fake_quant.product_forward`).
    constexpr int64_t kFqChunk = 3072;
    int64_t chunk = kFqChunk;
    if ((n + chunk - 1) / chunk > 0x40000000ll) chunk = ((n + 0x3FFFFFFFll) / 0x40000000ll + 1023) / 1024 * 1024;
    if (chunk > 0xFFFFFC00ll) chunk = 0xFFFFFC00ll;
    const int64_t blocks = (n + chunk - 1) / chunk;
    if (blocks > 0x7FFFFFFFll) return bad("tensor too large");
#define DPL_FQ_LAUNCH(PRE)                                                                                                    \
    hipLaunchKernelGGL((k_fake_quant<PRE, FMT>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_x, d_x2, d_y, (uint64_t)n,   \
                       (uint64_t)chunk, d_scale, d_zp, (uint32_t)n_channels, (uint32_t)inner, (float)qlo, (float)qhi)
    if (pre == DPL_FQ_PRE_ADD_RELU) DPL_FQ_LAUNCH(kFqPreAddRelu);
    else if (pre == DPL_FQ_PRE_RELU) DPL_FQ_LAUNCH(kFqPreRelu);
    else DPL_FQ_LAUNCH(kFqPreNone);
#undef DPL_FQ_LAUNCH
    DPL_LAUNCH_CHECK("k_fake_quant");
    return 0;
}

}  // namespace

// =================================================================================== C ABI
extern "C" {

int dpl_abi_version(void) { return DPL_ABI_VERSION; }
const char* dpl_last_error(void) { return g_err; }

int dpl_device_info(char* name, int name_cap, int* compute_units, uint64_t* hbm_bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail("hipGetDevice", e);
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return fail("hipGetDeviceProperties", e);
    if (name && name_cap > 0) snprintf(name, name_cap, "%s (%s)", p.name, p.gcnArchName);
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return fail_msg("current HIP device is not gfx950");
    return 0;
}

int dpl_stream_priority_range(int* least, int* greatest) {
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e != hipSuccess) return fail("hipDeviceGetStreamPriorityRange", e);
    if (least) *least = lo;
    if (greatest) *greatest = hi;
    return 0;
}

int dpl_stream_create(int priority, dpl_stream_t* out) {
    if (!out) return fail_msg("dpl_stream_create: null out");
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);   // (lo: the numerically largest = least urgent)
    if (e != hipSuccess) return fail("hipDeviceGetStreamPriorityRange", e);
    if (priority > lo) priority = lo;
    if (priority < hi) priority = hi;
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (e != hipSuccess) return fail("hipStreamCreateWithPriority", e);
    *out = (dpl_stream_t)s;
    return 0;
}

int dpl_stream_destroy(dpl_stream_t s) {
    if (!s) return 0;
    hipError_t e = hipStreamDestroy((hipStream_t)s);
    return e == hipSuccess ? 0 : fail("hipStreamDestroy", e);
}

int dpl_minmax_init(uint32_t* d_min_enc, uint32_t* d_max_enc, uint32_t* d_nan, int64_t n_slots, dpl_stream_t s) {
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_minmax_init, dim3(grid_for(n_slots, 256)), dim3(256), 0, (hipStream_t)s, d_min_enc,
                       d_max_enc, d_nan, n_slots);
    DPL_LAUNCH_CHECK("k_minmax_init");
    return 0;
}

// n_blocks = number of workgroups; d_block_begin (n_blocks + 1 entries) may be null, then n_blocks must equal
// n_items and workgroup b processes item b.
int dpl_minmax_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                          int64_t n_blocks, const float* const* d_seg_ptrs, uint32_t* d_min_enc,
                          uint32_t* d_max_enc, uint32_t* d_nan, dpl_stream_t s) {
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_minmax_accumulate", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_minmax, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)s, d_items, d_block_begin,
                       d_seg_ptrs, d_min_enc, d_max_enc, d_nan);
    DPL_LAUNCH_CHECK("k_minmax");
    return 0;
}

int dpl_minmax_finalize(const uint32_t* d_min_enc, const uint32_t* d_max_enc, const uint32_t* d_nan,
                        int64_t n_slots, float* d_min, float* d_max, dpl_stream_t s) {
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_minmax_finalize, dim3(grid_for(n_slots, 256)), dim3(256), 0, (hipStream_t)s, d_min_enc,
                       d_max_enc, d_nan, n_slots, d_min, d_max);
    DPL_LAUNCH_CHECK("k_minmax_finalize");
    return 0;
}

int dpl_minmax_encode(const float* d_min, const float* d_max, int64_t n_slots, uint32_t* d_min_enc,
                      uint32_t* d_max_enc, uint32_t* d_nan, dpl_stream_t s) {
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_minmax_encode, dim3(grid_for(n_slots, 256)), dim3(256), 0, (hipStream_t)s, d_min, d_max,
                       n_slots, d_min_enc, d_max_enc, d_nan);
    DPL_LAUNCH_CHECK("k_minmax_encode");
    return 0;
}

int dpl_hist_prepare(const float* d_min, const float* d_max, int64_t n_slots, int bins, dpl_hist_range* d_ranges,
                     dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_hist_prepare: bins must be in [1, 16384]");
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_hist_prepare, dim3(grid_for(n_slots, 64)), dim3(64), 0, (hipStream_t)s, d_min, d_max,
                       n_slots, bins, d_ranges);
    DPL_LAUNCH_CHECK("k_hist_prepare");
    return 0;
}

int dpl_abs_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                            int64_t n_blocks, const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges,
                            int bins, uint64_t* d_hist, dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_abs_hist_accumulate: bins must be in [1, 16384]");
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_abs_hist_accumulate", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_abs_hist, dim3((unsigned)n_blocks), dim3(kBlock),
                       ((size_t)bins + 1 + kBlock / kWave) * sizeof(uint32_t), (hipStream_t)s, d_items, d_block_begin,
                       d_seg_ptrs, d_ranges, bins, d_hist);
    DPL_LAUNCH_CHECK("k_abs_hist");
    return 0;
}

uint64_t dpl_hist_spec_entry_bytes(int64_t n_slots, int bins) {
    if (n_slots < 0 || bins < 1 || bins > DPL_MAX_BINS) return 0;
    return spec_counts_offset(n_slots) + (uint64_t)n_slots * (uint64_t)bins * sizeof(uint32_t);
}

int dpl_minmax_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                               int64_t n_blocks, const float* const* d_seg_ptrs, uint32_t* d_min_enc, uint32_t* d_max_enc,
                               uint32_t* d_nan, int64_t n_slots, int bins, void* d_entry, dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_minmax_hist_accumulate: bins must be in [1, 16384]");
    if (!d_entry || ((uintptr_t)d_entry & 15u)) return fail_msg("dpl_minmax_hist_accumulate: d_entry must be 16-byte aligned");
    if (n_slots <= 0 || n_slots > 0x7FFFFFFFll) return fail_msg("dpl_minmax_hist_accumulate: n_slots out of range");
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_minmax_hist_accumulate", n_items, d_block_begin, n_blocks)) return e;
    dpl_hist_range* snap = (dpl_hist_range*)d_entry;
    uint32_t* flags = (uint32_t*)(snap + n_slots);
    uint32_t* counts = (uint32_t*)((char*)d_entry + spec_counts_offset(n_slots));
    int64_t zb = grid_for(n_slots * (int64_t)bins, kBlock * 8);
    if (zb < grid_for(n_slots, kBlock)) zb = grid_for(n_slots, kBlock);
    if (zb > 1024) zb = 1024;
    hipLaunchKernelGGL(k_hist_snapshot, dim3((unsigned)zb), dim3(kBlock), 0, (hipStream_t)s, d_min_enc, d_max_enc, d_nan,
                       n_slots, bins, snap, flags, counts);
    DPL_LAUNCH_CHECK("k_hist_snapshot");
    hipLaunchKernelGGL(k_minmax_hist, dim3((unsigned)n_blocks), dim3(kBlock),
                       ((size_t)bins + 1 + 4 * (kBlock / kWave)) * sizeof(uint32_t), (hipStream_t)s, d_items, d_block_begin,
                       d_seg_ptrs, d_min_enc, d_max_enc, d_nan, snap, bins, counts);
    DPL_LAUNCH_CHECK("k_minmax_hist");
    return 0;
}

int dpl_hist_spec_accumulate(void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks,
                             const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges, int bins, uint64_t* d_hist,
                             uint64_t* d_stats, dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_hist_spec_accumulate: bins must be in [1, 16384]");
    if (!d_entry || ((uintptr_t)d_entry & 15u)) return fail_msg("dpl_hist_spec_accumulate: d_entry must be 16-byte aligned");
    if (n_slots <= 0 || n_slots > DPL_HIST_SPEC_MAX_TENSORS)
        return fail_msg("dpl_hist_spec_accumulate: n_slots must be in [1, DPL_HIST_SPEC_MAX_TENSORS]");
    if (n_blocks <= 0 || n_blocks > 0x7FFFFFFFll) return fail_msg("dpl_hist_spec_accumulate: n_blocks out of range");
    dpl_hist_range* snap = (dpl_hist_range*)d_entry;
    uint32_t* flags = (uint32_t*)(snap + n_slots);
    const uint32_t* counts = (const uint32_t*)((char*)d_entry + spec_counts_offset(n_slots));
    hipLaunchKernelGGL(k_hist_resolve, dim3((unsigned)n_slots), dim3(kBlock), 0, (hipStream_t)s, snap, d_ranges, counts, d_elems,
                       bins, d_hist, flags, (unsigned long long*)d_stats);
    DPL_LAUNCH_CHECK("k_hist_resolve");
    const size_t lds = ((size_t)n_slots + 1 + kBlock / kWave) * sizeof(uint64_t) + ((size_t)bins + 1 + kBlock / kWave) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_abs_hist_rest, dim3((unsigned)n_blocks), dim3(kBlock), lds, (hipStream_t)s, d_elems, flags, (int)n_slots,
                       d_seg_ptrs, d_ranges, bins, d_hist);
    DPL_LAUNCH_CHECK("k_abs_hist_rest");
    return 0;
}

int dpl_hist_spec_cuts(const void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks, uint64_t* d_cuts,
                       dpl_stream_t s) {
    if (!d_entry || !d_cuts) return fail_msg("dpl_hist_spec_cuts: null argument");
    if (n_slots <= 0 || n_slots > DPL_HIST_SPEC_MAX_TENSORS)
        return fail_msg("dpl_hist_spec_cuts: n_slots must be in [1, DPL_HIST_SPEC_MAX_TENSORS]");
    if (n_blocks <= 0 || n_blocks > 0x7FFFFFFFll) return fail_msg("dpl_hist_spec_cuts: n_blocks out of range");
    const uint32_t* flags = (const uint32_t*)((const dpl_hist_range*)d_entry + n_slots);
    hipLaunchKernelGGL(k_hist_spec_cuts, dim3((unsigned)n_blocks), dim3(kBlock),
                       ((size_t)n_slots + 1 + kBlock / kWave) * sizeof(uint64_t), (hipStream_t)s, d_elems, flags, (int)n_slots, d_cuts);
    DPL_LAUNCH_CHECK("k_hist_spec_cuts");
    return 0;
}

int dpl_hist_percentile(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins,
                        double threshold, float* d_clip, dpl_stream_t s) {
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_hist_percentile, dim3((unsigned)n_slots), dim3(kWave), 0, (hipStream_t)s, d_hist, d_min,
                       d_max, bins, threshold, d_clip);
    DPL_LAUNCH_CHECK("k_hist_percentile");
    return 0;
}

int dpl_hist_kl(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins, int levels,
                double* d_div, int32_t* d_best, float* d_clip, dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_hist_kl: bins must be in [1, 16384]");
    if (levels < 2 || levels > bins) return fail_msg("dpl_hist_kl: levels must be in [2, bins]");
    if (n_slots <= 0) return 0;
    // candidate chunks per tensor: about 1024 workgroups per launch, and no fewer than eight candidates per workgroup
    const int64_t n_cand = (int64_t)bins - levels + 1;
    int64_t chunks = (1024 + n_slots - 1) / n_slots;
    if (chunks > n_cand / 8) chunks = n_cand / 8;
    if (chunks < 1) chunks = 1;
    if (n_slots * chunks > 0x7FFFFFFFll) return fail_msg("dpl_hist_kl: too many slots");
    const size_t nblk = ((size_t)bins + 63) / 64;
    const size_t lds = ((size_t)bins + 1 + nblk + 1 + kBlock) * sizeof(uint64_t) + (nblk + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_hist_kl, dim3((unsigned)(n_slots * chunks)), dim3(kBlock), lds, (hipStream_t)s, d_hist, bins, levels,
                       (int)chunks, d_div);
    DPL_LAUNCH_CHECK("k_hist_kl");
    hipLaunchKernelGGL(k_hist_kl_pick, dim3((unsigned)n_slots), dim3(kWave), 0, (hipStream_t)s, d_div, d_min, d_max, bins,
                       d_best, d_clip);
    DPL_LAUNCH_CHECK("k_hist_kl_pick");
    return 0;
}

int dpl_hist_qmse(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins, int first, int grid,
                  int top, double* d_err, int32_t* d_best, float* d_clip, dpl_stream_t s) {
    if (bins < 1 || bins > DPL_MAX_BINS) return fail_msg("dpl_hist_qmse: bins must be in [1, 16384]");
    if (first < 1 || first > bins) return fail_msg("dpl_hist_qmse: first must be in [1, bins]");
    if (grid != DPL_GRID_UNIFORM && grid != DPL_GRID_E4M3) return fail_msg("dpl_hist_qmse: grid must be DPL_GRID_UNIFORM or DPL_GRID_E4M3");
    if (grid == DPL_GRID_UNIFORM && (top < 1 || top > 32767)) return fail_msg("dpl_hist_qmse: top must be in [1, 32767] on the uniform grid");
    if (grid == DPL_GRID_E4M3 && top != 0) return fail_msg("dpl_hist_qmse: top must be 0 on the E4M3 grid (its largest value is 448)");
    if (n_slots <= 0) return 0;
    // candidate chunks per tensor: about 1024 workgroups per launch, and no fewer than eight candidates per workgroup
    const int64_t n_cand = (int64_t)bins - first + 1;
    int64_t chunks = (1024 + n_slots - 1) / n_slots;
    if (chunks > n_cand / 8) chunks = n_cand / 8;
    if (chunks < 1) chunks = 1;
    if (n_slots * chunks > 0x7FFFFFFFll) return fail_msg("dpl_hist_qmse: too many slots");
    const size_t lds = (size_t)bins * sizeof(double) + (kBlock / kWave) * sizeof(uint64_t);
    const dim3 wgs((unsigned)(n_slots * chunks));
    if (grid == DPL_GRID_E4M3)
        hipLaunchKernelGGL(k_hist_qmse<kGridE4M3>, wgs, dim3(kBlock), lds, (hipStream_t)s, d_hist, bins, first, top, (int)chunks, d_err);
    else
        hipLaunchKernelGGL(k_hist_qmse<kGridUniform>, wgs, dim3(kBlock), lds, (hipStream_t)s, d_hist, bins, first, top, (int)chunks, d_err);
    DPL_LAUNCH_CHECK("k_hist_qmse");
    hipLaunchKernelGGL(k_hist_kl_pick, dim3((unsigned)n_slots), dim3(kWave), 0, (hipStream_t)s, d_err, d_min, d_max, bins,
                       d_best, d_clip);
    DPL_LAUNCH_CHECK("k_hist_kl_pick");
    return 0;
}

int dpl_rowwise_minmax(const float* d_w, int64_t rows, int64_t cols, float* d_min, float* d_max, dpl_stream_t s) {
    if (rows <= 0) return 0;
    if (cols <= 0 || cols > 0xFFFFFFFFll) return fail_msg("dpl_rowwise_minmax: cols out of range");
    hipLaunchKernelGGL(k_rowwise_minmax, dim3((unsigned)rows), dim3(kBlock), 0, (hipStream_t)s, d_w, cols, d_min,
                       d_max);
    DPL_LAUNCH_CHECK("k_rowwise_minmax");
    return 0;
}

int dpl_colwise_absmax(const float* d_x, int64_t rows, int64_t cols, float* d_acc, dpl_stream_t s) {
    if (rows < 0 || cols < 1) return fail_msg("dpl_colwise_absmax: rows must be >= 0 and cols >= 1");
    if (rows == 0) return 0;
    if (!d_x || !d_acc) return fail_msg("dpl_colwise_absmax: null pointer");
    if (rows > INT64_MAX / cols) return fail_msg("dpl_colwise_absmax: rows * cols overflows 64 bits");
    const bool vec = (cols % 4 == 0) && (((uintptr_t)d_x & 15u) == 0);     // every row then starts on 16 bytes
    const uint64_t cv = (uint64_t)(vec ? cols / 4 : cols);
    uint32_t tw = 1;
    while (tw < (uint32_t)kColMaxLanes && tw < cv) tw <<= 1;
    const uint64_t gx = (cv + tw - 1) / tw;
    if (gx > 0x7FFFFFFFull) return fail_msg("dpl_colwise_absmax: cols out of range");
    // rows: every workgroup makes the same number of trips (kColUnroll * 256 / tw rows each), at most kColMaxBlocks workgroups
    const uint64_t per_trip = (uint64_t)kColUnroll * (kBlock / tw);
    const uint64_t trips = ((uint64_t)rows + per_trip - 1) / per_trip;
    const uint64_t cap = gx >= (uint64_t)kColMaxBlocks ? 1 : (uint64_t)kColMaxBlocks / gx;
    const uint64_t passes = (trips + cap - 1) / cap;
    const dim3 g((unsigned)gx, (unsigned)((trips + passes - 1) / passes)), b(kBlock);
    uint32_t* acc = reinterpret_cast<uint32_t*>(d_acc);
    if (vec)
        hipLaunchKernelGGL(k_colwise_absmax<u4>, g, b, 0, (hipStream_t)s, reinterpret_cast<const u4*>(d_x), (uint64_t)rows, cv, tw, acc);
    else
        hipLaunchKernelGGL(k_colwise_absmax<uint32_t>, g, b, 0, (hipStream_t)s, reinterpret_cast<const uint32_t*>(d_x), (uint64_t)rows, cv,
                           tw, acc);
    DPL_LAUNCH_CHECK("k_colwise_absmax");
    return 0;
}

int dpl_fake_quant(const float* d_x, float* d_y, int64_t n, const float* d_scale, const int32_t* d_zp,
                   int64_t n_channels, int64_t inner, int32_t qlo, int32_t qhi, dpl_stream_t s) {
    return dpl_fake_quant_pre(DPL_FQ_PRE_NONE, d_x, nullptr, d_y, n, d_scale, d_zp, n_channels, inner, qlo, qhi, s);
}

int dpl_fake_quant_pre(int32_t pre, const float* d_x, const float* d_x2, float* d_y, int64_t n, const float* d_scale,
                       const int32_t* d_zp, int64_t n_channels, int64_t inner, int32_t qlo, int32_t qhi, dpl_stream_t s) {
    return fake_quant_launch<kFqFmtInt>("dpl_fake_quant_pre", pre, d_x, d_x2, d_y, n, d_scale, d_zp, n_channels, inner, qlo, qhi, s);
}

int dpl_fake_quant_fp8(int32_t pre, const float* d_x, const float* d_x2, float* d_y, int64_t n, const float* d_scale,
                       int64_t n_channels, int64_t inner, dpl_stream_t s) {
    return fake_quant_launch<kFqFmtE4M3>("dpl_fake_quant_fp8", pre, d_x, d_x2, d_y, n, d_scale, nullptr, n_channels, inner, 0, 0, s);
}

int dpl_fake_quant_items(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                         const float* const* d_seg_x, float* const* d_seg_y, const dpl_fake_quant_params* d_params, dpl_stream_t s) {
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_fake_quant_items", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_fake_quant_items<kFqFmtInt>, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)s, d_items, d_block_begin,
                       d_seg_x, d_seg_y, d_params);
    DPL_LAUNCH_CHECK("k_fake_quant_items");
    return 0;
}

int dpl_fake_quant_fp8_items(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin, int64_t n_blocks,
                             const float* const* d_seg_x, float* const* d_seg_y, const dpl_fake_quant_params* d_params, dpl_stream_t s) {
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_fake_quant_fp8_items", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_fake_quant_items<kFqFmtE4M3>, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)s, d_items, d_block_begin,
                       d_seg_x, d_seg_y, d_params);
    DPL_LAUNCH_CHECK("k_fake_quant_fp8_items");
    return 0;
}

int dpl_cos_accumulate(const float* d_a, const float* d_b, int64_t n, double* d_acc, int64_t slot, dpl_stream_t s) {
    if (n <= 0) return 0;
    if (((uintptr_t)d_a | (uintptr_t)d_b) & 15u) return fail_msg("dpl_cos_accumulate: buffers must be 16-B aligned");
    int64_t blocks = (n / 4 + kBlock * 8 - 1) / (kBlock * 8);
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_cos_acc, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_a, d_b, n,
                       d_acc + 3 * slot);
    DPL_LAUNCH_CHECK("k_cos_acc");
    return 0;
}

int dpl_channel_diff_sum(const float* d_a, const float* d_b, int64_t outer, int64_t n_channels, int64_t inner,
                         double* d_acc, dpl_stream_t s) {
    if (outer <= 0 || n_channels <= 0 || inner <= 0) return 0;
    if (n_channels > 0xFFFFFFFFll || inner > 0xFFFFFFFFll) return fail_msg("dpl_channel_diff_sum: extent out of range");
    const uint64_t rows = (uint64_t)outer * (uint64_t)n_channels;
    const int vec_ok = ((inner & 3) == 0) && ((((uintptr_t)d_a | (uintptr_t)d_b) & 15u) == 0);
    uint64_t work = inner == 1 ? (uint64_t)(n_channels + kWave - 1) / kWave : rows;
    uint64_t blocks = (work + kBlock / kWave - 1) / (kBlock / kWave);
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_channel_diff_sum, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)s, d_a, d_b, rows,
                       (uint32_t)n_channels, (uint32_t)inner, vec_ok, d_acc);
    DPL_LAUNCH_CHECK("k_channel_diff_sum");
    return 0;
}

int dpl_cos_items_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                             int64_t n_blocks, const float* const* d_seg_a, const float* const* d_seg_b,
                             double* d_acc, dpl_stream_t s) {
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_cos_items_accumulate", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_cos_items, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)s, d_items,
                       d_block_begin, d_seg_a, d_seg_b, d_acc);
    DPL_LAUNCH_CHECK("k_cos_items");
    return 0;
}

}  // extern "C"
