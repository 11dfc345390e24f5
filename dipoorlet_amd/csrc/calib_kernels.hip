// MI355X (gfx950 / CDNA4) activation-calibration kernels + their C ABI (include/dipoorlet_hip.h): the statistics chain — running
// min / max (K1), the |x| histogram and its range-pass speculation (K2, K2s), the clip searches on it (K4, K4b, K4c).  The Q/DQ
// pair is in fake_quant_kernels.hip, the row / column / cosine / bias-correction sums in side_kernels.hip, the ABI's version,
// error text, device info and streams in runtime_abi.hip.
//
// Everything here but the two searches K4b / K4c (fp64 arithmetic on an LDS-resident row) is an HBM-bound streaming
// reduction / scatter-add: no MFMA.  A kernel's dynamic-LDS layout is defined ONCE, in a struct of offset functions beside it:
// the kernel takes its region pointers from it, the launcher its byte count.  Design rules
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

// ================================================================ K1: running min / max  (MinMaxOp: common.hpp)
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

// LDS of a histogramming workgroup:  uint32 counters[bins + 1] | uint32 s_nz[waves]
// (counter `bins`: HistOp's estimates of `bins`; s_nz: hist_flush's non-zero count per wave).  k_abs_hist's whole dynamic LDS,
// the tail of k_hist_spec's (RestLds) and the head of k_minmax_hist's (MinMaxHistLds).
struct HistLds {
    static __host__ __device__ uint32_t* s_nz(uint32_t* counters, int bins) { return counters + bins + 1; }
    static __host__ __device__ uint32_t* end(uint32_t* counters, int bins) { return s_nz(counters, bins) + kBlock / kWave; }
    static __host__ __device__ constexpr size_t bytes(int bins) { return ((size_t)bins + 1 + kBlock / kWave) * sizeof(uint32_t); }
};

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
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // HistLds
    uint32_t* s_nz = HistLds::s_nz(lds, bins);
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
// k_hist_spec).
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
// byte, adds the rows that match and reads only the tensors whose guess was wrong (k_hist_spec: one launch).  A wrong
// guess costs what it always cost, so no count can change.
//
// A ledger entry (device memory, 16-byte aligned; the documented format: callers read the flags at n_slots * sizeof(dpl_hist_range)):
//   dpl_hist_range snap[n_slots] | uint32 flags[n_slots] | pad to 16 bytes | uint32 counts[n_slots, bins]
struct SpecEntry {
    dpl_hist_range* snap;
    uint32_t* flags;
    uint32_t* counts;
    SpecEntry(const void* d_entry, int64_t n_slots)   // (const: dpl_hist_spec_cuts only reads the flags)
        : snap((dpl_hist_range*)d_entry), flags((uint32_t*)(snap + n_slots)), counts((uint32_t*)((char*)d_entry + counts_offset(n_slots))) {}
    static uint64_t counts_offset(int64_t n_slots) {
        return (((uint64_t)n_slots * (sizeof(dpl_hist_range) + sizeof(uint32_t))) + 15ull) & ~15ull;
    }
    static uint64_t bytes(int64_t n_slots, int bins) { return counts_offset(n_slots) + (uint64_t)n_slots * (uint64_t)bins * sizeof(uint32_t); }
};

// Snapshot of the provisional ranges + the entry's counts zeroed.  A slot with no data yet, a NaN flag or a range numpy would
// refuse comes out with status != 0 ("no guess": the fused kernel takes its min / max only and k_hist_spec never accepts it).
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

// LDS of k_minmax_hist:  HistLds | float s_mn[waves] | float s_mx[waves] | uint32 s_nan[waves]   (minmax_commit's words)
struct MinMaxHistLds {
    static __host__ __device__ float* s_mn(uint32_t* base, int bins) { return reinterpret_cast<float*>(HistLds::end(base, bins)); }
    static __host__ __device__ float* s_mx(uint32_t* base, int bins) { return s_mn(base, bins) + kBlock / kWave; }
    static __host__ __device__ uint32_t* s_nan(uint32_t* base, int bins) {
        return reinterpret_cast<uint32_t*>(s_mx(base, bins) + kBlock / kWave);
    }
    static __host__ __device__ size_t bytes(int bins) { return HistLds::bytes(bins) + 3 * (kBlock / kWave) * sizeof(uint32_t); }
};

// k_minmax and k_abs_hist in one read: min / max / NaN into the accumulators as k_minmax does, counts against snap[slot] into the
// ledger entry as k_abs_hist does (same HistOp, same flush).
__global__ __launch_bounds__(kBlock) void k_minmax_hist(const dpl_work_item* __restrict__ items,
                                                         const uint32_t* __restrict__ bb,
                                                         const float* const* __restrict__ segs,
                                                         uint32_t* __restrict__ min_enc, uint32_t* __restrict__ max_enc,
                                                         uint32_t* __restrict__ nan_flag,
                                                         const dpl_hist_range* __restrict__ snap, int bins,
                                                         uint32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_mh[];  // MinMaxHistLds
    uint32_t* s_nz = HistLds::s_nz(lds_mh, bins);
    float* s_mn = MinMaxHistLds::s_mn(lds_mh, bins);
    float* s_mx = MinMaxHistLds::s_mx(lds_mh, bins);
    uint32_t* s_nan = MinMaxHistLds::s_nan(lds_mh, bins);
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

// What the histogram pass does with tensor t, the value of flags[t]: 1 = the entry's row is this batch's histogram and is added
// (the guess was right: the snapshot equals the final range in all 32 bytes — a sign-of-zero or NaN difference falls to the safe
// side — and numpy accepts the range); 2 = nothing to count (status != 0: k_abs_hist skips such a tensor too); 0 = to be read.
// A pure function of snap and fin, which no kernel writes during the histogram pass: every workgroup of k_hist_spec evaluates
// it for itself and gets the same answer.
struct SpecVerdict {
    const dpl_hist_range* __restrict__ snap;
    const dpl_hist_range* __restrict__ fin;
    __device__ __forceinline__ uint32_t operator()(int t) const {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(snap + t);
        const uint32_t* b = reinterpret_cast<const uint32_t*>(fin + t);
        bool same = true;
#pragma unroll
        for (int w = 0; w < (int)(sizeof(dpl_hist_range) / 4); ++w) same = same && (a[w] == b[w]);
        return fin[t].status != 0u ? 2u : (same ? 1u : 0u);
    }
};

// The verdicts the last histogram pass over the entry left in memory (the test hook k_hist_spec_cuts).
struct StoredVerdict {
    const uint32_t* __restrict__ flags;
    __device__ __forceinline__ uint32_t operator()(int t) const { return flags[t]; }
};

// rest_prefix's tally: a thread's share of {pairs added, elements, elements added} (k_hist_spec's statistics), or nothing.
struct SpecTally {
    unsigned long long n_add = 0, e_all = 0, e_add = 0;
    __device__ __forceinline__ void operator()(uint32_t f, uint64_t e) {
        e_all += e;
        n_add += f == 1u ? 1ull : 0ull;
        e_add += f == 1u ? e : 0ull;
    }
};
struct NoTally {
    __device__ __forceinline__ void operator()(uint32_t, uint64_t) {}
};

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d, kWave), hi = __shfl_up((uint32_t)(v >> 32), d, kWave);
    return ((uint64_t)hi << 32) | lo;
}

// k_abs_hist over the tensors whose verdict is 0, BALANCED: the remaining tensors' elements form one stream,
// workgroup b of G owns [cut(b), cut(b + 1)) of it, cut(b) = floor(total * b / G) rounded down to a multiple of 1024 elements
// from the start of the tensor it falls in — the cuts dpl_build_balanced_items makes, in closed form, so every workgroup derives
// its own share from the prefix sums (taken by each workgroup into LDS: T additions) with no list built and no host in between.
// Tensor t is segment t, slot t, offset 0 (the per-tensor spans of a TensorSetPlan); elems[t] < 2^32.
// (k_hist_spec below; rest_prefix and rest_cut are its two steps, shared with the test hook k_hist_spec_cuts.)
//
// Every tensor's verdict into v[0 .. n_tensors) and the exclusive prefix sums of the remaining tensors' element counts into
// P[0 .. n_tensors] (both LDS), by the whole workgroup.  A thread's loads (verdict's and elems') depend on nothing but t: one
// round trip.  (P[t] holds tensor t's remaining count between the two loops: a thread reads back only what it wrote itself.)
// tally(verdict, elements) sees every tensor once, spread over the workgroup's threads.
template <class Verdict, class Tally>
__device__ __forceinline__ void rest_prefix(const uint64_t* __restrict__ elems, const Verdict& verdict, int n_tensors,
                                            uint64_t* P, uint64_t* s_tot, uint32_t* v, Tally& tally) {
    const int per = (n_tensors + kBlock - 1) / kBlock;  // consecutive tensors per thread
    const int t0 = (int)threadIdx.x * per;
    uint64_t mine = 0;
    for (int j = 0; j < per; ++j) {
        const int t = t0 + j;
        if (t < n_tensors) {
            const uint32_t f = verdict(t);
            const uint64_t e = elems[t];
            const uint64_t rem = f == 0u ? e : 0ull;
            v[t] = f;
            P[t] = rem;
            mine += rem;
            tally(f, e);
        }
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
            const uint64_t rem = P[t];
            P[t] = run;
            run += rem;
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

// LDS of rest_prefix:  uint64 P[n_tensors + 1] | uint64 s_tot[3 * waves] | uint32 v[n_tensors]
// (the prefix sums; the scan's wave totals, afterwards the wave totals of k_hist_spec's three statistics; the verdicts).
// k_hist_spec_cuts's whole dynamic LDS and the head of k_hist_spec's (n_tensors <= DPL_HIST_SPEC_MAX_TENSORS: 24 KiB).
struct RestPrefixLds {
    static constexpr int kTotals = 3 * (kBlock / kWave);
    static __host__ __device__ uint64_t* P(uint32_t* base) { return reinterpret_cast<uint64_t*>(base); }
    static __host__ __device__ uint64_t* s_tot(uint32_t* base, int n_tensors) { return P(base) + n_tensors + 1; }
    static __host__ __device__ uint32_t* v(uint32_t* base, int n_tensors) {
        return reinterpret_cast<uint32_t*>(s_tot(base, n_tensors) + kTotals);
    }
    static __host__ __device__ uint32_t* end(uint32_t* base, int n_tensors) { return v(base, n_tensors) + n_tensors; }
    static __host__ __device__ constexpr size_t bytes(int64_t n_tensors) {
        return ((size_t)n_tensors + 1 + kTotals) * sizeof(uint64_t) + (size_t)n_tensors * sizeof(uint32_t);
    }
};

// LDS of k_hist_spec:  RestPrefixLds | HistLds
struct RestLds {
    static __host__ __device__ uint32_t* counters(uint32_t* base, int n_tensors) { return RestPrefixLds::end(base, n_tensors); }
    static __host__ __device__ constexpr size_t bytes(int64_t n_tensors, int bins) {
        return RestPrefixLds::bytes(n_tensors) + HistLds::bytes(bins);
    }
};
static_assert(RestLds::bytes(DPL_HIST_SPEC_MAX_TENSORS, DPL_MAX_BINS) <= 160 * 1024, "k_hist_spec's largest layout must fit a CU's LDS");

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

// The whole histogram-pass call over a bound set in ONE launch.  No workgroup waits for, or reads, anything another workgroup
// of the launch writes: each takes every tensor's verdict for itself (rest_prefix over SpecVerdict), so all agree on which rows
// are added and where the remaining stream is cut.
//   * Slot t has exactly one resolver, workgroup t mod G: it writes flags[t] and, where the verdict is 1, adds the entry's row
//     into hist[t, :].  Valid rows of hist are touched only by their resolver; invalid rows are touched only by the streaming
//     workgroups' atomics: the two sets are disjoint by construction.  The resolver adds with atomics that return nothing all
//     the same, as hist_flush does: they need no load of hist in front of them, so a resolver goes on to its share of the
//     stream at once.  The row of its first slot it requests BEFORE the verdicts (kAhead counts per thread, in flight beside
//     rest_prefix's loads: one round trip for both; unused where the verdict is not 1).
//   * Workgroup 0 adds the launch's totals to stats (may be null) += {pairs, pairs added, elements, elements added}: four
//     atomics per launch.
//   * Every workgroup then streams its share [cut(b), cut(b + 1)) of the tensors to be read, as k_abs_hist does.
// snap and counts are only read: an entry may be consumed by any number of histogram passes.
__global__ __launch_bounds__(kBlock) void k_hist_spec(const dpl_hist_range* __restrict__ snap, const uint32_t* __restrict__ counts,
                                                       uint32_t* __restrict__ flags, const uint64_t* __restrict__ elems,
                                                       int n_tensors, const float* const* __restrict__ segs,
                                                       const dpl_hist_range* __restrict__ ranges, int bins,
                                                       uint64_t* __restrict__ hist, unsigned long long* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_rest[];  // RestLds
    uint64_t* P = RestPrefixLds::P(lds_rest);
    uint64_t* s_tot = RestPrefixLds::s_tot(lds_rest, n_tensors);
    uint32_t* v = RestPrefixLds::v(lds_rest, n_tensors);
    uint32_t* lds = RestLds::counters(lds_rest, n_tensors);
    uint32_t* s_nz = HistLds::s_nz(lds, bins);
    constexpr int kAhead = 8;  // (2048 bins: the whole row)
    uint32_t ahead[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
        const int j = (int)threadIdx.x + u * kBlock;
        ahead[u] = (blockIdx.x < (uint32_t)n_tensors && j < bins) ? counts[(uint64_t)blockIdx.x * (uint64_t)bins + j] : 0u;
    }
    SpecTally tally;
    rest_prefix(elems, SpecVerdict{snap, ranges}, n_tensors, P, s_tot, v, tally);
    for (uint32_t t = blockIdx.x; t < (uint32_t)n_tensors; t += gridDim.x) {  // (no barrier inside: the trip count differs between workgroups only)
        const uint32_t f = v[t];
        if (threadIdx.x == 0) flags[t] = f;
        if (f != 1u) continue;
        const uint32_t* __restrict__ row = counts + (uint64_t)t * (uint64_t)bins;
        unsigned long long* __restrict__ out = reinterpret_cast<unsigned long long*>(hist + (uint64_t)t * (uint64_t)bins);
        int j = threadIdx.x;
        if (t == blockIdx.x) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
                if (ahead[u]) atomicAdd(out + j + u * kBlock, (unsigned long long)ahead[u]);  // (ahead[u] == 0 beyond the row)
            j += kAhead * kBlock;
        }
        for (; j < bins; j += kBlock) {
            const uint32_t c = row[j];
            if (c) atomicAdd(out + j, (unsigned long long)c);
        }
    }
    if (blockIdx.x == 0 && stats) {  // (uniform over the workgroup, as is the barrier inside)
        unsigned long long n_add = wave_sum_u64(tally.n_add), e_all = wave_sum_u64(tally.e_all), e_add = wave_sum_u64(tally.e_add);
        constexpr int kWaves = kBlock / kWave;
        if ((threadIdx.x & (kWave - 1)) == 0) {  // (s_tot is free: rest_prefix ended in a barrier)
            const int wv = threadIdx.x / kWave;
            s_tot[wv] = n_add;
            s_tot[kWaves + wv] = e_all;
            s_tot[2 * kWaves + wv] = e_add;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            n_add = e_all = e_add = 0;
            for (int w = 0; w < kWaves; ++w) {
                n_add += s_tot[w];
                e_all += s_tot[kWaves + w];
                e_add += s_tot[2 * kWaves + w];
            }
            atomicAdd(stats + 0, (unsigned long long)n_tensors);
            atomicAdd(stats + 1, n_add);
            atomicAdd(stats + 2, e_all);
            atomicAdd(stats + 3, e_add);
        }
    }
    if (P[n_tensors] == 0) return;  // (uniform; nothing to read: the steady state of a sweep over few distinct sets)
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
        const dpl_hist_range r = ranges[t];  // (status == 0 and a wrong guess: every other tensor adds nothing to P)
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

// The cuts k_hist_spec works to for the verdicts it left in flags, written out (dpl_hist_spec_cuts: what tests hold against
// tests/hist_spec_model.py).  flags[t] is SpecVerdict's value, so these are the cuts that launch worked to.
__global__ __launch_bounds__(kBlock) void k_hist_spec_cuts(const uint64_t* __restrict__ elems, const uint32_t* __restrict__ flags,
                                                            int n_tensors, uint64_t* __restrict__ cuts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cuts[];  // RestPrefixLds
    uint64_t* P = RestPrefixLds::P(lds_cuts);
    NoTally none;
    rest_prefix(elems, StoredVerdict{flags}, n_tensors, P, RestPrefixLds::s_tot(lds_cuts, n_tensors), RestPrefixLds::v(lds_cuts, n_tensors), none);
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

// LDS of k_hist_kl, nblk = ceil(bins / 64):
//   uint64 cs[bins + 1]    exclusive prefix sum of the counts
//   uint64 mask[nblk + 1]  bit b & 63 of mask[b >> 6]: count of bin b != 0 (the last entry is 0)
//   uint64 part[kBlock]    the scan's per-thread sums
//   uint32 bcnt[nblk + 1]  non-zero bins below bin 64 k
struct KlLds {
    static __host__ __device__ uint32_t nblk(int bins) { return ((uint32_t)bins + 63u) >> 6; }
    static __host__ __device__ uint64_t* mask(uint64_t* cs, int bins) { return cs + bins + 1; }
    static __host__ __device__ uint64_t* part(uint64_t* cs, int bins) { return mask(cs, bins) + nblk(bins) + 1; }
    static __host__ __device__ uint32_t* bcnt(uint64_t* cs, int bins) { return reinterpret_cast<uint32_t*>(part(cs, bins) + kBlock); }
    static __host__ __device__ size_t bytes(int bins) {
        return ((size_t)bins + 1 + nblk(bins) + 1 + kBlock) * sizeof(uint64_t) + ((size_t)nblk(bins) + 1) * sizeof(uint32_t);
    }
};

__global__ __launch_bounds__(kBlock) void k_hist_kl(const uint64_t* __restrict__ hist, int bins, int levels, int n_chunks,
                                                     double* __restrict__ div) {
    extern __shared__ __attribute__((aligned(16))) uint64_t kl_lds[];  // KlLds
    const uint32_t nblk = KlLds::nblk(bins);
    uint64_t* cs = kl_lds;
    uint64_t* mask = KlLds::mask(kl_lds, bins);
    uint64_t* part = KlLds::part(kl_lds, bins);
    uint32_t* bcnt = KlLds::bcnt(kl_lds, bins);
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

// LDS of k_hist_qmse:  double hd[bins] | uint64 part[waves]   (the counts; the waves' totals)
struct QmseLds {
    static __host__ __device__ uint64_t* part(double* hd, int bins) { return reinterpret_cast<uint64_t*>(hd + bins); }
    static __host__ __device__ size_t bytes(int bins) { return (size_t)bins * sizeof(double) + (kBlock / kWave) * sizeof(uint64_t); }
};

template <int GRID>
__global__ __launch_bounds__(kBlock) void k_hist_qmse(const uint64_t* __restrict__ hist, int bins, int first, int top, int n_chunks,
                                                       double* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double qm_lds[];  // QmseLds
    double* hd = qm_lds;
    uint64_t* part = QmseLds::part(qm_lds, bins);
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

// ================================================================ what the entry points below check alike (as check_blocks)
inline int check_bins(const char* who, int bins) {
    if (bins < 1 || bins > DPL_MAX_BINS) {
        snprintf(g_err, sizeof(g_err), "%s: bins must be in [1, %d]", who, DPL_MAX_BINS);
        return -2;
    }
    return 0;
}

// dpl_hist_spec_accumulate / dpl_hist_spec_cuts: P[n_slots + 1] must fit k_hist_spec's LDS, n_blocks a grid
inline int check_spec_geometry(const char* who, int64_t n_slots, int64_t n_blocks) {
    const bool slots_ok = n_slots > 0 && n_slots <= DPL_HIST_SPEC_MAX_TENSORS;
    if (slots_ok && n_blocks > 0 && n_blocks <= 0x7FFFFFFFll) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", who, slots_ok ? "n_blocks out of range" : "n_slots must be in [1, DPL_HIST_SPEC_MAX_TENSORS]");
    return -2;
}

// Candidate chunks per tensor of a clip search (k_hist_kl, k_hist_qmse): about 1024 workgroups per launch, and no fewer than
// eight candidates per workgroup.
inline int candidate_chunks(const char* who, int64_t n_slots, int64_t n_cand, int64_t& chunks) {
    chunks = (1024 + n_slots - 1) / n_slots;
    if (chunks > n_cand / 8) chunks = n_cand / 8;
    if (chunks < 1) chunks = 1;
    if (n_slots * chunks > 0x7FFFFFFFll) {
        snprintf(g_err, sizeof(g_err), "%s: too many slots", who);
        return -2;
    }
    return 0;
}

}  // namespace

// =================================================================================== C ABI
extern "C" {

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
    if (int e = check_bins("dpl_hist_prepare", bins)) return e;
    if (n_slots <= 0) return 0;
    hipLaunchKernelGGL(k_hist_prepare, dim3(grid_for(n_slots, 64)), dim3(64), 0, (hipStream_t)s, d_min, d_max,
                       n_slots, bins, d_ranges);
    DPL_LAUNCH_CHECK("k_hist_prepare");
    return 0;
}

int dpl_abs_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                            int64_t n_blocks, const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges,
                            int bins, uint64_t* d_hist, dpl_stream_t s) {
    if (int e = check_bins("dpl_abs_hist_accumulate", bins)) return e;
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_abs_hist_accumulate", n_items, d_block_begin, n_blocks)) return e;
    hipLaunchKernelGGL(k_abs_hist, dim3((unsigned)n_blocks), dim3(kBlock), HistLds::bytes(bins), (hipStream_t)s, d_items,
                       d_block_begin, d_seg_ptrs, d_ranges, bins, d_hist);
    DPL_LAUNCH_CHECK("k_abs_hist");
    return 0;
}

uint64_t dpl_hist_spec_entry_bytes(int64_t n_slots, int bins) {
    if (n_slots < 0 || bins < 1 || bins > DPL_MAX_BINS) return 0;
    return SpecEntry::bytes(n_slots, bins);
}

int dpl_minmax_hist_accumulate(const dpl_work_item* d_items, int64_t n_items, const uint32_t* d_block_begin,
                               int64_t n_blocks, const float* const* d_seg_ptrs, uint32_t* d_min_enc, uint32_t* d_max_enc,
                               uint32_t* d_nan, int64_t n_slots, int bins, void* d_entry, dpl_stream_t s) {
    if (int e = check_bins("dpl_minmax_hist_accumulate", bins)) return e;
    if (!d_entry || ((uintptr_t)d_entry & 15u)) return fail_msg("dpl_minmax_hist_accumulate: d_entry must be 16-byte aligned");
    if (n_slots <= 0 || n_slots > 0x7FFFFFFFll) return fail_msg("dpl_minmax_hist_accumulate: n_slots out of range");
    if (n_items <= 0) return 0;
    if (int e = check_blocks("dpl_minmax_hist_accumulate", n_items, d_block_begin, n_blocks)) return e;
    const SpecEntry entry(d_entry, n_slots);
    int64_t zb = grid_for(n_slots * (int64_t)bins, kBlock * 8);
    if (zb < grid_for(n_slots, kBlock)) zb = grid_for(n_slots, kBlock);
    if (zb > 1024) zb = 1024;
    hipLaunchKernelGGL(k_hist_snapshot, dim3((unsigned)zb), dim3(kBlock), 0, (hipStream_t)s, d_min_enc, d_max_enc, d_nan,
                       n_slots, bins, entry.snap, entry.flags, entry.counts);
    DPL_LAUNCH_CHECK("k_hist_snapshot");
    hipLaunchKernelGGL(k_minmax_hist, dim3((unsigned)n_blocks), dim3(kBlock), MinMaxHistLds::bytes(bins), (hipStream_t)s, d_items,
                       d_block_begin, d_seg_ptrs, d_min_enc, d_max_enc, d_nan, entry.snap, bins, entry.counts);
    DPL_LAUNCH_CHECK("k_minmax_hist");
    return 0;
}

int dpl_hist_spec_accumulate(void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks,
                             const float* const* d_seg_ptrs, const dpl_hist_range* d_ranges, int bins, uint64_t* d_hist,
                             uint64_t* d_stats, dpl_stream_t s) {
    if (int e = check_bins("dpl_hist_spec_accumulate", bins)) return e;
    if (!d_entry || ((uintptr_t)d_entry & 15u)) return fail_msg("dpl_hist_spec_accumulate: d_entry must be 16-byte aligned");
    if (int e = check_spec_geometry("dpl_hist_spec_accumulate", n_slots, n_blocks)) return e;
    const SpecEntry entry(d_entry, n_slots);
    hipLaunchKernelGGL(k_hist_spec, dim3((unsigned)n_blocks), dim3(kBlock), RestLds::bytes(n_slots, bins), (hipStream_t)s, entry.snap,
                       entry.counts, entry.flags, d_elems, (int)n_slots, d_seg_ptrs, d_ranges, bins, d_hist, (unsigned long long*)d_stats);
    DPL_LAUNCH_CHECK("k_hist_spec");
    return 0;
}

int dpl_hist_spec_cuts(const void* d_entry, const uint64_t* d_elems, int64_t n_slots, int64_t n_blocks, uint64_t* d_cuts,
                       dpl_stream_t s) {
    if (!d_entry || !d_cuts) return fail_msg("dpl_hist_spec_cuts: null argument");
    if (int e = check_spec_geometry("dpl_hist_spec_cuts", n_slots, n_blocks)) return e;
    hipLaunchKernelGGL(k_hist_spec_cuts, dim3((unsigned)n_blocks), dim3(kBlock), RestPrefixLds::bytes(n_slots), (hipStream_t)s, d_elems,
                       SpecEntry(d_entry, n_slots).flags, (int)n_slots, d_cuts);
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
    if (int e = check_bins("dpl_hist_kl", bins)) return e;
    if (levels < 2 || levels > bins) return fail_msg("dpl_hist_kl: levels must be in [2, bins]");
    if (n_slots <= 0) return 0;
    int64_t chunks;
    if (int e = candidate_chunks("dpl_hist_kl", n_slots, (int64_t)bins - levels + 1, chunks)) return e;
    hipLaunchKernelGGL(k_hist_kl, dim3((unsigned)(n_slots * chunks)), dim3(kBlock), KlLds::bytes(bins), (hipStream_t)s, d_hist, bins,
                       levels, (int)chunks, d_div);
    DPL_LAUNCH_CHECK("k_hist_kl");
    hipLaunchKernelGGL(k_hist_kl_pick, dim3((unsigned)n_slots), dim3(kWave), 0, (hipStream_t)s, d_div, d_min, d_max, bins,
                       d_best, d_clip);
    DPL_LAUNCH_CHECK("k_hist_kl_pick");
    return 0;
}

int dpl_hist_qmse(const uint64_t* d_hist, const float* d_min, const float* d_max, int64_t n_slots, int bins, int first, int grid,
                  int top, double* d_err, int32_t* d_best, float* d_clip, dpl_stream_t s) {
    if (int e = check_bins("dpl_hist_qmse", bins)) return e;
    if (first < 1 || first > bins) return fail_msg("dpl_hist_qmse: first must be in [1, bins]");
    if (grid != DPL_GRID_UNIFORM && grid != DPL_GRID_E4M3) return fail_msg("dpl_hist_qmse: grid must be DPL_GRID_UNIFORM or DPL_GRID_E4M3");
    if (grid == DPL_GRID_UNIFORM && (top < 1 || top > 32767)) return fail_msg("dpl_hist_qmse: top must be in [1, 32767] on the uniform grid");
    if (grid == DPL_GRID_E4M3 && top != 0) return fail_msg("dpl_hist_qmse: top must be 0 on the E4M3 grid (its largest value is 448)");
    if (n_slots <= 0) return 0;
    int64_t chunks;
    if (int e = candidate_chunks("dpl_hist_qmse", n_slots, (int64_t)bins - first + 1, chunks)) return e;
    const size_t lds = QmseLds::bytes(bins);
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

}  // extern "C"
