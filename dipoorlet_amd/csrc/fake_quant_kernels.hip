// K6: the fused quantize -> dequantize pair (Q/DQ) and its C ABI — an integer grid or OCP FP8 E4M3, one tensor or a whole tensor
// set per launch, the producer's ReLU / Add + ReLU applied on the way in.  HBM-bound: one read and one write per element.
// (The Microscaling formats are in mx_kernels.hip.)
#include "common.hpp"
#include "fq_elem.hpp"

namespace {

// ================================================================ K6: fused quantize -> dequantize
// (the element quantisers — fq_one, e4m3_round, fq_elem<FMT> — are in fq_elem.hpp, shared with gptq_kernels.hip)

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

extern "C" {

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

}  // extern "C"
