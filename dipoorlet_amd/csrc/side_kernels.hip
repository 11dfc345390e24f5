// The statistics beside the calibration chain, and their C ABI: per-row min / max and per-column running max |x| of a matrix
// (K5, K5b: weight ranges, --smooth), the cosine sums (N1, k_cos_items: profiling) and the per-channel sum of differences
// (N2: bias correction).  All HBM-bound streaming reductions.
#include "common.hpp"

namespace {

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

}  // namespace

extern "C" {

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
