// K14: GPTQ's layer Hessian on the device (--gptq_hessian device): H[i][j] += sum over r of X[r][i] X[r][j] for an fp64
// [K, K] matrix, X [rows, K] fp32 never materialised.  An fp64 SYRK: the products of two fp32 values are exact in fp64, so only the
// additions round, and they are made in one fixed order.
//
//   k_gh_tile<G>   workgroup (t, s): the 64 x 64 tile t = (i, j <= i) of X^T X over the rows of range s.  The tile body is the
//                  factorisation's (gptq_f64_tile.hpp): four waves in 2 x 2, each 2 x 2 v_mfma_f64_16x16x4_f64 accumulators.  The
//                  two column panels i and j of X are gathered 32 rows at a time, converted to double on the way into LDS as
//                  [32][64 + 16]; a tile on the diagonal stages one panel and reads it for both operands.  Columns >= K and rows
//                  beyond the range are staged as exact zeros: the inner loop tests no bound.  The gather of pass p + 1 is issued
//                  before the matrix instructions of pass p, into registers.  One range (S == 1): the tile is added onto H, the
//                  mirror H[j][i] written with the same value.  S > 1: the tile is stored whole into the workspace.
//   k_gh_reduce    S > 1: workgroup t adds the S partials of every element of tile t, in ascending s, onto the value in H, and
//                  writes the element and its mirror.
//
// G says how element (r, c) of X is addressed, and lays the staging threads along what is contiguous in memory:
//   GhDense   x[r * K + c].  Thread t: column t & 63, rows (t >> 6) + 4 u: a wave reads 256 contiguous bytes and writes 64
//             consecutive doubles of a staged row.
//   GhConv    x [B, C, H, W]; r = (b, oy, ox), c = (ci, ky, kx).  Consecutive ox are adjacent in memory (stride sx), so thread t
//             takes row t & 31 and the eight columns 8 (t >> 5) + u: a half-wave reads one (ci, ky, kx) of 32 consecutive output
//             positions.  The (ci, ky, kx) of a thread's columns are decomposed once, before the row loop (an element offset and
//             the window's reach, 16 + 16 bits); a pass decomposes its one row.  Lanes along rows would all write one column of
//             the staged panel, 16 lanes to a bank; each lane therefore rotates its eight values by (row >> 1) & 7 first (three
//             select stages, no indexed register), which spreads a half-wave's write over 16 of the 32 bank pairs.
//
// The summation order of an element: within a range, ascending rows, four at a time through the instruction's own chain; then the
// ranges in ascending s onto H.  Ranges and S come from (rows, K) alone (gptq_hessian_plan.hpp), nothing is atomic: the same call
// gives the same bits, on every rank.
#include "gptq_f64_tile.hpp"
#include "gptq_hessian_plan.hpp"

namespace {

constexpr int kGhVals = kGhPass * kGfB / kBlock;       // values a thread stages per panel and pass: 8
static_assert(kGhPass == kGfKc && kGhVals == 8, "the staging maps below are written for 32 x 64 panels and 256 threads");

struct GhDense {
    const float* __restrict__ x;
    uint32_t k;
    struct Cols {
        uint32_t c;      // the thread's column of X (>= k: none)
    };
    __device__ __forceinline__ void cols(uint32_t c0, Cols& q) const { q.c = c0 + (threadIdx.x & 63); }
    __device__ __forceinline__ void load(const Cols& q, uint32_t r0, uint32_t r_end, float (&v)[kGhVals]) const {
        const uint32_t r = r0 + (threadIdx.x >> 6);
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) v[u] = (r + 4 * u < r_end && q.c < k) ? x[(size_t)(r + 4 * u) * k + q.c] : 0.0f;
    }
    __device__ static __forceinline__ void store(double (*dst)[kGfLd], const float (&v)[kGhVals]) {
        const int n = threadIdx.x & 63, r = threadIdx.x >> 6;
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) dst[r + 4 * u][n] = (double)v[u];
    }
};

struct GhConv {
    const float* __restrict__ x;
    uint32_t k;
    int32_t height, width, hw, kw, khkw, stride_h, stride_w, pad_top, pad_left, dil_h, dil_w;
    uint32_t out_w, out_hw;
    int64_t image;        // elements of one image: C * H * W
    struct Cols {
        int32_t off[kGhVals];         // ci * H * W + ky * dy * W + kx * dx
        uint32_t reach[kGhVals];      // (ky * dy) << 16 | kx * dx; a column >= k: 0xFFFF << 16, which no row brings inside the image
    };
    __device__ __forceinline__ void cols(uint32_t c0, Cols& q) const {
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) {
            const uint32_t c = c0 + 8 * (threadIdx.x >> 5) + u;
            const int32_t ci = (int32_t)(c / (uint32_t)khkw), rem = (int32_t)c - ci * khkw;
            const int32_t ky = rem / kw, kx = rem - ky * kw;
            q.off[u] = c < k ? ci * hw + ky * dil_h * width + kx * dil_w : 0;
            q.reach[u] = c < k ? (uint32_t)(ky * dil_h) << 16 | (uint32_t)(kx * dil_w) : 0xFFFFu << 16;
        }
    }
    __device__ __forceinline__ void load(const Cols& q, uint32_t r0, uint32_t r_end, float (&v)[kGhVals]) const {
        const uint32_t r = r0 + (threadIdx.x & 31);
        int32_t iy0 = -(1 << 20), ix0 = 0;      // a row beyond the range: above every window's reach
        int64_t base = 0;
        if (r < r_end) {
            const uint32_t b = r / out_hw, rem = r - b * out_hw, oy = rem / out_w, ox = rem - oy * out_w;
            iy0 = (int32_t)oy * stride_h - pad_top;
            ix0 = (int32_t)ox * stride_w - pad_left;
            base = (int64_t)b * image + (int64_t)iy0 * width + ix0;
        }
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) {
            const int32_t iy = iy0 + (int32_t)(q.reach[u] >> 16), ix = ix0 + (int32_t)(q.reach[u] & 0xFFFFu);
            v[u] = ((uint32_t)iy < (uint32_t)height && (uint32_t)ix < (uint32_t)width) ? x[base + q.off[u]] : 0.0f;
        }
    }
    __device__ static __forceinline__ void store(double (*dst)[kGfLd], const float (&v)[kGhVals]) {
        const int r = threadIdx.x & 31, n0 = 8 * (threadIdx.x >> 5), j = (r >> 1) & 7;
        float a[kGhVals], b[kGhVals];      // b[u] = v[(u + j) & 7]
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) a[u] = (j & 1) ? v[(u + 1) & 7] : v[u];
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) b[u] = (j & 2) ? a[(u + 2) & 7] : a[u];
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) a[u] = (j & 4) ? b[(u + 4) & 7] : b[u];
#pragma unroll
        for (int u = 0; u < kGhVals; ++u) dst[r][n0 + ((u + j) & 7)] = (double)a[u];
    }
};

// (r, c) of H for element (m, n) of tile (ti, tj), when it is one the tile owns: inside H, on or below the diagonal.
__device__ __forceinline__ bool gh_owned(uint32_t ti, uint32_t tj, int m, int n, uint32_t k, uint32_t& r, uint32_t& c) {
    r = ti * kGfB + m;
    c = tj * kGfB + n;
    return r < k && c <= r;
}

template <class G>
__global__ __launch_bounds__(kBlock) void k_gh_tile(const G g, uint32_t k, uint32_t rows, uint32_t range_rows, uint32_t splits,
                                                     double* __restrict__ h, double* __restrict__ ws) {
    __shared__ GfTileLds s;
    uint32_t ti, tj;
    gf_lower_tile(blockIdx.x, ti, tj);
    const bool diag = ti == tj;      // (uniform over the workgroup)
    const uint32_t r_begin = blockIdx.y * range_rows, r_end = min(rows, r_begin + range_rows);
    typename G::Cols ca, cb;
    g.cols(ti * kGfB, ca);
    g.cols(tj * kGfB, cb);
    float va[kGhVals], vb[kGhVals];
    g.load(ca, r_begin, r_end, va);
    if (!diag) g.load(cb, r_begin, r_end, vb);
    d4 acc[2][2];
    gf_zero(acc);
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kGhPass) {
        G::store(s.a, va);
        if (!diag) G::store(s.b, vb);
        __syncthreads();
        if (r0 + kGhPass < r_end) {
            g.load(ca, r0 + kGhPass, r_end, va);
            if (!diag) g.load(cb, r0 + kGhPass, r_end, vb);
        }
        gf_mma_pass(s.a, diag ? s.a : s.b, acc);
        __syncthreads();
    }
    if (splits > 1) {
        double* p = ws + ((size_t)blockIdx.x * splits + blockIdx.y) * (kGfB * kGfB);
        gf_for_each(acc, [&](int m, int n, double v) { p[m * kGfB + n] = v; });
        return;
    }
    gf_for_each(acc, [&](int m, int n, double v) {
        uint32_t r, c;
        if (!gh_owned(ti, tj, m, n, k, r, c)) return;
        const double sum = h[(size_t)r * k + c] + v;
        h[(size_t)r * k + c] = sum;
        if (c != r) h[(size_t)c * k + r] = sum;
    });
}

__global__ __launch_bounds__(kBlock) void k_gh_reduce(const double* __restrict__ ws, uint32_t splits, uint32_t k, double* __restrict__ h) {
    uint32_t ti, tj;
    gf_lower_tile(blockIdx.x, ti, tj);
    const double* p = ws + (size_t)blockIdx.x * splits * (kGfB * kGfB);
    const int n = threadIdx.x & 63;
    for (int m = threadIdx.x >> 6; m < kGfB; m += kBlock / 64) {
        uint32_t r, c;
        if (!gh_owned(ti, tj, m, n, k, r, c)) continue;
        double sum = h[(size_t)r * k + c];
        for (uint32_t s = 0; s < splits; ++s) sum += p[(size_t)s * (kGfB * kGfB) + m * kGfB + n];
        h[(size_t)r * k + c] = sum;
        if (c != r) h[(size_t)c * k + r] = sum;
    }
}

template <class G>
void gh_launch(const G& g, const GhPlan& p, double* d_h, double* ws, hipStream_t s) {
    hipLaunchKernelGGL(k_gh_tile<G>, dim3(p.tiles, p.splits), dim3(kBlock), 0, s, g, p.k, p.rows, p.range_rows, p.splits, d_h, ws);
    if (p.splits > 1) hipLaunchKernelGGL(k_gh_reduce, dim3(p.tiles), dim3(kBlock), 0, s, ws, p.splits, p.k, d_h);
}

}  // namespace

extern "C" {

uint64_t dpl_gptq_hessian_workspace(int64_t k, int64_t rows) {
    return k < 1 || k > DPL_GPTQ_FACTOR_MAX_K || rows < 1 || rows > kGhMaxRows ? 0 : gh_plan(k, rows).bytes;
}

int dpl_gptq_hessian(const float* d_x, const dpl_gptq_hessian_geom* geom, int64_t k, int64_t rows, double* d_h, void* d_workspace,
                     uint64_t workspace_bytes, dpl_stream_t stream) {
    if (int rc = gh_check(d_x, geom, k, rows, d_h, d_workspace, workspace_bytes)) return rc;
    if (rows == 0) return 0;
    const GhPlan p = gh_plan(k, rows);
    if (geom == nullptr) {
        gh_launch(GhDense{d_x, p.k}, p, d_h, (double*)d_workspace, (hipStream_t)stream);
    } else {
        const dpl_gptq_hessian_geom& q = *geom;      // (gh_check: every value below fits its field)
        GhConv g;
        g.x = d_x;
        g.k = p.k;
        g.height = (int32_t)q.height, g.width = (int32_t)q.width, g.hw = (int32_t)(q.height * q.width);
        g.kw = (int32_t)q.kw, g.khkw = (int32_t)(q.kh * q.kw);
        g.stride_h = (int32_t)q.stride_h, g.stride_w = (int32_t)q.stride_w, g.pad_top = (int32_t)q.pad_top, g.pad_left = (int32_t)q.pad_left;
        g.dil_h = (int32_t)q.dil_h, g.dil_w = (int32_t)q.dil_w;
        g.out_w = (uint32_t)gh_out_w(q), g.out_hw = (uint32_t)(gh_out_h(q) * gh_out_w(q));
        g.image = q.channels * q.height * q.width;
        gh_launch(g, p, d_h, (double*)d_workspace, (hipStream_t)stream);
    }
    DPL_LAUNCH_CHECK("dpl_gptq_hessian");
    return 0;
}

}  // extern "C"
