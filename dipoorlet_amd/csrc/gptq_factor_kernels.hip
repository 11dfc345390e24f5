// K13: GPTQ's Hessian factorisation on the device, in fp64 (--gptq_factor device).  For H' = H with dead diagonals
// set to 1 plus damp * mean(diag) * I, U = the upper Cholesky factor of H'^-1 is ONE Cholesky factorisation and ONE triangular
// inverse: H'^-1 = U^T U means H' = V V^T with V = U^-1 upper, and with P the index reversal, P H' P = L L^T (L the ordinary lower
// factor) gives V = P L P and U = P L^-1 P.  The workspace holds P H' P padded to a multiple of 64 with an identity (kp = 64 * nb),
// L over it in place, a 64 x 64 inverse per diagonal block, and X = L^-1; every tile is whole, so no kernel below tests a bound.
//
//   k_gf_prepare      tile (i, j <= i) of P H' P; the diagonal tiles sum the diagonal themselves (fixed order, below) and add the
//                     damping; tile (0, 0) clears the status word.
//   per block step k = 0 .. nb - 1 of the right-looking Cholesky:
//   k_gf_diag         one workgroup: A_kk -> L_kk in LDS, column by column, then L_kk^-1 (row by row); a pivot that is not > 0 (a
//                     NaN too) is recorded, while the word is still 0, as 1 + its column of H (a pivot of the padding as k), and
//                     the sweep goes on.
//   k_gf_panel        L_ik = A_ik . (L_kk^-1)^T for i > k: a product on the matrix instruction, not a substitution.
//   k_gf_syrk         A_ij -= L_ik . L_jk^T for k < j <= i, one 64 x 64 tile per workgroup.
//   per block step k of the right-looking inverse (L X = I; DESIGN.md §3w says why not block row by block row):
//   k_gf_inv_row      X_kj = L_kk^-1 . B_kj for j < k, X_kk = L_kk^-1: row k is final.
//   k_gf_inv_update   B_ij -= L_ik . X_kj for i > k, j <= k; B_ik starts at 0, so j == k stores and does not read.
//   k_gf_store        U[a][b] = X[K - 1 - a][K - 1 - b] for a <= b, exact zeros below.
//
// The product.  Every 64 x 64 tile is gf_tile_mma over the tile body of gptq_f64_tile.hpp (2 x 2 waves of 2 x 2
// v_mfma_f64_16x16x4_f64 accumulators, operands staged [k][64 + 16]; the instruction's lane map is written down there).  An
// operand whose reduction index is contiguous in memory (rows of L, of L_kk^-1) is read 64 bytes per lane and transposed on the way
// in; X's rows go in as they are.  No split along k, no atomics: an element is one chain of fused multiply-adds in ascending k
// whatever the grid, so two runs on the same sources and hardware give the same bits, and so does every rank.
//
// Diagonal sum: thread t of the one workgroup's 256 adds d[t], d[t + 256], ... in ascending order, then the 256 partial sums are
// halved in LDS, 128 + 128, 64 + 64, ... — one order for every K.
#include "gptq_f64_tile.hpp"

namespace {

// Stage 64 (m) x 32 (k) of an operand whose k runs along memory: src[m * ld + k] -> dst[k][m].  Thread t: row t & 63, eight
// consecutive k from 8 * (t >> 6): 64 contiguous bytes per lane, and consecutive lanes write consecutive doubles of a staged row.
__device__ __forceinline__ void gf_stage_kcontig(double (*dst)[kGfLd], const double* __restrict__ src, size_t ld) {
    const int m = threadIdx.x & 63, k0 = (threadIdx.x >> 6) * 8;
    const double* p = src + (size_t)m * ld + k0;
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[u];
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[k0 + u][m] = v[u];
}

// Stage 32 (k) x 64 (n) of an operand whose n runs along memory: src[k * ld + n] -> dst[k][n].
__device__ __forceinline__ void gf_stage_ncontig(double (*dst)[kGfLd], const double* __restrict__ src, size_t ld) {
    const int n = threadIdx.x & 63, k0 = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[k0 + 4 * u][n] = src[(size_t)(k0 + 4 * u) * ld + n];
}

// acc += A . B over `depth` (a multiple of 32) values of k.  A: a[m * lda + k].  B: b[n * ldb + k] (B_KCONTIG) or b[k * ldb + n].
template <bool B_KCONTIG>
__device__ __forceinline__ void gf_tile_mma(GfTileLds& s, d4 (&acc)[2][2], const double* __restrict__ a, size_t lda,
                                            const double* __restrict__ b, size_t ldb, int depth) {
    for (int k = 0; k < depth; k += kGfKc) {
        gf_stage_kcontig(s.a, a + k, lda);
        if (B_KCONTIG) gf_stage_kcontig(s.b, b + k, ldb);
        else gf_stage_ncontig(s.b, b + (size_t)k * ldb, ldb);
        __syncthreads();
        gf_mma_pass(s, acc);
        __syncthreads();
    }
}

// mean(diag H') before the damping, the dead diagonals already 1: the fixed order of the head comment.  All 256 threads call it.
__device__ double gf_diag_mean(const double* __restrict__ h, uint32_t k, double* red) {
    double sum = 0.0;
    for (uint32_t c = threadIdx.x; c < k; c += kBlock) {
        const double d = h[(size_t)c * k + c];
        sum += d == 0.0 ? 1.0 : d;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0] / (double)k;
}

__global__ __launch_bounds__(kBlock) void k_gf_prepare(const double* __restrict__ h, uint32_t k, double damp, double* __restrict__ a,
                                                        size_t kp, int32_t* __restrict__ status) {
    __shared__ double red[kBlock];
    uint32_t ti, tj;
    gf_lower_tile(blockIdx.x, ti, tj);
    double add = 0.0;
    if (ti == tj) add = damp * gf_diag_mean(h, k, red);      // (uniform over the workgroup)
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
    const uint32_t c = tj * kGfB + (threadIdx.x & 63);
    for (int rr = threadIdx.x >> 6; rr < kGfB; rr += kBlock / 64) {
        const uint32_t r = ti * kGfB + rr;
        double v = r == c ? 1.0 : 0.0;                         // the padding: an identity
        if (r < k && c < k) {
            v = h[(size_t)(k - 1 - r) * k + (k - 1 - c)];
            if (r == c) v = (v == 0.0 ? 1.0 : v) + add;
        }
        a[(size_t)r * kp + c] = v;
    }
}

// A_kk -> L_kk (over it, zeros above the diagonal) and L_kk^-1 (linv, zeros above), both 64 x 64 in LDS.  L is held transposed
// (Lt[j][r] = L[r][j]): a column of L is then a row of LDS, and with lane = r every read of either sweep is a run of consecutive
// doubles or one address for the whole wave.  Step j of a sweep: one column of L (one row of the inverse) is scaled, then the rest
// takes its rank-1 update.
__global__ __launch_bounds__(kBlock) void k_gf_diag(double* __restrict__ a, size_t kp, uint32_t kb, uint32_t k, double* __restrict__ linv,
                                                     int32_t* __restrict__ status) {
    __shared__ double Lt[kGfB][kGfB];
    __shared__ double T[kGfB][kGfB];
    double* tile = a + ((size_t)kb * kGfB) * kp + (size_t)kb * kGfB;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = w; r < kGfB; r += 4) {
        Lt[lane][r] = lane <= r ? tile[(size_t)r * kp + lane] : 0.0;
        T[r][lane] = r == lane ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < kGfB; ++j) {
        const double d = Lt[j][j];
        __syncthreads();
        if (!(d > 0.0) && threadIdx.x == 0 && *status == 0) {      // (column k - 1 - index of H; the padding, index >= k, reports k)
            const uint32_t idx = kb * kGfB + j;
            *status = idx < k ? (int32_t)(k - idx) : (int32_t)k;
        }
        const double piv = sqrt(d);
        if (w == 0 && lane >= j) Lt[j][lane] = lane == j ? piv : Lt[j][lane] / piv;
        __syncthreads();
        for (int c = j + 1 + w; c <= lane; c += 4) Lt[c][lane] -= Lt[j][lane] * Lt[j][c];      // L[r][c] -= L[r][j] L[c][j], r = lane
        __syncthreads();
    }
    for (int j = 0; j < kGfB; ++j) {
        if (w == 0 && lane <= j) T[j][lane] /= Lt[j][j];
        __syncthreads();
        for (int r = j + 1 + w; r < kGfB; r += 4)
            if (lane <= j) T[r][lane] -= Lt[j][r] * T[j][lane];
        __syncthreads();
    }
    double* inv = linv + (size_t)kb * kGfB * kGfB;
    for (int r = w; r < kGfB; r += 4) {
        tile[(size_t)r * kp + lane] = Lt[lane][r];
        inv[r * kGfB + lane] = T[r][lane];
    }
}

// L_ik = A_ik . (L_kk^-1)^T, i = kb + 1 + blockIdx.x, in place: the workgroup reads no tile but its own and the inverse.
__global__ __launch_bounds__(kBlock) void k_gf_panel(double* __restrict__ a, size_t kp, uint32_t kb, const double* __restrict__ linv) {
    __shared__ GfTileLds s;
    double* tile = a + ((size_t)(kb + 1 + blockIdx.x) * kGfB) * kp + (size_t)kb * kGfB;
    d4 acc[2][2];
    gf_zero(acc);
    gf_tile_mma<true>(s, acc, tile, kp, linv + (size_t)kb * kGfB * kGfB, kGfB, kGfB);
    gf_for_each(acc, [&](int r, int c, double v) { tile[(size_t)r * kp + c] = v; });
}

// A_ij -= L_ik . L_jk^T over the tiles kb < j <= i: reads column block kb, writes to its right.
__global__ __launch_bounds__(kBlock) void k_gf_syrk(double* __restrict__ a, size_t kp, uint32_t kb) {
    __shared__ GfTileLds s;
    uint32_t ti, tj;
    gf_lower_tile(blockIdx.x, ti, tj);
    const size_t i0 = (size_t)(kb + 1 + ti) * kGfB, j0 = (size_t)(kb + 1 + tj) * kGfB, k0 = (size_t)kb * kGfB;
    d4 acc[2][2];
    gf_zero(acc);
    gf_tile_mma<true>(s, acc, a + i0 * kp + k0, kp, a + j0 * kp + k0, kp, kGfB);
    double* tile = a + i0 * kp + j0;
    gf_for_each(acc, [&](int r, int c, double v) { tile[(size_t)r * kp + c] -= v; });
}

// Row kb of X becomes final: X_kj = L_kk^-1 . B_kj in place for j = blockIdx.x < kb (both passes are staged before the first store),
// X_kk = L_kk^-1 for j == kb.
__global__ __launch_bounds__(kBlock) void k_gf_inv_row(double* __restrict__ x, size_t kp, uint32_t kb, const double* __restrict__ linv) {
    __shared__ GfTileLds s;
    const double* inv = linv + (size_t)kb * kGfB * kGfB;
    double* tile = x + ((size_t)kb * kGfB) * kp + (size_t)blockIdx.x * kGfB;
    if (blockIdx.x == kb) {
        const int c = threadIdx.x & 63;
        for (int r = threadIdx.x >> 6; r < kGfB; r += 4) tile[(size_t)r * kp + c] = inv[r * kGfB + c];
        return;
    }
    d4 acc[2][2];
    gf_zero(acc);
    gf_tile_mma<false>(s, acc, inv, kGfB, tile, kp, kGfB);
    gf_for_each(acc, [&](int r, int c, double v) { tile[(size_t)r * kp + c] = v; });
}

// B_ij -= L_ik . X_kj for i = kb + 1 + blockIdx.y, j = blockIdx.x <= kb: reads row kb of X and column block kb of L, writes below.
__global__ __launch_bounds__(kBlock) void k_gf_inv_update(double* __restrict__ x, size_t kp, uint32_t kb, const double* __restrict__ l) {
    __shared__ GfTileLds s;
    const size_t i0 = (size_t)(kb + 1 + blockIdx.y) * kGfB, j0 = (size_t)blockIdx.x * kGfB, k0 = (size_t)kb * kGfB;
    d4 acc[2][2];
    gf_zero(acc);
    gf_tile_mma<false>(s, acc, l + i0 * kp + k0, kp, x + k0 * kp + j0, kp, kGfB);
    double* tile = x + i0 * kp + j0;
    if (blockIdx.x == kb) gf_for_each(acc, [&](int r, int c, double v) { tile[(size_t)r * kp + c] = -v; });
    else gf_for_each(acc, [&](int r, int c, double v) { tile[(size_t)r * kp + c] -= v; });
}

// U[a][b] = X[k - 1 - a][k - 1 - b] on and above the diagonal, 0.0 below: 64 x 64 of U per workgroup (the edges are tested: U has
// no padding).
__global__ __launch_bounds__(kBlock) void k_gf_store(const double* __restrict__ x, size_t kp, uint32_t k, double* __restrict__ u) {
    const uint32_t b = blockIdx.x * kGfB + (threadIdx.x & 63);
    if (b >= k) return;
    for (int rr = threadIdx.x >> 6; rr < kGfB; rr += 4) {
        const uint32_t a = blockIdx.y * kGfB + rr;
        if (a < k) u[(size_t)a * k + b] = a <= b ? x[(size_t)(k - 1 - a) * kp + (k - 1 - b)] : 0.0;
    }
}

}  // namespace

extern "C" {

uint64_t dpl_gptq_factor_workspace(int64_t k) { return k < 1 || k > DPL_GPTQ_FACTOR_MAX_K ? 0 : gf_plan(k).bytes; }

int dpl_gptq_factor_phase(const double* d_h, int64_t k, double damp, double* d_u, int32_t* d_status, void* d_workspace,
                          uint64_t workspace_bytes, int32_t phases, dpl_stream_t stream) {
    if (int rc = gf_check(d_h, k, damp, d_u, d_status, d_workspace, workspace_bytes, phases)) return rc;
    const GfPlan p = gf_plan(k);
    const size_t kp = (size_t)p.kp;
    double *a = (double*)d_workspace, *x = a + p.x, *linv = a + p.linv;
    hipStream_t s = (hipStream_t)stream;
    if (phases & 1) {
        hipLaunchKernelGGL(k_gf_prepare, dim3(GfPlan::lower(p.nb)), dim3(kBlock), 0, s, d_h, p.k, damp, a, kp, d_status);
        for (uint32_t kb = 0; kb < p.nb; ++kb) {
            hipLaunchKernelGGL(k_gf_diag, dim3(1), dim3(kBlock), 0, s, a, kp, kb, p.k, linv, d_status);
            if (p.below(kb) == 0) break;
            hipLaunchKernelGGL(k_gf_panel, dim3(p.below(kb)), dim3(kBlock), 0, s, a, kp, kb, linv);
            hipLaunchKernelGGL(k_gf_syrk, dim3(GfPlan::lower(p.below(kb))), dim3(kBlock), 0, s, a, kp, kb);
        }
        DPL_LAUNCH_CHECK("dpl_gptq_factor (Cholesky)");
    }
    if (phases & 2) {
        for (uint32_t kb = 0; kb < p.nb; ++kb) {
            hipLaunchKernelGGL(k_gf_inv_row, dim3(kb + 1), dim3(kBlock), 0, s, x, kp, kb, linv);
            if (p.below(kb) > 0) hipLaunchKernelGGL(k_gf_inv_update, dim3(kb + 1, p.below(kb)), dim3(kBlock), 0, s, x, kp, kb, a);
        }
        hipLaunchKernelGGL(k_gf_store, dim3(p.nb, p.nb), dim3(kBlock), 0, s, x, kp, p.k, d_u);
        DPL_LAUNCH_CHECK("dpl_gptq_factor (inverse)");
    }
    return 0;
}

int dpl_gptq_factor(const double* d_h, int64_t k, double damp, double* d_u, int32_t* d_status, void* d_workspace, uint64_t workspace_bytes,
                    dpl_stream_t s) {
    return dpl_gptq_factor_phase(d_h, k, damp, d_u, d_status, d_workspace, workspace_bytes, 3, s);
}

}  // extern "C"
