// What gfx950's v_cvt_pk_fp8_f32 / v_cvt_f32_fp8 do, over ALL 2^32 fp32 bit patterns, against the definition of the Float8E4M3FN
// quantisation type (tests/fp8_model.py, restated here in fp32 arithmetic — the form the kernel's e4m3_round uses,
// csrc/fake_quant_kernels.hip).  It answers whether the two instructions could replace that arithmetic:
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o fp8_cvt_probe scripts/fp8_cvt_probe.hip && ./fp8_cvt_probe
// Counts: `raw` = the two instructions alone; `guarded` = with an fp32 clamp to +-448 in front and NaN routed around them.  A
// result counts as equal when its 32 bits are (NaN: when both are NaN).  Exit status 0: guarded == definition everywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

enum { kInRangeBad, kAboveTo448, kAboveToNan, kAboveOther, kInfTo448, kInfToNan, kNanToNan, kNanOther, kGuardedBad, kCounters };

__device__ float raw_cvt(float v) {
    return __builtin_amdgcn_cvt_f32_fp8(__builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false), 0);
}

__device__ float guarded_cvt(float v) {
    const float r = raw_cvt(fminf(fmaxf(v, -448.f), 448.f));
    return v != v ? v : r;
}

__device__ float definition(float v) {   // step 2^(max(e, -6) - 3) of |v|'s binade e, round half to even, saturate, keep NaN and the sign
    if (v != v) return v;
    const float a = fminf(fabsf(v), 448.f);
    uint32_t e = __float_as_uint(a) >> 23;
    if (e < 121u) e = 121u;
    const float step = __uint_as_float((e - 3u) << 23);
    return copysignf(rintf(a / step) * step, v);
}

__device__ bool same(float a, float b) { return (a != a && b != b) || __float_as_uint(a) == __float_as_uint(b); }

__global__ void k_probe(unsigned long long* out, uint32_t* first_bad) {
    unsigned long long c[kCounters] = {};
    const uint64_t n_threads = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t b = t; b < (1ull << 32); b += n_threads) {
        const float v = __uint_as_float((uint32_t)b), want = definition(v), raw = raw_cvt(v);
        if (v != v) {
            c[raw != raw ? kNanToNan : kNanOther]++;
        } else if (isinf(v)) {
            c[raw != raw ? kInfToNan : kInfTo448]++;
        } else if (fabsf(v) > 448.f) {
            c[raw != raw ? kAboveToNan : fabsf(raw) == 448.f ? kAboveTo448 : kAboveOther]++;
        } else if (!same(raw, want)) {
            if (c[kInRangeBad]++ == 0) atomicMin(first_bad, (uint32_t)b);
        }
        if (!same(guarded_cvt(v), want)) c[kGuardedBad]++;
    }
    for (int i = 0; i < kCounters; ++i)
        if (c[i]) atomicAdd(out + i, c[i]);
}

__global__ void k_samples(const float* in, float* out, int n) {
    const int i = threadIdx.x;
    if (i < n) out[i] = raw_cvt(in[i]);
}

#define CHECK(x)                                                            \
    do {                                                                    \
        hipError_t e_ = (x);                                                \
        if (e_ != hipSuccess) {                                             \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    unsigned long long* d_c;
    uint32_t* d_first;
    unsigned long long c[kCounters];
    uint32_t first = 0xFFFFFFFFu;
    CHECK(hipMalloc(&d_c, sizeof(c)));
    CHECK(hipMalloc(&d_first, 4));
    CHECK(hipMemset(d_c, 0, sizeof(c)));
    CHECK(hipMemcpy(d_first, &first, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe, dim3(4096), dim3(256), 0, 0, d_c, d_first);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(c, d_c, sizeof(c), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&first, d_first, 4, hipMemcpyDeviceToHost));
    printf("finite |v| <= 448: raw != definition on %llu patterns (lowest: 0x%08x)\n", c[kInRangeBad], first);
    printf("finite |v| >  448: raw -> +-448 %llu, -> NaN %llu, -> other %llu\n", c[kAboveTo448], c[kAboveToNan], c[kAboveOther]);
    printf("+-inf: raw -> +-448 %llu, -> NaN %llu\n", c[kInfTo448], c[kInfToNan]);
    printf("NaN: raw -> NaN %llu, -> other %llu\n", c[kNanToNan], c[kNanOther]);
    printf("all 2^32 patterns: guarded != definition on %llu\n", c[kGuardedBad]);
    const float h_in[] = {0.0009765625f, 0.0029296875f, 0.00146484375f, -1e-9f, 449.f, 464.f, 465.f, 480.f, 1e9f, INFINITY, -INFINITY, NAN};
    const int n = sizeof(h_in) / sizeof(float);
    float *d_in, *d_out, h_out[n];
    CHECK(hipMalloc(&d_in, sizeof(h_in)));
    CHECK(hipMalloc(&d_out, sizeof(h_in)));
    CHECK(hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_samples, dim3(1), dim3(64), 0, 0, d_in, d_out, n);
    CHECK(hipMemcpy(h_out, d_out, sizeof(h_in), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) printf("raw(%.10g) = %.10g\n", h_in[i], h_out[i]);
    return c[kGuardedBad] != 0;
}
