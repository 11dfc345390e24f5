// Host-side harness of csrc/mx_plan.hpp (tests/test_mx_plan_host.py): the argument checks, the launch plans and the dispatches of the
// MX block kernels and of the two kernels on the block-scaled MFMA, on the CPU.  One request per line of stdin, one answer per line
// of stdout (a pointer the request does not give is a valid one; bit i of <null> makes the i-th of a_codes, a_scales, b_codes,
// b_scales, c null):
//   p <fp> <outer> <k> <inner> <tiles>                          -> rc K nblk cs vec n blocks | message
//   c <elem> <n null of 3> <outer> <k> <inner> <padded> <codes>  -> over rc | message
//   d <elem> <rows> <vec>                                       -> the (ELEM, ROWS, VEC) the dispatch instantiates
//   t <batch> <m> <n>                                           -> rc tiles_m tiles_n blocks | message
//   g <ea> <eb> <null> <a_codes> <b_codes> <batch> <m> <n> <k>   -> over rc tiles_m tiles_n blocks | message
//   v <ea> <eb> <null> <a_codes> <b_codes> <n h w c cout kh kw sh sw pt pl dh dw oh ow>
//                                                               -> over rc cb nblk m tiles_m tiles_n blocks | message
//   e <ea> <eb>                                                 -> the (EA, EB) the pair dispatch instantiates
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../dipoorlet_amd/csrc/mx_plan.hpp"

static MxPair pair_of(const uint64_t* a) {
    static const uint8_t there = 0;
    static float out = 0.f;
    const auto unless = [&](int bit, const uint8_t* p) { return (a[2] >> bit) & 1u ? nullptr : p; };
    return MxPair{(int32_t)a[0], (int32_t)a[1], unless(0, (const uint8_t*)(uintptr_t)a[3]), unless(1, &there), unless(2, (const uint8_t*)(uintptr_t)a[4]),
                  unless(3, &there), (a[2] >> 4) & 1u ? nullptr : &out};
}

int main() {
    char line[512];
    static const int there = 0;
    while (fgets(line, sizeof(line), stdin)) {
        uint64_t a[20];
        int n = 0;
        char* at = line + 1;
        for (char* end; n < 20; ++n, at = end) {      // (a negative number arrives as its two's complement)
            a[n] = strtoull(at, &end, 10);
            if (end == at) break;
        }
        g_err[0] = 0;
        if (line[0] == 'p' && n == 5) {
            MxPlan p;
            memset(&p, 0, sizeof(p));
            const int rc = mx_plan(p, "who", (uintptr_t)a[0], a[1], a[2], a[3], a[4] != 0);
            printf("%d %u %u %u %d %" PRIu64 " %" PRIu64 " | %s\n", rc, p.K, p.nblk, p.cs, (int)p.vec, p.n, p.blocks, g_err);
        } else if (line[0] == 'c' && n == 7) {
            const void* ptr[3] = {&there, &there, &there};
            for (uint64_t i = 0; i < a[1] && i < 3; ++i) ptr[2 - i] = nullptr;
            int rc = 77;
            const bool over = mx_check(rc, "who", (int32_t)a[0], "a, b and c", {ptr[0], ptr[1], ptr[2]}, a[2], a[3], a[4], a[5] != 0, (const void*)(uintptr_t)a[6]);
            printf("%d %d | %s\n", (int)over, rc, g_err);
        } else if (line[0] == 'd' && n == 3) {
            const int rc = mx_dispatch((int32_t)a[0], a[1] != 0, a[2] != 0, [](auto E, auto ROWS, auto VEC) {
                static_assert(E == DPL_MX_E4M3 || E == DPL_MX_E2M1, "");
                static_assert(VEC == 4 || VEC == 1, "");
                return 100 * (int)E + 10 * (int)ROWS + (int)VEC;
            });
            printf("%d\n", rc);
        } else if (line[0] == 't' && n == 3) {
            MxTiles t;
            memset(&t, 0, sizeof(t));
            const int rc = mx_tiles(t, "who", a[0], a[1], a[2]);
            printf("%d %u %u %" PRIu64 " | %s\n", rc, t.tiles_m, t.tiles_n, t.blocks, g_err);
        } else if (line[0] == 'g' && n == 9) {
            MxTiles t;
            memset(&t, 0, sizeof(t));
            int rc = 77;
            const bool over = mx_gemm_check(rc, t, pair_of(a), a[5], a[6], a[7], a[8]);
            printf("%d %d %u %u %" PRIu64 " | %s\n", (int)over, rc, t.tiles_m, t.tiles_n, t.blocks, g_err);
        } else if (line[0] == 'v' && n == 20) {
            MxConvPlan p;
            memset(&p, 0, sizeof(p));
            MxConvDims d;
            memcpy(&d, a + 5, sizeof(d));
            int rc = 77;
            const bool over = mx_conv_check(rc, p, pair_of(a), d);
            printf("%d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " | %s\n", (int)over, rc, p.cb, p.nblk, p.m, p.t.tiles_m, p.t.tiles_n,
                   p.t.blocks, g_err);
        } else if (line[0] == 'e' && n == 2) {
            const int rc = mx_pair_dispatch(MxPair{(int32_t)a[0], (int32_t)a[1], nullptr, nullptr, nullptr, nullptr, nullptr}, [](auto EA, auto EB) {
                static_assert((EA == DPL_MX_E4M3 || EA == DPL_MX_E2M1) && (EB == DPL_MX_E4M3 || EB == DPL_MX_E2M1), "");
                return 10 * (int)EA + (int)EB;
            });
            printf("%d\n", rc);
        } else {
            return 2;
        }
    }
    return 0;
}
