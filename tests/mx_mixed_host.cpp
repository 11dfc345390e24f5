// Host-side harness of csrc/mx_plan.hpp's mx_gemm_err_check (tests/test_mx_mixed_host.py): dpl_mx_gemm_err's argument rules on the
// CPU, in the manner of tests/mx_plan_host.cpp.  One request per line of stdin, one answer per line of stdout (a pointer the request
// does not give is a valid one; bit i of <null> makes the i-th of a_codes, a_scales, b_codes, b_scales, ref, part null):
//   r <ea> <eb> <null> <a_codes> <b_codes> <batch> <m> <n> <k>   -> over rc tiles_m tiles_n blocks | message
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../dipoorlet_amd/csrc/mx_plan.hpp"

int main() {
    char line[512];
    static const uint8_t there = 0;
    static const float ref = 0.f;
    static double part = 0.0;
    while (fgets(line, sizeof(line), stdin)) {
        uint64_t a[9];
        int n = 0;
        char* at = line + 1;
        for (char* end; n < 9; ++n, at = end) {       // (a negative number arrives as its two's complement)
            a[n] = strtoull(at, &end, 10);
            if (end == at) break;
        }
        g_err[0] = 0;
        if (line[0] != 'r' || n != 9) return 2;
        const auto unless = [&](int bit, const uint8_t* p) { return (a[2] >> bit) & 1u ? nullptr : p; };
        // (c is not an argument of dpl_mx_gemm_err: null here, and the check must not look at it)
        const MxPair o = {(int32_t)a[0], (int32_t)a[1], unless(0, (const uint8_t*)(uintptr_t)a[3]), unless(1, &there),
                          unless(2, (const uint8_t*)(uintptr_t)a[4]), unless(3, &there), nullptr};
        MxTiles t;
        memset(&t, 0, sizeof(t));
        int rc = 77;
        const bool over = mx_gemm_err_check(rc, t, o, (a[2] >> 4) & 1u ? nullptr : &ref, (a[2] >> 5) & 1u ? nullptr : &part, a[5], a[6], a[7], a[8]);
        printf("%d %d %u %u %" PRIu64 " | %s\n", (int)over, rc, t.tiles_m, t.tiles_n, t.blocks, g_err);
    }
    return 0;
}
