// Host-side harness of the two MXFP6 formats (tests/test_mx_fp6_host.py): csrc/mx_format.hpp's arithmetic under the records
// Fmt<DPL_MX_E2M3> and Fmt<DPL_MX_E3M2>, and csrc/mx_plan.hpp's checks and dispatches over all four formats, on the CPU.  One
// request per line of stdin, one answer per line of stdout:
//   r <elem> <|v| bits> <se + 127>   -> round_bits round_code encode_bits(round_bits) decode_bits(round_code), all as integers
//   s <elem> <|a| bits>              -> shared_exponent
//   x <elem> <code> <se + 127>       -> decode_bits, and encode_bits of it
//   t <elem>                         -> bits nan_code mfma of the format's record
//   d <elem> <rows> <vec>            -> the (ELEM, ROWS, VEC) mx_dispatch_all instantiates
//   e <ea> <eb>                      -> the (EA, EB) mx_pair_dispatch_all instantiates
//   c <elem>                         -> over rc | message of mx_check
//   g <ea> <eb>                      -> over rc | message of mx_gemm_check
//   m <ea> <eb>                      -> over rc | message of mx_gemm_err_check
//   v <ea> <eb>                      -> over rc | message of mx_conv_check
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../dipoorlet_amd/csrc/mx_format.hpp"
#include "../dipoorlet_amd/csrc/mx_plan.hpp"

template <class F>
static int by_fp6(int elem, F f) {
    return elem == DPL_MX_E2M3 ? f(std::integral_constant<int, DPL_MX_E2M3>{}) : f(std::integral_constant<int, DPL_MX_E3M2>{});
}

int main() {
    char line[256];
    static const uint8_t there[64] = {0};
    static float out = 0.f;
    static double part[2] = {0.0, 0.0};
    alignas(16) static const uint8_t codes[64] = {0};
    while (fgets(line, sizeof(line), stdin)) {
        uint64_t a[4];
        int n = 0;
        char* at = line + 1;
        for (char* end; n < 4; ++n, at = end) {
            a[n] = strtoull(at, &end, 10);
            if (end == at) break;
        }
        g_err[0] = 0;
        const int elem = (int)(int64_t)a[0];
        const MxPair pair = {(int32_t)(int64_t)a[0], (int32_t)(int64_t)a[1], codes, there, codes, there, &out};
        if (line[0] == 'r' && n == 3 && (elem == DPL_MX_E2M3 || elem == DPL_MX_E3M2)) {
            by_fp6(elem, [&](auto E) {
                const uint32_t b = (uint32_t)a[1];
                const int se = (int)a[2] - 127;
                const uint32_t y = dpl_mx::round_bits<E>(b, se), c = dpl_mx::round_code<E>(b, se);
                printf("%u %u %u %u\n", y, c, dpl_mx::encode_bits<E>(y, se), dpl_mx::decode_bits<E>(c, se));
                return 0;
            });
        } else if (line[0] == 's' && n == 2 && (elem == DPL_MX_E2M3 || elem == DPL_MX_E3M2)) {
            printf("%d\n", by_fp6(elem, [&](auto E) { return dpl_mx::shared_exponent<E>((uint32_t)a[1]); }));
        } else if (line[0] == 'x' && n == 3 && (elem == DPL_MX_E2M3 || elem == DPL_MX_E3M2)) {
            by_fp6(elem, [&](auto E) {
                const int se = (int)a[2] - 127;
                const uint32_t y = dpl_mx::decode_bits<E>((uint32_t)a[1], se);
                printf("%u %u\n", y, dpl_mx::encode_bits<E>(y, se));
                return 0;
            });
        } else if (line[0] == 't' && n == 1 && (elem == DPL_MX_E2M3 || elem == DPL_MX_E3M2)) {
            by_fp6(elem, [&](auto E) {
                printf("%u %u %d\n", dpl_mx::Fmt<E>::bits, dpl_mx::Fmt<E>::nan_code, dpl_mx::Fmt<E>::mfma);
                return 0;
            });
        } else if (line[0] == 'd' && n == 3) {
            printf("%d\n", mx_dispatch_all((int32_t)elem, a[1] != 0, a[2] != 0, [](auto E, auto ROWS, auto VEC) {
                       static_assert(VEC == 4 || VEC == 1, "");
                       return 100 * (int)E + 10 * (int)ROWS + (int)VEC;
                   }));
        } else if (line[0] == 'e' && n == 2) {
            printf("%d\n", mx_pair_dispatch_all(pair, [](auto EA, auto EB) { return 10 * (int)EA + (int)EB; }));
        } else if (line[0] == 'c' && n == 1) {
            int rc = 77;
            const bool over = mx_check(rc, "who", (int32_t)elem, "a and b", {there, there}, 2, 40, 3, true, codes);
            printf("%d %d | %s\n", (int)over, rc, g_err);
        } else if (line[0] == 'g' && n == 2) {
            int rc = 77;
            MxTiles t;
            memset(&t, 0, sizeof(t));
            const bool over = mx_gemm_check(rc, t, pair, 1, 8, 6, 64);
            printf("%d %d | %s\n", (int)over, rc, g_err);
        } else if (line[0] == 'm' && n == 2) {
            int rc = 77;
            MxTiles t;
            memset(&t, 0, sizeof(t));
            const bool over = mx_gemm_err_check(rc, t, pair, &out, part, 1, 8, 6, 64);
            printf("%d %d | %s\n", (int)over, rc, g_err);
        } else if (line[0] == 'v' && n == 2) {
            int rc = 77;
            MxConvPlan p;
            memset(&p, 0, sizeof(p));
            const bool over = mx_conv_check(rc, p, pair, MxConvDims{2, 9, 9, 33, 5, 3, 3, 2, 2, 1, 1, 1, 1, 5, 5});
            printf("%d %d | %s\n", (int)over, rc, g_err);
        } else {
            return 2;
        }
    }
    return 0;
}
