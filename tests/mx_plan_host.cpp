// Host-side harness of csrc/mx_plan.hpp (tests/test_mx_plan_host.py): the argument check, the launch plan and the dispatch of the MX
// block kernels, on the CPU.  One request per line of stdin, one answer per line of stdout:
//   p <fp> <outer> <k> <inner> <tiles>                          -> rc K nblk cs vec n blocks | message
//   c <elem> <n null of 3> <outer> <k> <inner> <padded> <codes>  -> over rc | message
//   d <elem> <rows> <vec>                                       -> the (ELEM, ROWS, VEC) the dispatch instantiates
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../dipoorlet_amd/csrc/mx_plan.hpp"

int main() {
    char line[256];
    static const int there = 0;
    while (fgets(line, sizeof(line), stdin)) {
        uint64_t a[7] = {0, 0, 0, 0, 0, 0, 0};
        const int n = sscanf(line + 1, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a[0], &a[1], &a[2], &a[3],
                             &a[4], &a[5], &a[6]);
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
        } else {
            return 2;
        }
    }
    return 0;
}
