// Host-side harness of csrc/mx_format.hpp (tests/test_mx_format_host.py): the arithmetic the MX kernels run per block, on the CPU.
//   mx_format_host <0|1> in.f32 out.f32 out.scales     — in: [blocks, 32] fp32 patterns; elem 0 = E4M3, 1 = E2M1
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../dipoorlet_amd/csrc/mx_format.hpp"

template <int ELEM>
static void run(const std::vector<uint32_t>& x, std::vector<uint32_t>& y, std::vector<uint8_t>& sc) {
    for (size_t b = 0; b < sc.size(); ++b) {
        uint32_t a = 0;
        for (int i = 0; i < 32; ++i) a = std::max(a, x[b * 32 + i] & 0x7FFFFFFFu);
        const bool nan = a >= 0x7F800000u;
        const int se = (nan || a == 0) ? -127 : dpl_mx::shared_exponent<ELEM>(a);
        sc[b] = nan ? 0xFF : (uint8_t)(se + 127);
        for (int i = 0; i < 32; ++i) {
            const uint32_t v = x[b * 32 + i];
            y[b * 32 + i] = nan ? 0x7FC00000u : ((v & 0x80000000u) | dpl_mx::round_bits<ELEM>(v & 0x7FFFFFFFu, se));
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / 4;
    fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> x(n), y(n);
    std::vector<uint8_t> sc(n / 32);
    if (fread(x.data(), 4, n, f) != (size_t)n) return 4;
    fclose(f);
    if (argv[1][0] == '0') run<0>(x, y, sc); else run<1>(x, y, sc);
    f = fopen(argv[3], "wb");
    fwrite(y.data(), 4, n, f);
    fclose(f);
    f = fopen(argv[4], "wb");
    fwrite(sc.data(), 1, sc.size(), f);
    fclose(f);
    return 0;
}
