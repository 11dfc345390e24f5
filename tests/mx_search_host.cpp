// Host-side harness of csrc/mx_search.hpp (tests/test_mx_search_host.py): the per-block arithmetic of --mx_scale_search, on the CPU.
//   mx_search_host <0|1> in.f32 out.scales out.err     — in: [blocks, 32] fp32 patterns; elem 0 = E4M3, 1 = E2M1;
//                                                        out.err: [blocks, 2] fp64 (the error at the floor, at the chosen byte)
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../dipoorlet_amd/csrc/mx_search.hpp"

template <int ELEM>
static void run(const std::vector<uint32_t>& x, std::vector<uint8_t>& sc, std::vector<double>& err) {
    for (size_t b = 0; b < sc.size(); ++b) {
        uint32_t a = 0;
        for (int i = 0; i < 32; ++i) a = std::max(a, x[b * 32 + i] & 0x7FFFFFFFu);
        sc[b] = (uint8_t)dpl_mx::search_block<ELEM>(&x[b * 32], a, &err[2 * b]);
    }
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / 4;
    fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> x(n);
    std::vector<uint8_t> sc(n / 32);
    std::vector<double> err(2 * (n / 32));
    if (fread(x.data(), 4, n, f) != (size_t)n) return 4;
    fclose(f);
    if (argv[1][0] == '0') run<0>(x, sc, err); else run<1>(x, sc, err);
    f = fopen(argv[3], "wb");
    fwrite(sc.data(), 1, sc.size(), f);
    fclose(f);
    f = fopen(argv[4], "wb");
    fwrite(err.data(), 8, err.size(), f);
    fclose(f);
    return 0;
}
