// Host-side harness of csrc/mx_format.hpp's element codes (tests/test_mx_codes_host.py): encode_bits / decode_bits on the CPU, in
// the rows layout of tests/mx_pack_model.py (blocks of 32 back to back; E2M1 two to a byte, the even index in the low nibble).
//   mx_codes_host <0|1> enc in.f32 out.codes out.scales    — in: [blocks, 32] fp32 patterns; elem 0 = E4M3, 1 = E2M1; exit 5
//                                                            if round_code (the kernels' one step) disagrees with encode_bits anywhere
//   mx_codes_host <0|1> dec in.codes in.scales out.f32     — in: [blocks, 32 | 16] code bytes, [blocks] scale bytes
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../dipoorlet_amd/csrc/mx_format.hpp"

template <typename T>
static bool slurp(const char* path, std::vector<T>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(T);
    fseek(f, 0, SEEK_SET);
    v.resize(n);
    const bool ok = n == 0 || fread(v.data(), sizeof(T), n, f) == (size_t)n;
    fclose(f);
    return ok;
}

template <typename T>
static bool dump(const char* path, const std::vector<T>& v) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

static size_t mismatches = 0;     // encode_bits(round_bits(v)) != round_code(v)

template <int ELEM>
static void enc(const std::vector<uint32_t>& x, std::vector<uint8_t>& codes, std::vector<uint8_t>& sc) {
    constexpr int per_byte = ELEM == 0 ? 1 : 2;
    sc.assign(x.size() / 32, 0);
    codes.assign(x.size() / per_byte, 0);
    for (size_t b = 0; b < sc.size(); ++b) {
        uint32_t a = 0;
        for (int i = 0; i < 32; ++i) a = std::max(a, x[b * 32 + i] & 0x7FFFFFFFu);
        const bool nan = a >= 0x7F800000u;
        const int se = (nan || a == 0) ? -127 : dpl_mx::shared_exponent<ELEM>(a);
        sc[b] = nan ? 0xFF : (uint8_t)(se + 127);
        for (int i = 0; i < 32; ++i) {
            const uint32_t v = x[b * 32 + i];
            const uint32_t y = (v & 0x80000000u) | dpl_mx::round_bits<ELEM>(v & 0x7FFFFFFFu, se);
            const uint32_t c = nan ? (ELEM == 0 ? 0x7Fu : 0u) : dpl_mx::encode_bits<ELEM>(y, se);
            // the kernels' one-step form must be the same code (a NaN element of a 0xFF block has no code of its own)
            if (!nan && c != (((v >> 31) << (ELEM == 0 ? 7 : 3)) | dpl_mx::round_code<ELEM>(v & 0x7FFFFFFFu, se))) ++mismatches;
            if (ELEM == 0)
                codes[b * 32 + i] = (uint8_t)c;
            else
                codes[b * 16 + i / 2] |= (uint8_t)(c << (4 * (i & 1)));
        }
    }
}

template <int ELEM>
static void dec(const std::vector<uint8_t>& codes, const std::vector<uint8_t>& sc, std::vector<uint32_t>& y) {
    y.assign(sc.size() * 32, 0);
    for (size_t b = 0; b < sc.size(); ++b)
        for (int i = 0; i < 32; ++i) {
            const uint32_t c = ELEM == 0 ? codes[b * 32 + i] : (codes[b * 16 + i / 2] >> (4 * (i & 1))) & 0xFu;
            y[b * 32 + i] = sc[b] == 0xFF ? 0x7FC00000u : dpl_mx::decode_bits<ELEM>(c, (int)sc[b] - 127);
        }
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const bool e4m3 = argv[1][0] == '0';
    if (!strcmp(argv[2], "enc")) {
        std::vector<uint32_t> x;
        std::vector<uint8_t> codes, sc;
        if (!slurp(argv[3], x) || x.size() % 32) return 3;
        if (e4m3) enc<0>(x, codes, sc); else enc<1>(x, codes, sc);
        if (mismatches) return 5;
        return dump(argv[4], codes) && dump(argv[5], sc) ? 0 : 4;
    }
    if (!strcmp(argv[2], "dec")) {
        std::vector<uint8_t> codes, sc;
        std::vector<uint32_t> y;
        if (!slurp(argv[3], codes) || !slurp(argv[4], sc) || codes.size() != sc.size() * (e4m3 ? 32 : 16)) return 3;
        if (e4m3) dec<0>(codes, sc, y); else dec<1>(codes, sc, y);
        return dump(argv[5], y) ? 0 : 4;
    }
    return 2;
}
