// A host build of csrc/slk_cut8.h for tests/test_cut8_sr_cpu.py: the stochastic-rounding encode of whole samples
// with the header's integer functions, so the test can hold them to tests/cut8_sr_ref.py without a GPU.
//   cut8_sr_host IN OUT FMT SEED STEP ROW0
// IN: n rows of 16,384 bf16 (uint16, little endian). OUT: n records of 16,400 bytes, then n decoded rows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slk_cut8.h"

template <int FMT>
static void run(const std::vector<uint16_t>& x, size_t n, uint32_t seed, uint32_t step, uint32_t row0, std::vector<uint8_t>& rec,
                std::vector<uint16_t>& dec) {
    for (size_t row = 0; row < n; ++row) {
        const uint16_t* xr = &x[row * cut8::SAMPLE];
        uint8_t* r = &rec[row * cut8::RECORD];
        uint16_t* d = &dec[row * cut8::SAMPLE];
        uint32_t a = 0;
        for (int i = 0; i < cut8::SAMPLE; ++i) a = a > (xr[i] & 0x7fffu) ? a : (xr[i] & 0x7fffu);
        const bool poison = a >= 0x7f80u;
        const int32_t e = poison ? cut8::POISON : cut8::scale_exp<FMT>(a);
        const uint32_t head[4] = {(uint32_t)e, (uint32_t)FMT, 0u, 0u};
        std::memcpy(r, head, sizeof head);
        const uint32_t base = cut8::sr_base(row0 + (uint32_t)row, step, seed, FMT);
        for (int i = 0; i < cut8::SAMPLE; ++i) {
            const uint32_t c = poison ? 0u : cut8::encode_one_sr<FMT>(xr[i], e, cut8::sr_word(base, (uint32_t)i));
            r[cut8::HEADER + i] = (uint8_t)c;
            d[i] = poison ? cut8::BF16_NAN : cut8::decode_one<FMT>(c, e);
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    std::fseek(in, 0, SEEK_END);
    const long bytes = std::ftell(in);
    std::fseek(in, 0, SEEK_SET);
    const size_t n = (size_t)bytes / (2 * cut8::SAMPLE);
    std::vector<uint16_t> x(n * cut8::SAMPLE), dec(n * cut8::SAMPLE);
    std::vector<uint8_t> rec(n * cut8::RECORD);
    if (std::fread(x.data(), 2, x.size(), in) != x.size()) return 4;
    std::fclose(in);
    const int fmt = std::atoi(argv[3]);
    const uint32_t seed = (uint32_t)std::strtoul(argv[4], nullptr, 0), step = (uint32_t)std::strtoul(argv[5], nullptr, 0);
    const uint32_t row0 = (uint32_t)std::strtoul(argv[6], nullptr, 0);
    if (fmt == 0) run<0>(x, n, seed, step, row0, rec, dec);
    else if (fmt == 1) run<1>(x, n, seed, step, row0, rec, dec);
    else return 5;
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 6;
    std::fwrite(rec.data(), 1, rec.size(), out);
    std::fwrite(dec.data(), 2, dec.size(), out);
    return std::fclose(out) == 0 ? 0 : 7;
}
