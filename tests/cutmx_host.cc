// cutmx_host.cc — a host build of csrc/slk_cutmx.h for tests/test_cutmx_cpu.py: the integer arithmetic the kernels
// run with -DSLK_CUTMX_HWCVT=0, around the record layout of include/slk.h ("MX cut records") restated here in plain
// loops. Stand-alone (its own main), so that it can also be built with -fsanitize=address,undefined and run as is.
//
//   cutmx_host exps  FMT out          int16 [0x7f80]: block_exp of every finite amax bit pattern
//   cutmx_host codes FMT out          u8 [e_hi - e_lo + 1][65536]: encode_code of every bf16 bit pattern under every
//                                     e in [-100, e_hi] (the caller ignores the entries the rule does not reach)
//   cutmx_host vals  FMT out          u16 [228][16 | 256]: decode_code of every code under every scale byte 27..254
//   cutmx_host encode FMT in out      bf16 [n][16384] -> records u8 [n][R]
//   cutmx_host decode FMT in out      records -> bf16 [n][16384]; prints the error flag
//   cutmx_host roundtrip FMT in out   bf16 -> bf16, without a record
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "slk_cutmx.h"

namespace {
std::vector<uint8_t> read_all(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::vector<uint8_t> buf;
    uint8_t tmp[1 << 16];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    std::fclose(f);
    return buf;
}

void write_all(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::perror(path); std::exit(2); }
    std::fclose(f);
}

uint16_t load16(const uint8_t* p) { uint16_t v; std::memcpy(&v, p, 2); return v; }
void store16(uint8_t* p, uint16_t v) { std::memcpy(p, &v, 2); }
void store32(uint8_t* p, uint32_t v) { std::memcpy(p, &v, 4); }
uint32_t load32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

template <int FMT> void put_code(uint8_t* payload, int i, uint32_t c) {
    if (FMT == 0) payload[i >> 1] = (uint8_t)(payload[i >> 1] | (c << (4 * (i & 1))));
    else payload[i] = (uint8_t)c;
}
template <int FMT> uint32_t get_code(const uint8_t* payload, int i) {
    return FMT == 0 ? (payload[i >> 1] >> (4 * (i & 1))) & 0xfu : payload[i];
}

// One block of 32 bf16 -> (scale byte, 32 codes); false where the block is poisoned.
template <int FMT> bool block_scale(const uint8_t* x, int& e) {
    uint32_t a = 0;
    for (int i = 0; i < cutmx::BLOCK; ++i) {
        const uint32_t m = load16(x + 2 * i) & 0x7fffu;
        a = m > a ? m : a;
    }
    if (a >= 0x7f80u) return false;
    e = cutmx::block_exp<FMT>(a);
    return true;
}

template <int FMT> void encode(const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    const size_t n = in.size() / (2 * cutmx::SAMPLE);
    constexpr int R = cutmx::record_bytes<FMT>();
    out.assign(n * R, 0);
    for (size_t s = 0; s < n; ++s) {
        uint8_t* r = out.data() + s * R;
        store32(r, cutmx::BLOCK);
        store32(r + 4, cutmx::FMT_WORD + FMT);
        for (int k = 0; k < cutmx::BLOCKS; ++k) {
            const uint8_t* x = in.data() + 2 * (s * cutmx::SAMPLE + (size_t)k * cutmx::BLOCK);
            int e = 0;
            if (!block_scale<FMT>(x, e)) {
                r[cutmx::HEADER + k] = (uint8_t)cutmx::SCALE_NAN;
                continue;
            }
            r[cutmx::HEADER + k] = (uint8_t)(e + cutmx::BIAS);
            for (int i = 0; i < cutmx::BLOCK; ++i)
                put_code<FMT>(r + cutmx::PAYLOAD_OFF, k * cutmx::BLOCK + i, cutmx::encode_code<FMT>(load16(x + 2 * i), e));
        }
    }
}

template <int FMT> int decode(const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    constexpr int R = cutmx::record_bytes<FMT>();
    const size_t n = in.size() / R;
    out.assign(n * 2 * cutmx::SAMPLE, 0);
    int flag = 0;
    for (size_t s = 0; s < n; ++s) {
        const uint8_t* r = in.data() + s * R;
        const bool bad_head = load32(r) != (uint32_t)cutmx::BLOCK || load32(r + 4) != cutmx::FMT_WORD + FMT ||
                              load32(r + 8) != 0 || load32(r + 12) != 0;
        if (bad_head) flag = 1;
        for (int k = 0; k < cutmx::BLOCKS; ++k) {
            const uint32_t sb = r[cutmx::HEADER + k];
            const bool bad_scale = sb < (uint32_t)(cutmx::E_MIN + cutmx::BIAS);
            if (bad_scale && !bad_head) flag = 1;
            for (int i = 0; i < cutmx::BLOCK; ++i) {
                const int el = k * cutmx::BLOCK + i;
                const uint16_t v = (bad_head || bad_scale || sb == cutmx::SCALE_NAN)
                                       ? cutmx::BF16_NAN
                                       : cutmx::decode_code<FMT>(get_code<FMT>(r + cutmx::PAYLOAD_OFF, el), (int)sb - cutmx::BIAS);
                store16(out.data() + 2 * (s * cutmx::SAMPLE + el), v);
            }
        }
    }
    return flag;
}

template <int FMT> void roundtrip(const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    const size_t blocks = in.size() / (2 * cutmx::BLOCK);
    out.assign(in.size(), 0);
    for (size_t k = 0; k < blocks; ++k) {
        const uint8_t* x = in.data() + 2 * k * cutmx::BLOCK;
        int e = 0;
        const bool ok = block_scale<FMT>(x, e);
        for (int i = 0; i < cutmx::BLOCK; ++i)
            store16(out.data() + 2 * (k * cutmx::BLOCK + i),
                    ok ? cutmx::decode_code<FMT>(cutmx::encode_code<FMT>(load16(x + 2 * i), e), e) : cutmx::BF16_NAN);
    }
}

template <int FMT> int run(const std::string& mode, int argc, char** argv) {
    std::vector<uint8_t> out;
    if (mode == "exps") {
        std::vector<int16_t> e(0x7f80);
        for (uint32_t a = 0; a < 0x7f80u; ++a) e[a] = (int16_t)cutmx::block_exp<FMT>(a);
        write_all(argv[3], e.data(), e.size() * 2);
        return 0;
    }
    if (mode == "codes") {
        const int e_hi = cutmx::block_exp<FMT>(0x7f7f);
        out.resize((size_t)(e_hi - cutmx::E_MIN + 1) << 16);
        for (int e = cutmx::E_MIN; e <= e_hi; ++e)
            for (uint32_t b = 0; b < 0x10000u; ++b)
                out[((size_t)(e - cutmx::E_MIN) << 16) + b] = (b & 0x7fffu) < 0x7f80u ? (uint8_t)cutmx::encode_code<FMT>(b, e) : 0xEE;
        write_all(argv[3], out.data(), out.size());
        return 0;
    }
    if (mode == "vals") {
        constexpr int NC = 1 << cutmx::Fmt<FMT>::BITS;
        std::vector<uint16_t> v;
        for (int sb = cutmx::E_MIN + cutmx::BIAS; sb <= 254; ++sb)
            for (int c = 0; c < NC; ++c) v.push_back(cutmx::decode_code<FMT>((uint32_t)c, sb - cutmx::BIAS));
        write_all(argv[3], v.data(), v.size() * 2);
        return 0;
    }
    if (argc < 5) return 2;
    const std::vector<uint8_t> in = read_all(argv[3]);
    if (mode == "encode") encode<FMT>(in, out);
    else if (mode == "decode") std::printf("flag %d\n", decode<FMT>(in, out));
    else if (mode == "roundtrip") roundtrip<FMT>(in, out);
    else return 2;
    write_all(argv[4], out.data(), out.size());
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: cutmx_host exps|codes|vals|encode|decode|roundtrip FMT [in] out\n");
        return 2;
    }
    const std::string mode = argv[1];
    const int fmt = std::atoi(argv[2]);
    return fmt == 0 ? run<0>(mode, argc, argv) : fmt == 1 ? run<1>(mode, argc, argv) : 2;
}
