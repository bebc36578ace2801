// slk_cut8.h — the element arithmetic of the FP8 cut codec (include/slk.h, "FP8 cut records"), in integer
// arithmetic in plain C++ so that the same functions compile for the host: a host build of this header is what
// was checked against torch's float8 casts, over every finite bf16 value at every scale exponent that can meet it.
// The kernels convert with gfx950's own instructions by default (SLK_CUT8_HWCVT in slk_cut8.hip) and keep
// scale_exp and scaled_bf16 from here; a build with -DSLK_CUT8_HWCVT=0 runs encode_one / decode_bits instead, and
// tools/cut8_cvt_check.py holds the two builds to the same bits. Internal; not part of the ABI.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SLK_CUT8_FN __host__ __device__ __forceinline__
#else
#define SLK_CUT8_FN static inline
#endif

namespace cut8 {
constexpr int SAMPLE = 16384;            // bf16 elements of one K5 cut (or cut-gradient row)
constexpr int HEADER = 16;               // bytes in front of the payload
constexpr int RECORD = HEADER + SAMPLE;  // 16400 = 16 x 1025
constexpr int E_MIN = -100, E_MAX = 127;
constexpr int32_t POISON = 0x7FFFFFFF;
constexpr uint16_t BF16_NAN = 0x7FC0;

// A format: mantissa bits, exponent of the smallest normal, and K with F_MAX = 1.75 * 2^K.
template <int FMT> struct Fmt;
template <> struct Fmt<0> { static constexpr int M = 3, EMIN = -6, K = 8; };    // e4m3fn, F_MAX 448
template <> struct Fmt<1> { static constexpr int M = 2, EMIN = -14, K = 15; };  // e5m2,   F_MAX 57344

// The record's exponent from a = max (bits & 0x7fff) of a sample without non-finite elements (a < 0x7f80):
// the smallest e with amax * 2^-e <= 1.75 * 2^K, clamped below at E_MIN; 0 for an all-zero sample. amax =
// (1 + man / 128) * 2^(ex - 127) is at most 1.75 * 2^(ex - 127) exactly when man <= 0x60; a subnormal amax
// (ex == 0) is below 2^-126, where the clamp binds for both formats.
template <int FMT> SLK_CUT8_FN int32_t scale_exp(uint32_t a) {
    if (a == 0) return 0;
    const int ex = (int)(a >> 7), man = (int)(a & 0x7f);
    if (ex == 0) return E_MIN;
    const int e = ex - 127 - Fmt<FMT>::K + (man > 0x60 ? 1 : 0);
    return e < E_MIN ? E_MIN : e;
}

// The fp8 code of x * 2^-e, x a finite bf16 (its 16 bits) with |x| * 2^-e <= F_MAX: round to nearest even.
// x = sig * 2^q0 with an integer sig < 256, so y = sig * 2^q; with p = floor(log2 y) the target's quantum is
// 2^(max(p, EMIN) - M), and the code is the rounded multiple of it with the exponent field added on — a carry
// out of the mantissa lands in the exponent field by the addition itself, and a subnormal that rounds up to
// 2^M is the smallest normal. Nothing saturates: F_MAX is representable and rounding is monotonic.
template <int FMT> SLK_CUT8_FN uint32_t encode_one(uint32_t b, int e) {
    constexpr int M = Fmt<FMT>::M, EMIN = Fmt<FMT>::EMIN;
    const uint32_t sign = (b >> 8) & 0x80u;
    const int ex = (int)((b >> 7) & 0xffu);
    const uint32_t sig = (b & 0x7fu) | (ex ? 0x80u : 0u);
    if (sig == 0) return sign;
    const int q = (ex ? ex : 1) - 134 - e;
    const int p = (31 - __builtin_clz(sig)) + q;
    const int pe = p > EMIN ? p : EMIN;
    const int s = pe - M - q;   // the quantum is 2^s units of sig; s >= -M
    uint32_t r;
    if (s <= 0) {
        r = sig << -s;
    } else if (s > 9) {
        r = 0;                  // sig * 2^-s < 1/4
    } else {
        r = (sig + (1u << (s - 1)) - 1u + ((sig >> s) & 1u)) >> s;
    }
    return sign | (r + ((uint32_t)(pe - EMIN) << M));
}

// ---- stochastic rounding (include/slk.h, "FP8 cut records: stochastic rounding"). These functions are the
// specification: the kernels' default build converts with v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32, whose mapping from the
// random word to the rounding direction sr_up restates (measured: tools/cut8_sr_check.py), and a -DSLK_CUT8_HWCVT=0
// build runs encode_one_sr itself.
SLK_CUT8_FN uint32_t hash32(uint32_t x) {   // lowbias32 (slk_common.h), here for the host as well
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// The key of one sample: g its global row, t the step counter's value, all uint32.
SLK_CUT8_FN uint32_t sr_base(uint32_t g, uint32_t t, uint32_t seed, int fmt) {
    return hash32(g * 0x9E3779B1u + t * 0x85EBCA77u + seed * 0xC2B2AE3Du + (uint32_t)(fmt + 1) * 0x27D4EB2Fu);
}
// The random word of element i.
SLK_CUT8_FN uint32_t sr_word(uint32_t base, uint32_t i) { return hash32(base + i * 0x9E3779B1u); }

// Whether sig = (k << s) + rem, 0 <= rem < 2^s, s >= 1, goes to k + 1: the instruction's rule. It keeps float32's
// 23 fraction bits, of which the target has M, so NB = 23 - M bits are discarded in the normal range; it adds the top
// NB bits of r to them and rounds up on the carry. In the subnormal range it first shifts the fraction right,
// dropping what falls off the end, so T below is rem's 2^-s scaled to NB bits, floored where s > NB. For s <= NB
// exactly rem * 2^(NB - s) of the 2^NB values of r >> (32 - NB) carry: P(up) = rem / 2^s, and rem = 0 never does.
template <int FMT> SLK_CUT8_FN uint32_t sr_up(uint32_t rem, int s, uint32_t r) {
    constexpr int NB = 23 - Fmt<FMT>::M;   // 20 (e4m3), 21 (e5m2)
    const uint32_t T = s <= NB ? rem << (NB - s) : (s - NB < 8 ? rem >> (s - NB) : 0u);   // rem < 2^8
    return ((r >> (32 - NB)) + T) >> NB;
}

// encode_one with stochastic rounding under the random word r: one of the two neighbouring codes of x * 2^-e, the
// lower one in magnitude (truncation) plus sr_up. A representable value (s <= 0, or rem == 0) is its own code for
// every r; the upper neighbour of the largest value below F_MAX is F_MAX itself, so nothing saturates.
template <int FMT> SLK_CUT8_FN uint32_t encode_one_sr(uint32_t b, int e, uint32_t r) {
    constexpr int M = Fmt<FMT>::M, EMIN = Fmt<FMT>::EMIN;
    const uint32_t sign = (b >> 8) & 0x80u;
    const int ex = (int)((b >> 7) & 0xffu);
    const uint32_t sig = (b & 0x7fu) | (ex ? 0x80u : 0u);
    if (sig == 0) return sign;
    const int q = (ex ? ex : 1) - 134 - e;
    const int p = (31 - __builtin_clz(sig)) + q;
    const int pe = p > EMIN ? p : EMIN;
    const int s = pe - M - q;
    uint32_t c;
    if (s <= 0) {
        c = sig << -s;
    } else {
        const uint32_t k = s < 8 ? sig >> s : 0u;   // sig < 2^8
        c = k + sr_up<FMT>(sig - (s < 8 ? k << s : 0u), s, r);
    }
    return sign | (c + ((uint32_t)(pe - EMIN) << M));
}

// fp8 code -> float32 bits (exact; NaN and inf codes become a float32 NaN / inf of the code's sign).
template <int FMT> SLK_CUT8_FN uint32_t decode_bits(uint32_t c) {
    constexpr int M = Fmt<FMT>::M, EMIN = Fmt<FMT>::EMIN;
    const uint32_t sign = (c & 0x80u) << 24, u = c & 0x7fu;
    const uint32_t ef = u >> M, man = u & ((1u << M) - 1u);
    if (FMT == 0 ? u == 0x7fu : ef == 31u) return sign | (FMT == 1 && man == 0 ? 0x7f800000u : 0x7fc00000u);
    if (ef == 0) {
        // man * 2^(EMIN - M): man in [0, 2^M), normalised by hand
        if (man == 0) return sign;
        const int h = 31 - __builtin_clz(man);
        return sign | ((uint32_t)(127 + EMIN - M + h) << 23) | ((man << (23 - h)) & 0x7fffffu);
    }
    return sign | ((ef + (uint32_t)(126 + EMIN)) << 23) | (man << (23 - M));
}

// The bf16 of f * 2^e, f the float32 bits of a code's value and e in [E_MIN, E_MAX]: the product has at most four
// significant bits and is a normal float32 (or 0, inf, NaN), so adding e to the exponent field and keeping the upper
// 16 bits is the exact product. A NaN is written as 0x7FC0, whatever its sign and payload. A finite code never
// becomes inf: a product at or past 2^128 — the rounded amax of a sample whose amax lies above F_MAX / 2 * 2^e in
// bf16's top binade, e.g. 255 * 2^120 -> code 256 -> 2^128 — is the largest finite bf16 of its sign, which is
// nearer to x than the bound asks and keeps decode(encode(.)) idempotent.
SLK_CUT8_FN uint16_t scaled_bf16(uint32_t f, int e) {
    const uint32_t sign = (f >> 16) & 0x8000u;
    const int ef = (int)((f >> 23) & 0xffu);
    if (ef == 0) return (uint16_t)sign;   // a code's value is never a float32 subnormal
    if (ef == 255) return (uint16_t)((f & 0x7fffffu) ? BF16_NAN : (sign | 0x7f80u));
    const int ne = ef + e;   // >= 127 - 16 - 100 > 0
    if (ne >= 255) return (uint16_t)(sign | 0x7f7fu);
    return (uint16_t)(((f & 0x807fffffu) | ((uint32_t)ne << 23)) >> 16);
}

template <int FMT> SLK_CUT8_FN uint16_t decode_one(uint32_t c, int e) { return scaled_bf16(decode_bits<FMT>(c), e); }
}  // namespace cut8
