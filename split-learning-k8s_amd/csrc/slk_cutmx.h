// slk_cutmx.h — the element arithmetic of the MX cut codec (include/slk.h, "MX cut records"), in integer arithmetic
// in plain C++ so that the same functions compile for the host: tests/cutmx_host.cc is a host build of this header,
// held to tests/cutmx_ref.py over every finite bf16 value at every block exponent that can meet it. It reuses
// slk_cut8.h's encode_one / decode_bits / scaled_bf16, which are written over (M, EMIN) and carry over to e2m1 through
// one more Fmt; nothing of that header changes. The kernels convert e2m1 with gfx950's v_cvt_scalef32_pk_fp4_f32 /
// v_cvt_scalef32_pk_f32_fp4 and e4m3 with the FP8 records' v_cvt_pk_fp8_f32 / v_cvt_f32_fp8 by default
// (SLK_CUTMX_HWCVT in slk_cutmx.hip) and keep block_exp and scaled_bf16 from here; -DSLK_CUTMX_HWCVT=0 runs
// encode_code / code_bits instead, and tools/cutmx_cvt_check.py holds the two builds to the same bits. Internal; not
// part of the ABI.
#pragma once

#include "slk_cut8.h"

namespace cut8 {
// OCP e2m1 under cut8's conventions: one mantissa bit, smallest normal 2^0. encode_one<2> / decode_bits<2> keep the
// sign in bit 7 and the magnitude code (exp << 1 | man) in bits 0..2; cutmx::encode_code / code_bits move the sign.
template <> struct Fmt<2> { static constexpr int M = 1, EMIN = 0, K = 2; };
}  // namespace cut8

namespace cutmx {
constexpr int SAMPLE = cut8::SAMPLE;     // 16384 bf16 elements
constexpr int BLOCK = 32;                // elements under one scale
constexpr int BLOCKS = SAMPLE / BLOCK;   // 512 scale bytes
constexpr int HEADER = 16;
constexpr int PAYLOAD_OFF = HEADER + BLOCKS;   // 528 = 16 x 33
constexpr int E_MIN = cut8::E_MIN;       // -100: scale byte 27
constexpr int BIAS = 127;
constexpr uint32_t SCALE_NAN = 0xFFu;    // E8M0's NaN: a poisoned block
constexpr uint32_t FMT_WORD = 0x10u;     // header word 1 = FMT_WORD + fmt
constexpr uint16_t BF16_NAN = cut8::BF16_NAN;

// fmt 0 = e2m1 (4-bit codes, F_MAX 6 = 1.5 * 2^2), fmt 1 = e4m3 (the FP8 records' format 0, F_MAX 448 = 1.75 * 2^8).
template <int FMT> struct Fmt;
template <> struct Fmt<0> { static constexpr int C8 = 2, BITS = 4, TOP = 0x40; };
template <> struct Fmt<1> { static constexpr int C8 = 0, BITS = 8, TOP = 0x60; };
template <int FMT> constexpr int payload_bytes() { return SAMPLE * Fmt<FMT>::BITS / 8; }
template <int FMT> constexpr int record_bytes() { return PAYLOAD_OFF + payload_bytes<FMT>(); }   // 8720 / 16912

// The block's exponent from a = max (bits & 0x7fff) of a block without non-finite elements (a < 0x7f80): the
// smallest e with amax * 2^-e <= F_MAX, clamped below at E_MIN; 0 for an all-zero block. F_MAX = (1 + TOP / 128) *
// 2^K and amax = (1 + man / 128) * 2^(ex - 127), so e = ex - 127 - K, one more where man > TOP; a subnormal amax is
// below 2^-126, where the clamp binds.
template <int FMT> SLK_CUT8_FN int block_exp(uint32_t a) {
    if (a == 0) return 0;
    const int ex = (int)(a >> 7), man = (int)(a & 0x7f);
    if (ex == 0) return E_MIN;
    const int e = ex - 127 - cut8::Fmt<Fmt<FMT>::C8>::K + (man > Fmt<FMT>::TOP ? 1 : 0);
    return e < E_MIN ? E_MIN : e;
}

// The code of x * 2^-e, x a finite bf16 (its 16 bits) with |x| * 2^-e <= F_MAX: round to nearest even, a zero keeps
// the sign of x. e2m1: sign << 3 | exp << 1 | man.
template <int FMT> SLK_CUT8_FN uint32_t encode_code(uint32_t b, int e) {
    const uint32_t c = cut8::encode_one<Fmt<FMT>::C8>(b, e);
    return FMT == 0 ? ((c >> 4) & 0x8u) | (c & 0x7u) : c;
}

// code -> the float32 bits of its value (exact; an e4m3 NaN code gives a float32 NaN).
template <int FMT> SLK_CUT8_FN uint32_t code_bits(uint32_t c) {
    return cut8::decode_bits<Fmt<FMT>::C8>(FMT == 0 ? ((c & 0x8u) << 4) | (c & 0x7u) : c);
}

// value(code) * 2^e as bf16, e in [E_MIN, 127]: exact, except that a finite product at or past 2^128 is the largest
// finite bf16 of its sign (cut8::scaled_bf16).
template <int FMT> SLK_CUT8_FN uint16_t decode_code(uint32_t c, int e) { return cut8::scaled_bf16(code_bits<FMT>(c), e); }
}  // namespace cutmx
