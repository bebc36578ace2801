// slk_cutmx.hip — block-scaled MX records of the K5 cut and its gradient (include/slk.h, "MX cut records").
//
// One workgroup of 256 threads owns one sample of 16,384 bf16 elements = 512 blocks of 32. Thread t owns the two
// whole blocks t and 256 + t: four 16-byte loads each, 32 elements in 16 registers, from the block's amax to its
// codes, so the amax is a register maximum — no LDS, no barrier, no shuffle (the sample-wide reduction of
// slk_cut8.hip is gone). The amax is an integer max over bits & 0x7fff (the order of non-negative floats is the order
// of their bits, and a non-finite element is any value >= 0x7f80). A block's codes are 16 (e2m1) or 32 (e4m3)
// contiguous bytes: one or two 16-byte stores by the block's thread. The scale bytes of four neighbouring lanes are
// gathered into one word by lane shuffles and stored by the first of the four; the decoder loads 16 scale bytes in
// every sixteenth lane and hands them out the same way. Every output byte is written by exactly one thread, the
// record's header included (one vector store by thread 0); no atomics, no scratch.
//
// Conversions: e2m1 through gfx950's v_cvt_scalef32_pk_fp4_f32 / v_cvt_scalef32_pk_f32_fp4 with the scale operand
// held at 1.0 — the kernel forms the exact float32 product x * 2^-e itself and applies 2^e in integers
// (cut8::scaled_bf16), so the instructions' own scaling, saturation and overflow never come into play; e4m3 through
// v_cvt_pk_fp8_f32 / v_cvt_f32_fp8, exactly the conversions of slk_cut8.hip's format 0. -DSLK_CUTMX_HWCVT=0 builds the
// integer arithmetic of slk_cutmx.h instead, and tools/cutmx_cvt_check.py compares the two builds bit for bit.
#include "slk_common.h"
#include "slk_cutmx.h"

#ifndef SLK_CUTMX_HWCVT
#define SLK_CUTMX_HWCVT 1
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {
constexpr int THREADS = 256;
constexpr int PER_THREAD = cutmx::BLOCKS / THREADS;   // 2 blocks per thread: t and 256 + t

struct Block {
    u32x4 v[4];   // 32 bf16, element 2i in the low half of word i
};

__device__ __forceinline__ int block_of(int j) { return j * THREADS + (int)threadIdx.x; }

__device__ __forceinline__ void load_block(const uint16_t* __restrict__ x, int k, Block& b) {
    const u32x4* p = reinterpret_cast<const u32x4*>(x + (size_t)k * cutmx::BLOCK);
#pragma unroll
    for (int i = 0; i < 4; ++i) b.v[i] = p[i];
}

__device__ __forceinline__ void store_block(uint16_t* __restrict__ out, int k, const Block& b) {
    u32x4* p = reinterpret_cast<u32x4*>(out + (size_t)k * cutmx::BLOCK);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = b.v[i];
}

__device__ __forceinline__ void nan_block(Block& b) {
    const uint32_t n2 = cutmx::BF16_NAN | ((uint32_t)cutmx::BF16_NAN << 16);
    const u32x4 nan = {n2, n2, n2, n2};
#pragma unroll
    for (int i = 0; i < 4; ++i) b.v[i] = nan;
}

// max (bits & 0x7fff) over the block.
__device__ __forceinline__ uint32_t amax_bits(const Block& b) {
    uint32_t a = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = b.v[i][k] & 0x7fff7fffu;
            a = max(a, max(w & 0xffffu, w >> 16));
        }
    }
    return a;
}

// The float32 of x * 2^-e for the two bf16 of a word: exact products of a bf16 value and a power of two in
// [2^-127, 2^100], at most F_MAX in magnitude (one below float32's normal range is far below a quarter of either
// format's smallest value: it converts to a zero of its sign whether or not it is kept as a subnormal).
__device__ __forceinline__ void scaled_pair(uint32_t w, float s, float& lo, float& hi) {
    lo = __uint_as_float(w << 16) * s;
    hi = __uint_as_float(w & 0xffff0000u) * s;
}

// 2^-e as a float32 multiplier. e <= 127 - 2 + 1 = 126 keeps the exponent field positive.
__device__ __forceinline__ float inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

// The codes of a block under exponent e. e2m1: c[0] holds the 32 nibbles, element 2i in bits 0..3 of byte i;
// e4m3: c[0], c[1] hold one byte per element.
template <int FMT> struct Codes { u32x4 c[FMT == 0 ? 1 : 2]; };

__device__ __forceinline__ void encode_block(const Block& b, int e, Codes<0>& out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // output word i: elements 8 i .. 8 i + 7, the pair words b.v[i][0..3]
#if SLK_CUTMX_HWCVT
        const float s = inv_scale(e);
        uint32_t w = 0;
        float lo, hi;
        scaled_pair(b.v[i][0], s, lo, hi);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, lo, hi, 1.0f, 0);
        scaled_pair(b.v[i][1], s, lo, hi);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, lo, hi, 1.0f, 1);
        scaled_pair(b.v[i][2], s, lo, hi);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, lo, hi, 1.0f, 2);
        scaled_pair(b.v[i][3], s, lo, hi);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, lo, hi, 1.0f, 3);
        out.c[0][i] = w;
#else
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = b.v[i][k];
            w |= (cutmx::encode_code<0>(p & 0xffffu, e) | (cutmx::encode_code<0>(p >> 16, e) << 4)) << (8 * k);
        }
        out.c[0][i] = w;
#endif
    }
}

__device__ __forceinline__ void encode_block(const Block& b, int e, Codes<1>& out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // output word i: elements 4 i .. 4 i + 3, the pair words 2 i and 2 i + 1
        const uint32_t p0 = b.v[i >> 1][2 * (i & 1)], p1 = b.v[i >> 1][2 * (i & 1) + 1];
#if SLK_CUTMX_HWCVT
        const float s = inv_scale(e);
        float f0, f1, f2, f3;
        scaled_pair(p0, s, f0, f1);
        scaled_pair(p1, s, f2, f3);
        const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
        out.c[i >> 2][i & 3] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, lo, true);
#else
        out.c[i >> 2][i & 3] = cutmx::encode_code<1>(p0 & 0xffffu, e) | (cutmx::encode_code<1>(p0 >> 16, e) << 8) |
                               (cutmx::encode_code<1>(p1 & 0xffffu, e) << 16) | (cutmx::encode_code<1>(p1 >> 16, e) << 24);
#endif
    }
}

// The float32 bits of the values of the two e2m1 codes in byte K of a word (low nibble first).
template <int K> __device__ __forceinline__ void fp4_pair_bits(uint32_t word, uint32_t& lo, uint32_t& hi) {
#if SLK_CUTMX_HWCVT
    const f32x2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, K);
    lo = __float_as_uint(v[0]);
    hi = __float_as_uint(v[1]);
#else
    lo = cutmx::code_bits<0>((word >> (8 * K)) & 0xfu);
    hi = cutmx::code_bits<0>((word >> (8 * K + 4)) & 0xfu);
#endif
}

template <int K> __device__ __forceinline__ uint32_t fp8_bits(uint32_t word) {
#if SLK_CUTMX_HWCVT
    return __float_as_uint(__builtin_amdgcn_cvt_f32_fp8((int)word, K));
#else
    return cutmx::code_bits<1>((word >> (8 * K)) & 0xffu);
#endif
}

__device__ __forceinline__ uint32_t bf16_pair(uint32_t lo, uint32_t hi, int e) {
    return (uint32_t)cut8::scaled_bf16(lo, e) | ((uint32_t)cut8::scaled_bf16(hi, e) << 16);
}

__device__ __forceinline__ void decode_block(const Codes<0>& in, int e, Block& b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = in.c[0][i];
        uint32_t lo, hi;
        fp4_pair_bits<0>(w, lo, hi);
        b.v[i][0] = bf16_pair(lo, hi, e);
        fp4_pair_bits<1>(w, lo, hi);
        b.v[i][1] = bf16_pair(lo, hi, e);
        fp4_pair_bits<2>(w, lo, hi);
        b.v[i][2] = bf16_pair(lo, hi, e);
        fp4_pair_bits<3>(w, lo, hi);
        b.v[i][3] = bf16_pair(lo, hi, e);
    }
}

__device__ __forceinline__ void decode_block(const Codes<1>& in, int e, Block& b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t w = in.c[i >> 2][i & 3];
        b.v[i >> 1][2 * (i & 1)] = bf16_pair(fp8_bits<0>(w), fp8_bits<1>(w), e);
        b.v[i >> 1][2 * (i & 1) + 1] = bf16_pair(fp8_bits<2>(w), fp8_bits<3>(w), e);
    }
}

template <int FMT> __device__ __forceinline__ uint8_t* payload_of(uint8_t* r, int k) {
    return r + cutmx::PAYLOAD_OFF + (size_t)k * (cutmx::BLOCK * cutmx::Fmt<FMT>::BITS / 8);
}

template <int FMT>
__global__ __launch_bounds__(THREADS) void cutmx_encode_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ rec) {
    const uint16_t* xs = x + (size_t)blockIdx.x * cutmx::SAMPLE;
    uint8_t* r = rec + (size_t)blockIdx.x * cutmx::record_bytes<FMT>();
    Block b[PER_THREAD];
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) load_block(xs, block_of(j), b[j]);
    if (threadIdx.x == 0) {
        const u32x4 head = {(uint32_t)cutmx::BLOCK, cutmx::FMT_WORD + (uint32_t)FMT, 0u, 0u};
        *reinterpret_cast<u32x4*>(r) = head;
    }
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const uint32_t a = amax_bits(b[j]);
        const bool poison = a >= 0x7f80u;
        const int e = poison ? 0 : cutmx::block_exp<FMT>(a);
        const uint32_t sb = poison ? cutmx::SCALE_NAN : (uint32_t)(e + cutmx::BIAS);
        // four lanes' scale bytes -> one word, stored by the first of the four (all 64 lanes are active)
        const uint32_t w = sb | ((uint32_t)__shfl_down((int)sb, 1, 64) << 8) | ((uint32_t)__shfl_down((int)sb, 2, 64) << 16) |
                           ((uint32_t)__shfl_down((int)sb, 3, 64) << 24);
        if ((threadIdx.x & 3u) == 0) *reinterpret_cast<uint32_t*>(r + cutmx::HEADER + block_of(j)) = w;
        Codes<FMT> c;
        encode_block(b[j], e, c);
        u32x4* p = reinterpret_cast<u32x4*>(payload_of<FMT>(r, block_of(j)));
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < (FMT == 0 ? 1 : 2); ++i) p[i] = poison ? zero : c.c[i];
    }
}

template <int FMT>
__global__ __launch_bounds__(THREADS) void cutmx_decode_kernel(const uint8_t* __restrict__ rec, uint16_t* __restrict__ out,
                                                               int* __restrict__ err_flag) {
    const uint8_t* r = rec + (size_t)blockIdx.x * cutmx::record_bytes<FMT>();
    uint16_t* o = out + (size_t)blockIdx.x * cutmx::SAMPLE;
    const u32x4 head = *reinterpret_cast<const u32x4*>(r);
    const bool bad_head = head[0] != (uint32_t)cutmx::BLOCK || head[1] != cutmx::FMT_WORD + (uint32_t)FMT ||
                          (head[2] | head[3]) != 0u;
    if (bad_head && threadIdx.x == 0) err_flag[0] = 1;   // uniform over the workgroup: every block becomes NaNs below
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        // every sixteenth lane loads the 16 scale bytes of its 16 lanes; the others take their byte from it
        u32x4 s16 = {0u, 0u, 0u, 0u};
        if ((threadIdx.x & 15u) == 0) s16 = *reinterpret_cast<const u32x4*>(r + cutmx::HEADER + block_of(j));
        const int src = (int)(threadIdx.x & 63u & ~15u), q = (int)((threadIdx.x >> 2) & 3u);
        const uint32_t w0 = (uint32_t)__shfl((int)s16[0], src, 64), w1 = (uint32_t)__shfl((int)s16[1], src, 64);
        const uint32_t w2 = (uint32_t)__shfl((int)s16[2], src, 64), w3 = (uint32_t)__shfl((int)s16[3], src, 64);
        const uint32_t word = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
        const uint32_t sb = (word >> (8 * (threadIdx.x & 3u))) & 0xffu;
        Codes<FMT> c;
        const u32x4* p = reinterpret_cast<const u32x4*>(payload_of<FMT>(const_cast<uint8_t*>(r), block_of(j)));
#pragma unroll
        for (int i = 0; i < (FMT == 0 ? 1 : 2); ++i) c.c[i] = p[i];
        const bool bad_scale = sb < (uint32_t)(cutmx::E_MIN + cutmx::BIAS);
        Block b;
        if (bad_head || bad_scale || sb == cutmx::SCALE_NAN) {
            if (bad_scale && !bad_head) err_flag[0] = 1;
            nan_block(b);
        } else {
            decode_block(c, (int)sb - cutmx::BIAS, b);
        }
        store_block(o, block_of(j), b);
    }
}

// decode(encode(x)) without the record; x and out are not __restrict__: they may be the same buffer (a thread reads
// both of its blocks before its first store, and no other thread touches them).
template <int FMT>
__global__ __launch_bounds__(THREADS) void cutmx_roundtrip_kernel(const uint16_t* x, uint16_t* out) {
    const uint16_t* xs = x + (size_t)blockIdx.x * cutmx::SAMPLE;
    uint16_t* o = out + (size_t)blockIdx.x * cutmx::SAMPLE;
    Block b[PER_THREAD];
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) load_block(xs, block_of(j), b[j]);
    Block d[PER_THREAD];
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const uint32_t a = amax_bits(b[j]);
        if (a >= 0x7f80u) {
            nan_block(d[j]);
        } else {
            const int e = cutmx::block_exp<FMT>(a);
            Codes<FMT> c;
            encode_block(b[j], e, c);
            decode_block(c, e, d[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) store_block(o, block_of(j), d[j]);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace

extern "C" int64_t slk_cutmx_record_bytes(int fmt) {
    return fmt == 0 ? cutmx::record_bytes<0>() : fmt == 1 ? cutmx::record_bytes<1>() : -1;
}

extern "C" int slk_cutmx_encode(const void* x_bf16, int n, int fmt, void* rec, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && rec && aligned16(x_bf16) && aligned16(rec));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint8_t* r = static_cast<uint8_t*>(rec);
    if (fmt == 0) cutmx_encode_kernel<0><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r);
    else cutmx_encode_kernel<1><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r);
    return slk_launch_status();
}

extern "C" int slk_cutmx_decode(const void* rec, int n, int fmt, void* out_bf16, int* err_flag, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(rec && out_bf16 && err_flag && aligned16(rec) && aligned16(out_bf16));
    SLK_CHECK_ARG((reinterpret_cast<uintptr_t>(err_flag) & 3u) == 0);
    const uint8_t* r = static_cast<const uint8_t*>(rec);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    if (fmt == 0) cutmx_decode_kernel<0><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(r, o, err_flag);
    else cutmx_decode_kernel<1><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(r, o, err_flag);
    return slk_launch_status();
}

extern "C" int slk_cutmx_roundtrip(const void* x_bf16, int n, int fmt, void* out_bf16, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && aligned16(x_bf16) && aligned16(out_bf16));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    if (fmt == 0) cutmx_roundtrip_kernel<0><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o);
    else cutmx_roundtrip_kernel<1><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o);
    return slk_launch_status();
}
