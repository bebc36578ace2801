// slk_cut8.hip — FP8 records of the K5 cut and its gradient (include/slk.h, "FP8 cut records").
//
// One block of 256 threads owns one sample of 16,384 bf16 elements and reads it once: thread t holds elements
// [16 (256 j + t), +16) for j = 0..3 — two 16-byte loads each, 64 elements in 32 registers — from the amax
// reduction to the conversion. The amax is an integer max over bits & 0x7fff (the order of non-negative floats
// is the order of their bits, and a non-finite element is any value >= 0x7f80): inside the wave by shuffles,
// across the four waves through 16 bytes of LDS. Every output byte is written by exactly one thread with a
// 16-byte store, the record's header included (one vector store by thread 0); no atomics.
//
// The conversions are gfx950's v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 (OCP e4m3fn / e5m2, round to nearest even) on the
// exact float32 product x * 2^-e, and v_cvt_f32_fp8 / v_cvt_f32_bf8 back; -DSLK_CUT8_HWCVT=0 builds the integer
// arithmetic of slk_cut8.h instead — the form that compiles for the host, where it was checked against torch's
// float8 casts — and tools/cut8_cvt_check.py compares the two builds bit for bit.
//
// The _sr entries run the same per-sample skeleton with another rounding (the Round parameter below): each element
// goes to one of its two neighbouring codes under a random word keyed on (seed, *step, global row, element) —
// v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32, or cut8::encode_one_sr, which restates them, with -DSLK_CUT8_HWCVT=0
// (tools/cut8_sr_check.py compares the two builds and the instruction's rule).
#include "slk_common.h"
#include "slk_cut8.h"

#ifndef SLK_CUT8_HWCVT
#define SLK_CUT8_HWCVT 1
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int THREADS = 256;
constexpr int CHUNKS = cut8::SAMPLE / (16 * THREADS);  // 4 chunks of 16 elements per thread

struct Sample {
    u32x4 v[2 * CHUNKS];  // chunk j: v[2j], v[2j + 1] — 16 bf16, element 2i in the low half of word i
};

__device__ __forceinline__ size_t chunk_elem(int j) { return 16 * ((size_t)j * THREADS + threadIdx.x); }

__device__ __forceinline__ void load_sample(const uint16_t* __restrict__ x, Sample& s) {
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const u32x4* p = reinterpret_cast<const u32x4*>(x + chunk_elem(j));
        s.v[2 * j] = p[0];
        s.v[2 * j + 1] = p[1];
    }
}

// max (bits & 0x7fff) over the block's sample, the same value in every thread (one barrier).
__device__ __forceinline__ uint32_t block_amax_bits(const Sample& s, uint32_t* red) {
    uint32_t a = 0;
#pragma unroll
    for (int i = 0; i < 2 * CHUNKS; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = s.v[i][k] & 0x7fff7fffu;
            a = max(a, max(w & 0xffffu, w >> 16));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return max(max(red[0], red[1]), max(red[2], red[3]));
}

// Four elements (two words of bf16 pairs) -> four fp8 codes of x * 2^-e, byte i the code of element i.
template <int FMT>
__device__ __forceinline__ uint32_t encode4(uint32_t a, uint32_t b, int e) {
#if SLK_CUT8_HWCVT
    // the products are exact: a bf16 value times a power of two in [2^-120, 2^100], at most F_MAX in magnitude
    // (a result below float32's normal range is far below half of either format's smallest value: it converts to
    // a zero of its sign whether or not it is kept as a subnormal)
    const float s = __uint_as_float((uint32_t)(127 - e) << 23);
    const float f0 = __uint_as_float(a << 16) * s, f1 = __uint_as_float(a & 0xffff0000u) * s;
    const float f2 = __uint_as_float(b << 16) * s, f3 = __uint_as_float(b & 0xffff0000u) * s;
    if (FMT == 0) {
        const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
        return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, lo, true);
    }
    const int lo = __builtin_amdgcn_cvt_pk_bf8_f32(f0, f1, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(f2, f3, lo, true);
#else
    return cut8::encode_one<FMT>(a & 0xffffu, e) | (cut8::encode_one<FMT>(a >> 16, e) << 8) |
           (cut8::encode_one<FMT>(b & 0xffffu, e) << 16) | (cut8::encode_one<FMT>(b >> 16, e) << 24);
#endif
}

// The float32 bits of the value of code K (0..3) of a word of four codes.
template <int FMT, int K>
__device__ __forceinline__ uint32_t code_bits(uint32_t word) {
#if SLK_CUT8_HWCVT
    return __float_as_uint(FMT == 0 ? __builtin_amdgcn_cvt_f32_fp8((int)word, K) : __builtin_amdgcn_cvt_f32_bf8((int)word, K));
#else
    return cut8::decode_bits<FMT>((word >> (8 * K)) & 0xffu);
#endif
}

// encode4 under stochastic rounding: element k of the four has the random word rnd[k].
template <int FMT>
__device__ __forceinline__ uint32_t encode4_sr(uint32_t a, uint32_t b, int e, const uint32_t (&rnd)[4]) {
#if SLK_CUT8_HWCVT
    const float s = __uint_as_float((uint32_t)(127 - e) << 23);   // exact products, as in encode4
    const float f0 = __uint_as_float(a << 16) * s, f1 = __uint_as_float(a & 0xffff0000u) * s;
    const float f2 = __uint_as_float(b << 16) * s, f3 = __uint_as_float(b & 0xffff0000u) * s;
    int w = 0;
    if (FMT == 0) {
        w = __builtin_amdgcn_cvt_sr_fp8_f32(f0, rnd[0], w, 0);
        w = __builtin_amdgcn_cvt_sr_fp8_f32(f1, rnd[1], w, 1);
        w = __builtin_amdgcn_cvt_sr_fp8_f32(f2, rnd[2], w, 2);
        return (uint32_t)__builtin_amdgcn_cvt_sr_fp8_f32(f3, rnd[3], w, 3);
    }
    w = __builtin_amdgcn_cvt_sr_bf8_f32(f0, rnd[0], w, 0);
    w = __builtin_amdgcn_cvt_sr_bf8_f32(f1, rnd[1], w, 1);
    w = __builtin_amdgcn_cvt_sr_bf8_f32(f2, rnd[2], w, 2);
    return (uint32_t)__builtin_amdgcn_cvt_sr_bf8_f32(f3, rnd[3], w, 3);
#else
    return cut8::encode_one_sr<FMT>(a & 0xffffu, e, rnd[0]) | (cut8::encode_one_sr<FMT>(a >> 16, e, rnd[1]) << 8) |
           (cut8::encode_one_sr<FMT>(b & 0xffffu, e, rnd[2]) << 16) | (cut8::encode_one_sr<FMT>(b >> 16, e, rnd[3]) << 24);
#endif
}

// The rounding of a launch: four elements starting at element `i` of the sample -> four codes.
struct Nearest {
    template <int FMT> __device__ __forceinline__ uint32_t encode4(uint32_t a, uint32_t b, int e, uint32_t) const {
        return ::encode4<FMT>(a, b, e);
    }
};
struct Stochastic {
    uint32_t base;   // cut8::sr_base of the block's sample
    template <int FMT> __device__ __forceinline__ uint32_t encode4(uint32_t a, uint32_t b, int e, uint32_t i) const {
        const uint32_t rnd[4] = {cut8::sr_word(base, i), cut8::sr_word(base, i + 1), cut8::sr_word(base, i + 2),
                                 cut8::sr_word(base, i + 3)};
        return encode4_sr<FMT>(a, b, e, rnd);
    }
};
// The block's rounding from the kernel's trailing arguments: none (Nearest), or (seed, step, row0) — step a device
// int32 the kernel reads and never writes, row0 the global row of the launch's first sample.
template <int FMT, class Round> __device__ __forceinline__ Round block_round() { return Round{}; }
template <int FMT, class Round> __device__ __forceinline__ Round block_round(uint32_t seed, const int* step, int row0) {
    return Round{cut8::sr_base((uint32_t)row0 + blockIdx.x, (uint32_t)*step, seed, FMT)};
}

// 16 elements (two vectors of bf16) starting at element i of the sample -> 16 fp8 codes, byte k the code of i + k.
template <int FMT, class Round>
__device__ __forceinline__ u32x4 encode16(const u32x4& lo, const u32x4& hi, int e, const Round& round, uint32_t i) {
    u32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const u32x4& src = w < 2 ? lo : hi;
        out[w] = round.template encode4<FMT>(src[2 * (w & 1)], src[2 * (w & 1) + 1], e, i + 4 * w);
    }
    return out;
}

// 16 fp8 codes -> 16 bf16 under exponent e.
template <int FMT>
__device__ __forceinline__ void decode16(const u32x4& c, int e, u32x4& lo, u32x4& hi) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t d0 = cut8::scaled_bf16(code_bits<FMT, 0>(c[w]), e), d1 = cut8::scaled_bf16(code_bits<FMT, 1>(c[w]), e);
        const uint32_t d2 = cut8::scaled_bf16(code_bits<FMT, 2>(c[w]), e), d3 = cut8::scaled_bf16(code_bits<FMT, 3>(c[w]), e);
        u32x4& dst = w < 2 ? lo : hi;
        dst[2 * (w & 1)] = d0 | (d1 << 16);
        dst[2 * (w & 1) + 1] = d2 | (d3 << 16);
    }
}

__device__ __forceinline__ void store_nan_row(uint16_t* __restrict__ out) {
    const uint32_t n2 = cut8::BF16_NAN | ((uint32_t)cut8::BF16_NAN << 16);
    const u32x4 nan = {n2, n2, n2, n2};
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        u32x4* p = reinterpret_cast<u32x4*>(out + chunk_elem(j));
        p[0] = nan;
        p[1] = nan;
    }
}

template <int FMT, class Round, class... Key>
__global__ __launch_bounds__(THREADS) void cut8_encode_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ rec,
                                                              Key... key) {
    __shared__ uint32_t red[4];
    const Round round = block_round<FMT, Round>(key...);
    Sample s;
    load_sample(x + (size_t)blockIdx.x * cut8::SAMPLE, s);
    const uint32_t a = block_amax_bits(s, red);
    const bool poison = a >= 0x7f80u;
    const int32_t e = poison ? cut8::POISON : cut8::scale_exp<FMT>(a);
    uint8_t* r = rec + (size_t)blockIdx.x * cut8::RECORD;
    if (threadIdx.x == 0) {
        const u32x4 head = {(uint32_t)e, (uint32_t)FMT, 0u, 0u};
        *reinterpret_cast<u32x4*>(r) = head;
    }
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        const u32x4 codes = poison ? zero : encode16<FMT>(s.v[2 * j], s.v[2 * j + 1], e, round, (uint32_t)chunk_elem(j));
        *reinterpret_cast<u32x4*>(r + cut8::HEADER + chunk_elem(j)) = codes;
    }
}

template <int FMT>
__global__ __launch_bounds__(THREADS) void cut8_decode_kernel(const uint8_t* __restrict__ rec, uint16_t* __restrict__ out,
                                                              int* __restrict__ err_flag) {
    const uint8_t* r = rec + (size_t)blockIdx.x * cut8::RECORD;
    uint16_t* o = out + (size_t)blockIdx.x * cut8::SAMPLE;
    const u32x4 head = *reinterpret_cast<const u32x4*>(r);
    const int32_t e = (int32_t)head[0];
    const bool poison = e == cut8::POISON;
    const bool bad = head[1] != (uint32_t)FMT || (head[2] | head[3]) != 0u ||
                     (!poison && (e < cut8::E_MIN || e > cut8::E_MAX));
    if (bad || poison) {   // uniform over the block
        if (bad && threadIdx.x == 0) err_flag[0] = 1;
        store_nan_row(o);
        return;
    }
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const u32x4 codes = *reinterpret_cast<const u32x4*>(r + cut8::HEADER + chunk_elem(j));
        u32x4 lo, hi;
        decode16<FMT>(codes, e, lo, hi);
        u32x4* p = reinterpret_cast<u32x4*>(o + chunk_elem(j));
        p[0] = lo;
        p[1] = hi;
    }
}

// decode(encode(x)) without the record; x and out are not __restrict__: they may be the same buffer (a block
// has read its whole sample, and passed the reduction's barrier, before its first store); the step counter is read
// before that barrier too.
template <int FMT, class Round, class... Key>
__global__ __launch_bounds__(THREADS) void cut8_roundtrip_kernel(const uint16_t* x, uint16_t* out, Key... key) {
    __shared__ uint32_t red[4];
    const Round round = block_round<FMT, Round>(key...);
    Sample s;
    load_sample(x + (size_t)blockIdx.x * cut8::SAMPLE, s);
    const uint32_t a = block_amax_bits(s, red);
    uint16_t* o = out + (size_t)blockIdx.x * cut8::SAMPLE;
    if (a >= 0x7f80u) {
        store_nan_row(o);
        return;
    }
    const int e = cut8::scale_exp<FMT>(a);
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const u32x4 codes = encode16<FMT>(s.v[2 * j], s.v[2 * j + 1], e, round, (uint32_t)chunk_elem(j));
        u32x4 lo, hi;
        decode16<FMT>(codes, e, lo, hi);
        u32x4* p = reinterpret_cast<u32x4*>(o + chunk_elem(j));
        p[0] = lo;
        p[1] = hi;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
}  // namespace

extern "C" int64_t slk_cut8_record_bytes() { return cut8::RECORD; }

extern "C" int slk_cut8_encode(const void* x_bf16, int n, int fmt, void* rec, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && rec && aligned16(x_bf16) && aligned16(rec));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint8_t* r = static_cast<uint8_t*>(rec);
    if (fmt == 0) cut8_encode_kernel<0, Nearest><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r);
    else cut8_encode_kernel<1, Nearest><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r);
    return slk_launch_status();
}

extern "C" int slk_cut8_decode(const void* rec, int n, int fmt, void* out_bf16, int* err_flag, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(rec && out_bf16 && err_flag && aligned16(rec) && aligned16(out_bf16));
    SLK_CHECK_ARG((reinterpret_cast<uintptr_t>(err_flag) & 3u) == 0);
    const uint8_t* r = static_cast<const uint8_t*>(rec);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    if (fmt == 0) cut8_decode_kernel<0><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(r, o, err_flag);
    else cut8_decode_kernel<1><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(r, o, err_flag);
    return slk_launch_status();
}

extern "C" int slk_cut8_roundtrip(const void* x_bf16, int n, int fmt, void* out_bf16, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && aligned16(x_bf16) && aligned16(out_bf16));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    if (fmt == 0) cut8_roundtrip_kernel<0, Nearest><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o);
    else cut8_roundtrip_kernel<1, Nearest><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o);
    return slk_launch_status();
}

extern "C" int slk_cut8_encode_sr(const void* x_bf16, int n, int fmt, void* rec, uint32_t seed, const int* step, int row0,
                                  void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1) && row0 >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && rec && aligned16(x_bf16) && aligned16(rec) && step && aligned4(step));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint8_t* r = static_cast<uint8_t*>(rec);
    if (fmt == 0) cut8_encode_kernel<0, Stochastic><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r, seed, step, row0);
    else cut8_encode_kernel<1, Stochastic><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, r, seed, step, row0);
    return slk_launch_status();
}

extern "C" int slk_cut8_roundtrip_sr(const void* x_bf16, int n, int fmt, void* out_bf16, uint32_t seed, const int* step,
                                     int row0, void* stream) {
    SLK_CHECK_ARG(n >= 0 && (fmt == 0 || fmt == 1) && row0 >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && aligned16(x_bf16) && aligned16(out_bf16) && step && aligned4(step));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    if (fmt == 0) cut8_roundtrip_kernel<0, Stochastic><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o, seed, step, row0);
    else cut8_roundtrip_kernel<1, Stochastic><<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(x, o, seed, step, row0);
    return slk_launch_status();
}
