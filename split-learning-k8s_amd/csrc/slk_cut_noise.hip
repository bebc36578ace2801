// slk_cut_noise.hip — per-sample norm clip and additive table noise on the K5 cut (include/slk.h, "Cut noise").
//
// The skeleton is slk_cut8.hip's: one block of 256 threads owns one sample of 16,384 bf16 elements and reads it
// once — thread t holds elements [16 (256 j + t), +16) for j = 0..3, two 16-byte loads each, 64 elements in 32
// registers — from the reduction to the store. The squared norm is summed in ONE fixed order (the thread's 64
// products in ascending element order, the xor butterfly inside the wave, (w0 + w1) + (w2 + w3) across the four
// waves through 16 bytes of LDS), so the same sample gives the same bits whatever shares the launch. The noise table
// is staged once per block in 4 KB of LDS and gathered by the draw's stratum k. Every output element is written by
// exactly one thread with a 16-byte store and the sample's stats pair by thread 0 with one 8-byte store; no atomics.
//
// Every float operation of the rule is rounded on its own: the whole file is compiled without fma contraction.
#include "slk_common.h"

#pragma clang fp contract(off)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {
constexpr int THREADS = 256;
constexpr int SAMPLE = 16384;                      // bf16 elements of one K5 cut (or cut-gradient row)
constexpr int CHUNKS = SAMPLE / (16 * THREADS);    // 4 chunks of 16 elements per thread
constexpr int TABLE = 1024;                        // strata of the noise table

struct Sample {
    u32x4 v[2 * CHUNKS];  // chunk j: v[2j], v[2j + 1] — 16 bf16, element 2i in the low half of word i
};

__device__ __forceinline__ size_t chunk_elem(int j) { return 16 * ((size_t)j * THREADS + threadIdx.x); }

__device__ __forceinline__ void load_sample(const uint16_t* x, Sample& s) {
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        const u32x4* p = reinterpret_cast<const u32x4*>(x + chunk_elem(j));
        s.v[2 * j] = p[0];
        s.v[2 * j + 1] = p[1];
    }
}

__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

// bf16(a) | bf16(b) << 16, round to nearest even, a NaN stays a (quiet) NaN: gfx950's packed convert.
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The thread's part of s2: fl(x * x) added one at a time from 0, chunk ascending, then element ascending.
__device__ __forceinline__ float thread_sumsq(const Sample& s) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * CHUNKS; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float lo = bf16_lo(s.v[i][k]), hi = bf16_hi(s.v[i][k]);
            a = a + lo * lo;
            a = a + hi * hi;
        }
    }
    return a;
}

// The key of one sample (g its global row, t the step counter's value) and the noise of element i under it.
__device__ __forceinline__ uint32_t noise_base(uint32_t g, uint32_t t, uint32_t seed) {
    return lowbias32(g * 0x9E3779B1u + t * 0x85EBCA77u + seed * 0xC2B2AE3Du + 3u * 0x27D4EB2Fu);
}
__device__ __forceinline__ float noise_at(uint32_t base, uint32_t i, const float* tab, float tail, float scale) {
    const uint32_t r = lowbias32(base + i * 0x9E3779B1u);
    const uint32_t r2 = lowbias32(r + 0x9E3779B9u);
    const uint32_t k = (r >> 21) & (TABLE - 1);
    const float G = (float)(r2 ? __builtin_clz(r2) : 32);
    const float a = tail * G + tab[k];
    const float n = scale * a;
    return __uint_as_float(__float_as_uint(n) ^ (r & 0x80000000u));
}

// x and out are not __restrict__: they may be the same buffer (a thread stores only the elements it loaded).
template <bool CLIP, bool NOISE>
__global__ __launch_bounds__(THREADS) void cut_noise_kernel(const uint16_t* x, uint16_t* out,
                                                            const float* __restrict__ table, float tail,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ max_norm, uint32_t seed,
                                                            const int* __restrict__ step, uint32_t row0,
                                                            float* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float tab[TABLE];
    __shared__ float red[4];
    Sample s;
    load_sample(x + (size_t)blockIdx.x * SAMPLE, s);
    uint32_t base = 0;
    float sc = 0.f;
    if (NOISE) {
        reinterpret_cast<f32x4*>(tab)[threadIdx.x] = reinterpret_cast<const f32x4*>(table)[threadIdx.x];
        sc = *scale;
        base = noise_base(row0 + blockIdx.x, (uint32_t)*step, seed);
    }
    if (CLIP) {
        float a = thread_sumsq(s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a = a + __shfl_xor(a, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    }
    if (CLIP || NOISE) __syncthreads();
    float coef = 1.f;
    if (CLIP) {
        const float s2 = (red[0] + red[1]) + (red[2] + red[3]);
        // sqrtf and / are correctly rounded under hipcc's defaults (v_sqrt_f32 plus its fma fix-up, the v_div_scale /
        // v_div_fmas / v_div_fixup sequence). NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS that name is the
        // bare v_sqrt_f32 (1 ulp), which the listing showed.
        const float norm = sqrtf(s2);
        const float q = *max_norm / (norm + 1e-6f);
        coef = q > 1.f ? 1.f : q;   // a compare: a NaN norm gives a NaN coefficient
        if (stats && threadIdx.x == 0) {
            const f32x2 pair = {norm, coef};
            *reinterpret_cast<f32x2*>(stats + 2 * (size_t)blockIdx.x) = pair;
        }
    }
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 v = s.v[2 * j + h];
            u32x4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = (uint32_t)chunk_elem(j) + 8 * h + 2 * k;
                float c0 = bf16_lo(v[k]), c1 = bf16_hi(v[k]);
                if (CLIP) {
                    c0 = coef * c0;
                    c1 = coef * c1;
                }
                if (NOISE) {
                    c0 = c0 + noise_at(base, i, tab, tail, sc);
                    c1 = c1 + noise_at(base, i + 1, tab, tail, sc);
                }
                y[k] = pack_bf16x2(c0, c1);
            }
            reinterpret_cast<u32x4*>(o + chunk_elem(j))[h] = y;
        }
    }
}

// out_i = bf16(fl(coef_row * x_i)), coef_row = stats[row][1]; x and out may be the same buffer.
__global__ __launch_bounds__(THREADS) void cut_scale_rows_kernel(const uint16_t* x, uint16_t* out,
                                                                 const float* __restrict__ stats) {
    const float coef = stats[2 * (size_t)blockIdx.x + 1];
    Sample s;
    load_sample(x + (size_t)blockIdx.x * SAMPLE, s);
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 v = s.v[2 * j + h];
            u32x4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = pack_bf16x2(coef * bf16_lo(v[k]), coef * bf16_hi(v[k]));
            reinterpret_cast<u32x4*>(o + chunk_elem(j))[h] = y;
        }
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" int slk_cut_noise(const void* x_bf16, int n, const float* table, float tail, const float* scale,
                             const float* max_norm, uint32_t seed, const int* step, int row0, void* out_bf16,
                             float* stats, void* stream) {
    SLK_CHECK_ARG(n >= 0 && row0 >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && aligned(x_bf16, 16) && aligned(out_bf16, 16));
    SLK_CHECK_ARG(!scale || (aligned(scale, 4) && table && aligned(table, 16) && step && aligned(step, 4)));
    SLK_CHECK_ARG(!max_norm || aligned(max_norm, 4));
    SLK_CHECK_ARG(!stats || aligned(stats, 8));
    const uint16_t* x = static_cast<const uint16_t*>(x_bf16);
    uint16_t* o = static_cast<uint16_t*>(out_bf16);
    const dim3 grid((unsigned)n), block(THREADS);
    hipStream_t st = slk_stream(stream);
    const uint32_t r0 = (uint32_t)row0;
    if (max_norm && scale)
        cut_noise_kernel<true, true><<<grid, block, 0, st>>>(x, o, table, tail, scale, max_norm, seed, step, r0, stats);
    else if (max_norm)
        cut_noise_kernel<true, false><<<grid, block, 0, st>>>(x, o, table, tail, scale, max_norm, seed, step, r0, stats);
    else if (scale)
        cut_noise_kernel<false, true><<<grid, block, 0, st>>>(x, o, table, tail, scale, max_norm, seed, step, r0, stats);
    else
        cut_noise_kernel<false, false><<<grid, block, 0, st>>>(x, o, table, tail, scale, max_norm, seed, step, r0, stats);
    return slk_launch_status();
}

extern "C" int slk_cut_scale_rows(const void* x_bf16, int n, const float* stats, void* out_bf16, void* stream) {
    SLK_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && stats && aligned(x_bf16, 16) && aligned(out_bf16, 16) && aligned(stats, 8));
    cut_scale_rows_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(static_cast<const uint16_t*>(x_bf16),
                                                                         static_cast<uint16_t*>(out_bf16), stats);
    return slk_launch_status();
}
