// slk_wide_head.h — the device helpers the K5 server head's kernels share: slk_wide_head.hip (the head on a bf16 cut)
// and slk_wide_head_mx.hip (the same head on MX cut records). The dropout hash, the chunk arithmetic of the cut
// gradient and the tiling constants live here once, so both files run the same float32 expressions in the same
// order. Internal; not part of the ABI.
#pragma once

#include "slk_common.h"

namespace {
constexpr int CUTF = 16384;       // features per sample
constexpr int NCH = CUTF / 8;     // 2048 chunks of 8 channels (C8 order: chunk = plane*64 + pixel)
constexpr int NC = 10;
}  // namespace

// keep bits of the 8 features of chunk fc (C8 order) of sample b: feature index (torch flatten) of
// element k is (plane*8 + k)*64 + pixel.
__device__ __forceinline__ uint32_t keep_bits(uint32_t b, int fc, uint32_t step, uint32_t seed, uint32_t thresh) {
    const uint32_t plane = fc >> 6, pix = fc & 63;
    const uint32_t base = step * 0x85EBCA77u + seed * 0xC2B2AE3Du;
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t e = b * (uint32_t)CUTF + (plane * 8 + k) * 64 + pix;
        bits |= (lowbias32(e * 0x9E3779B1u + base) >= thresh ? 1u : 0u) << k;
    }
    return bits;
}

__device__ __forceinline__ void unpack8(const uint4 v, float (&f)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = __uint_as_float(w[k] << 16);
        f[2 * k + 1] = __uint_as_float(w[k] & 0xFFFF0000u);
    }
}
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (uint32_t)__builtin_bit_cast(uint16_t, x) | ((uint32_t)__builtin_bit_cast(uint16_t, y) << 16);
}

constexpr int HSLICE = 8;            // 2048-feature slices (256 chunks each)
#ifndef SLK_HSG
#define SLK_HSG 64
#endif
constexpr int HSG = SLK_HSG;         // samples per group (= per fc weight-gradient slab)
#ifndef SLK_HEAD_PF
#define SLK_HEAD_PF 1
#endif
constexpr int HPF = SLK_HEAD_PF;     // samples' cut chunks in flight ahead of the one in use (A/B: 2 and 4 no gain)

__device__ __forceinline__ void load_w(const float* __restrict__ wf8, int fc, float (&w)[NC][8]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const float4 lo = *reinterpret_cast<const float4*>(wf8 + (size_t)j * CUTF + fc * 8);
        const float4 hi = *reinterpret_cast<const float4*>(wf8 + (size_t)j * CUTF + fc * 8 + 4);
        w[j][0] = lo.x; w[j][1] = lo.y; w[j][2] = lo.z; w[j][3] = lo.w;
        w[j][4] = hi.x; w[j][5] = hi.y; w[j][6] = hi.z; w[j][7] = hi.w;
    }
}

// dropout applied to a loaded cut chunk v of sample b; returns the keep bits
__device__ __forceinline__ uint32_t dropped(uint4 v, int b, int fc, uint32_t step, uint32_t seed, uint32_t thresh,
                                            float keep_scale, float (&d)[8]) {
    const uint32_t kb = keep_bits((uint32_t)b, fc, step, seed, thresh);
    unpack8(v, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = (kb >> k) & 1 ? d[k] * keep_scale : 0.f;
    return kb;
}

// cut gradient of one 8-feature chunk: (dlogits @ Wf) masked and scaled like the forward's dropout
__device__ __forceinline__ uint4 dcut_chunk(const float (&w)[NC][8], const float (&dlr)[NC], uint32_t kb, float keep_scale) {
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) a = __builtin_fmaf(dlr[j], w[j][k], a);
        o[k] = (kb >> k) & 1 ? a * keep_scale : 0.f;
    }
    return make_uint4(pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7]));
}

// wide_head16_kernel's tiling (slk_wide_head.hip): 16 samples per workgroup of 8 waves, wave w owning chunks
// [256 w, 256 w + 256) in blocks of 4 (one per kg lane group).
constexpr int WH_S = 16, WH_T = 512, WH_W = WH_T / 64;
constexpr int WH_CPW = NCH / WH_W;  // 256 chunks per wave = 64 blocks of 4
constexpr int WH_KBS = NCH + 16;    // LDS row stride of the dropout bits (16 rows x 4 dwords: 64 distinct banks)
