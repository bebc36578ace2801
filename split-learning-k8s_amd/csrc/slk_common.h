// slk_common.h — shared helpers for the gfx950 split-CNN kernels (internal; not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slk.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Fixed model geometry (src/model_def.py:8,18,20,22).
namespace slk {
constexpr int IN_HW = 28;            // x: 1 x 28 x 28
constexpr int C1 = 32;               // conv1 out channels
constexpr int A_HW = 26;             // cut activation spatial size
constexpr int A_PIX = A_HW * A_HW;   // 676
constexpr int A_SAMPLE = C1 * A_PIX; // 21632 floats per sample (86,528 B)
constexpr int C2 = 64;               // conv2 out channels
constexpr int O_HW = 24;             // conv2 output spatial size
constexpr int P_HW = 12;             // pooled spatial size
constexpr int P_WIN = P_HW * P_HW;   // 144 pooling windows per channel
constexpr int P_SAMPLE = C2 * P_WIN; // 9216 = fc1 in_features
constexpr int NCLS = 10;
constexpr int K2 = C1 * 9;           // conv2 reduction length per output (288)
constexpr int W2_N = C2 * K2;        // 18432
constexpr int W3_N = NCLS * P_SAMPLE;// 92160
constexpr int CODE_NONE = 4;         // pooled value <= 0: ReLU blocks the gradient
}  // namespace slk

template <typename T>
__device__ __forceinline__ void slk_keep(T& v) { asm volatile("" : "+v"(v)); }

#define SLK_CHECK_ARG(cond)                 \
    do {                                    \
        if (!(cond)) return (int)hipErrorInvalidValue; \
    } while (0)

static inline int slk_launch_status() { return (int)hipGetLastError(); }

static inline hipStream_t slk_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Learning rate of optimizer step `step` from a device table (slk_sgdm_* / slk_adamw_*): the schedule is
// device memory, so a captured HIP graph reads this replay's rate; past the end the last value holds.
__device__ __forceinline__ float slk_lr_at(const float* __restrict__ lr_table, int lr_len, int step) {
    return lr_table[min(max(step, 0), lr_len - 1)];
}

// The counter-based hash behind the K5 dropout mask (slk_wide_head.hip) and the augmentation draws
// (slk_data.hip): a pure function of its 32-bit input, so a draw depends on what it is keyed on alone.
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// The soft-target heads (slk_*_soft, include/slk.h "mixed label"): decode y = a | b << 8 | bits(wb) << 32, validate
// it, and build the row's target distribution t[10] in the documented float32 order:
//   u_j = (j == a ? fl(1 - wb) : 0) + (j == b ? wb : 0);  t_j = fmaf(fl(1 - smoothing), u_j, fl(smoothing / 10)).
// Returns whether the target is well formed (NaN and negative wb fail the compares; y < 0 is wb's sign bit).
__device__ __forceinline__ bool slk_soft_target(int64_t y, float smoothing, float (&t)[10]) {
    const uint32_t lo = (uint32_t)(uint64_t)y, hi = (uint32_t)((uint64_t)y >> 32);
    const uint32_t a = lo & 0xffu, b = (lo >> 8) & 0xffu;
    const float wb = __uint_as_float(hi);
    const bool ok = y >= 0 && a < 10u && b < 10u && (lo >> 16) == 0u && wb >= 0.f && wb <= 1.f;
    const float wa = 1.f - wb, keep = 1.f - smoothing, flat = smoothing / 10.f;
#pragma unroll
    for (uint32_t j = 0; j < 10u; ++j) {
        const float u = (j == a ? wa : 0.f) + (j == b ? wb : 0.f);
        t[j] = __builtin_fmaf(keep, u, flat);
    }
    return ok;
}
// S = sum_j t_j z_j over ascending j by fmaf from S = 0, classes with t_j == 0 skipped (a select: 0 * -inf is NaN).
__device__ __forceinline__ float slk_soft_dot(const float (&t)[10], const float (&z)[10]) {
    float S = 0.f;
#pragma unroll
    for (int j = 0; j < 10; ++j) S = t[j] != 0.f ? __builtin_fmaf(t[j], z[j], S) : S;
    return S;
}

// f32-input MFMA wrappers (exact f32, k-ordered fma chain; cdna_hip_programming.md §3).
// 32x32x2: lane l supplies A[i=l&31][k=l>>5] and B[k=l>>5][j=l&31];
//          D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5), r in [0,16).
// 16x16x4: lane l supplies A[i=l&15][k=l>>4] and B[k=l>>4][j=l&15];
//          D: col = l&15, row = 4*(l>>4) + r, r in [0,4).
__device__ __forceinline__ f32x16 mfma32x32x2(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Butterfly sum over the 64 lanes: every lane ends with the total, bit-identically (each step adds
// the same two partial sums, commutatively, in both partner lanes). Inside a 16-lane row by DPP
// (quad_perm 1032 / 2301, row_half_mirror, row_mirror: no LDS traffic), then across rows by
// ds_swizzle/bpermute.
__device__ __forceinline__ float wave_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm 1,0,3,2
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad_perm 2,3,0,1
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));  // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Sum of one value per thread over a 1024-thread block, the same bits in every thread: wave_sum inside each
// of the 16 waves, lane 0 of wave w leaves its wave's sum in red[w], then every thread adds red[0..15] in
// ascending wave order. Block-wide (one barrier); red holds 16 floats of LDS scratch.
__device__ __forceinline__ float slk_block_sum_1024(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += red[w];
    return t;
}

// Global-norm gradient clipping (slk_reduce_sqnorm_multi -> slk_sgdm_clip_multi / slk_adamw_clip_multi).
// The coefficient of one group from the block partials of its squared norm; every thread of a 1024-thread
// block calls it. Thread j adds partials j, j + 1024, j + 2048, ... in ascending order (starting from 0),
// then slk_block_sum_1024: a fixed function of (partials, npart) alone, so every block of every launch holds
// the same total, whatever else shares the launch. norm = sqrtf(total); coef = max_norm / (norm + 1e-6f)
// clamped from above at 1 by a compare, so a NaN norm gives a NaN coefficient (torch.clamp(max=1.0)), an
// infinite one 0 and a zero one 1: torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) in float32.
__device__ __forceinline__ float slk_clip_coef(const float* __restrict__ partials, int npart,
                                               const float* __restrict__ max_norm, float* red, float& norm) {
    float s = 0.f;
    for (int j = threadIdx.x; j < npart; j += 1024) s += partials[j];
    norm = sqrtf(slk_block_sum_1024(s, red));
    const float coef = *max_norm / (norm + 1e-6f);
    return coef > 1.f ? 1.f : coef;
}

// Host side of the two clip passes: where each segment's block partials live. Segments of one group (one
// stage) are consecutive, group ids start at 0 and rise by at most 1; segment s writes / its group reads
// partials[group[s]][off[s] + blk], blk < nblk[s] = slk_reduce_sqnorm_nblk(n[s], nslab[s]); npart[s] is the
// group's total and first[s] marks the group's first non-empty segment (its first block reports norm, coef).
constexpr int SLK_CLIP_MAXSEG = 4;
struct SlkClipLayout {
    int nblk[SLK_CLIP_MAXSEG], off[SLK_CLIP_MAXSEG], npart[SLK_CLIP_MAXSEG], first[SLK_CLIP_MAXSEG];
};
static inline bool slk_clip_layout(const int* nslab, const int* n, const int* group, int nseg, int ngroup,
                                   SlkClipLayout& L) {
    if (nseg < 1 || nseg > SLK_CLIP_MAXSEG || ngroup < 1 || ngroup > nseg || !nslab || !n || !group) return false;
    int gtot[SLK_CLIP_MAXSEG] = {0, 0, 0, 0};
    bool seen[SLK_CLIP_MAXSEG] = {false, false, false, false};
    for (int s = 0; s < nseg; ++s) {
        const int g = group[s];
        if (g >= ngroup || (s == 0 ? g != 0 : (g != group[s - 1] && g != group[s - 1] + 1))) return false;
        if (n[s] < 0 || nslab[s] < 1) return false;
        L.nblk[s] = slk_reduce_sqnorm_nblk(n[s], nslab[s]);
        L.off[s] = gtot[g];
        gtot[g] += L.nblk[s];
        L.first[s] = L.nblk[s] > 0 && !seen[g];
        seen[g] = seen[g] || L.nblk[s] > 0;
    }
    if (group[nseg - 1] != ngroup - 1) return false;
    for (int s = 0; s < nseg; ++s) L.npart[s] = gtot[group[s]];
    return true;
}

// Layer-wise trust ratios (slk_reduce_tnorm_multi -> slk_lars_multi, slk_lamb_moments_multi -> slk_lamb_multi).
// A segment is one [W | b] pair: elements [0, nw) are the weight tensor, [nw, n) the bias. Block blk of a
// segment's pass 1 leaves four partials [x2_W, p2_W, x2_b, p2_b] at partials[group][4 * (off + blk)], x the
// gradient (LARS) or the update direction (LAMB), p the parameter before the step.
//
// Four block sums at once, each the bits of slk_block_sum_1024 (one barrier; red is [4][16] floats of LDS).
__device__ __forceinline__ void slk_block_sum4_1024(float (&v)[4], float (*red)[16]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float t = red[k][0];
#pragma unroll
        for (int w = 1; w < 16; ++w) t += red[k][w];
        v[k] = t;
    }
}
// The four totals of one segment from its npart blocks' partials, in slk_clip_coef's order per component:
// thread j adds partials j, j + 1024, ... ascending from 0, then the block sum. A fixed function of the
// segment's own partials, so every block of every launch holds the same bits.
__device__ __forceinline__ void slk_tensor_totals(const float* __restrict__ partials, int npart, float (*red)[16],
                                                  float (&tot)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = 0.f;
    for (int j = threadIdx.x; j < npart; j += 1024) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(partials + 4 * (size_t)j);
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] += q[k];
    }
    slk_block_sum4_1024(tot, red);
}
// LARS (You, Gitman, Ginsburg 2017): wn = sqrt(sum p^2), gn = sqrt(sum g^2),
// ratio = fl(trust_coef * wn) / ((gn + fl(wd * wn)) + eps) where wn > 0 and gn > 0, else 1 (a NaN norm fails
// the compare). Both products are rounded on their own.
__device__ __forceinline__ float slk_lars_ratio(float sum_g2, float sum_p2, float trust_coef, float wd, float eps,
                                                float& wn, float& gn) {
    wn = sqrtf(sum_p2);
    gn = sqrtf(sum_g2);
    float num = trust_coef * wn, dw = wd * wn;
    slk_keep(num);
    slk_keep(dw);
    const float r = num / ((gn + dw) + eps);
    return (wn > 0.f && gn > 0.f) ? r : 1.f;
}
// LAMB (You et al. 2019): ratio = wn / un where both are > 0, else 1.
__device__ __forceinline__ float slk_lamb_ratio(float sum_u2, float sum_p2, float& wn, float& un) {
    wn = sqrtf(sum_p2);
    un = sqrtf(sum_u2);
    const float r = wn / un;
    return (wn > 0.f && un > 0.f) ? r : 1.f;
}

// Host side of the layer-wise passes: slk_clip_layout's block counts and offsets (in blocks: a block owns four
// floats of partials), plus the checks on nw and each segment's index inside its group (its two rows of the
// group's trust_out).
struct SlkTrustLayout {
    SlkClipLayout c;
    int slot[SLK_CLIP_MAXSEG];
};
static inline bool slk_trust_layout(const int* nslab, const int* n, const int* nw, const int* group, int nseg,
                                    int ngroup, SlkTrustLayout& L) {
    if (!nw || !slk_clip_layout(nslab, n, group, nseg, ngroup, L.c)) return false;
    for (int s = 0; s < nseg; ++s) {
        if (nw[s] < 0 || nw[s] > n[s]) return false;
        L.slot[s] = (s > 0 && group[s] == group[s - 1]) ? L.slot[s - 1] + 1 : 0;
    }
    return true;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The x3 scale value of the cut a = relu(conv1(x) + b1) of one sample, computed by the client's conv1
// kernels (round 5): an upper bound of max a from the image's max |x| alone,
//     bound = max_c fma(sum_k |W1[c][k]| (taps in order), max|x|, max(b1[c], 0)),
// the same float expression in every kernel that emits it, so their act_amax outputs agree bit for bit.
// Only the scale's power of two is derived from it (x3_exp: the bound lands in [2^13, 2^14)), so the
// image writer needs no first pass over its own outputs. How far the cut's max sits below the bound depends
// on the data and the weights (mixed-sign W1 or cancelling inputs make it loose): every factor of 2 of
// slack moves the whole split one bit lower, so elements ~2^-24 of the bound and below lose lo-part bits to
// f16's subnormal range — the absolute error stays ~2^-24 of the bound (tests/test_x3_gpu.py checks x3 vs the
// f32 path with a bound 2^4-2^6 x the max). Block-wide: every thread calls it after xs
// (the 28 x 28 image in LDS) is complete; red holds >= 8 floats of scratch; returns the bound to all.
__device__ __forceinline__ float conv1_cut_bound(const float* xs, const float* __restrict__ W1,
                                                 const float* __restrict__ b1, float* red) {
    const int tid = threadIdx.x, nw = (blockDim.x + 63) >> 6;
    float m = 0.f;
    for (int i = tid; i < slk::IN_HW * slk::IN_HW; i += blockDim.x) m = fmaxf(m, fabsf(xs[i]));
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    float xmax = red[0];
    for (int w = 1; w < nw; ++w) xmax = fmaxf(xmax, red[w]);
    float bc = 0.f;
    if (tid < 64) {
        if (tid < slk::C1) {
            float ws = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) ws += fabsf(W1[tid * 9 + k]);
            bc = fmaf(ws, xmax, fmaxf(b1[tid], 0.f));
        }
        bc = wave_max(bc);
    }
    __syncthreads();  // every wave has read red[]
    if (tid == 0) red[0] = bc;
    __syncthreads();
    return red[0];
}

// ---------------------------------------------------------------------------- LDS-DMA as inline asm
// global_load_lds issued through asm: hipcc then neither counts it nor inserts its own vmcnt(0) in
// front of LDS reads and writes it cannot prove disjoint from a DMA in flight (it cannot tell a
// prefetch buffer from the one being read, so the prefetch would drain before every use). The kernel
// retires the DMA with its own counted `s_waitcnt vmcnt` + barrier. lds_dst is wave-uniform.
typedef __attribute__((address_space(3))) void* slk_lds_ptr;
__device__ __forceinline__ uint32_t lds_u32(const void* p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(slk_lds_ptr)(const_cast<void*>(p)));
}
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// Scalar base + per-lane 32-bit byte offset (saddr form): with the lane offsets computed once per
// launch, a piece costs no VALU address arithmetic at all (sbase is wave-uniform).
__device__ __forceinline__ void glds16_so(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
