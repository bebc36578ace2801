// slk_wide_headn.hip — the K5 server head for 1 <= nc <= 128 classes (include/slk.h, "The n-class head"): dropout,
// Linear(16384, nc), cross-entropy and their backward as three bf16 GEMMs on v_mfma_f32_16x16x32_bf16, plus the
// evaluation kernels for nc classes. The 10-class head (slk_wide_head.hip) keeps its own kernels; nothing is shared
// with it but the dropout hash (keep_bits of slk_wide_head.h).
//
// Operands. wq = [bf16(Wf) in the cut's C8 order, [128][16384], rows >= nc zero | its transpose [16384][128]]
// (slk_wide_fcn_shadow); the cut is bf16 C8 [B][16384]; dlq = bf16(dlogits) padded to [Bp][128] and its transpose
// [128][Bp], Bp = B rounded up to 256 (headn_dlq_kernel, into `work`). Every GEMM's K index is a memory order both
// of its operands share, so a lane's A and B fragments (8 consecutive K elements each) are plain 16-byte reads
// except the weight gradient's cut operand, which needs 8 consecutive SAMPLES of one feature and comes out of LDS
// by ds_read_b64_tr_b16. The dropout mask is applied to the cut's bits while staging (a dropped element becomes +0),
// keep_scale once to each finished f32 sum.
//
//   logits   M = 128 classes, N = samples, K = 16384. Grid = (128-sample tile) x (8 slices of 2048 features), 4
//            waves as 2 (class halves) x 2 (sample halves), 4 x 4 accumulator tiles a wave. A slice is walked in 32
//            stages of 64 features: the wq tile and the masked cut tile [128][64] go global -> registers -> LDS
//            (rows 144 B apart: a 16-lane fragment read covers all banks), the next stage's loads and hashes are
//            issued before the stage's 32 MFMAs a wave. Each workgroup leaves its f32 partial [slice][B][128] in
//            `work` (float4 stores: a lane holds 4 consecutive classes of one sample); wq traffic = cut traffic.
//            Accumulation order of S_j: within a slice ascending stages, K step 0 then 1 of a stage, the MFMA's own
//            order inside a K step; then slices 0..7 ascending (headn_ce_kernel).
//   ce       16 samples a workgroup: 16 threads a sample add the 8 partials in slice order, z = fl(keep_scale S) +
//            bf; one thread a sample runs the cross-entropy of slk_wide_head over nc classes, ascending j.
//   dcut     M = features, N = samples, K = 128 classes (4 K steps). A wave owns 64 consecutive C8 features: its 16
//            A fragments of wq's transpose live in registers for the whole launch; it walks 16-sample tiles, reading
//            dlq fragments straight from global (1 MB at B = 4096: cache hits), the next tile's before this tile's
//            16 MFMAs. M rows are permuted so that a lane ends with the 8 features of one chunk of one sample: mask,
//            scale, pack, one 16-byte store (128 B contiguous per sample and wave).
//   wgrad    M = 128 classes, N = features, K = a 256-sample share of the batch = one slab. Grid = (128-feature
//            block) x (share). Stages of 64 samples: dlq's transpose tile [128][64] (rows 144 B) and the masked cut
//            tile [16 chunks][64 samples][8] (chunk planes 1088 B apart = 64 mod 256, samples xor-swizzled by chunk
//            pair so the staging writes spread over the banks) in LDS; a wave holds 8 x 2 accumulator tiles (all
//            classes x 32 features). dbf = one more MFMA against a ones fragment in the workgroups of feature block
//            0. The epilogue scales and stores in torch's parameter order (4-byte stores, 8-byte runs: the C8 order
//            of the N tile is not torch's).
// No atomics except the label flag, one writer per output byte, every sum in a fixed order: bits repeat run to run.
#include "slk_common.h"
#include "slk_wide_head.h"   // keep_bits: the dropout hash, and CUTF / NCH

#pragma clang fp contract(off)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int NP = 128;              // classes, padded
constexpr int HN_SLICES = 8;         // logits: K slices
constexpr int HN_KSL = CUTF / HN_SLICES;
constexpr int HN_TM = 128;           // logits: samples per workgroup
constexpr int HN_KC = 64;            // features (logits) / samples (wgrad) per LDS stage
constexpr int HN_RST = 2 * HN_KC + 16;   // bytes between two LDS rows of 64 bf16
constexpr int HN_SHARE = 256;        // wgrad: samples per slab
constexpr int HN_PST = (HN_KC + 4) * 16; // wgrad: bytes between two chunk planes of the cut tile
constexpr int HN_NF = 128;           // wgrad: features per workgroup (16 chunks)
constexpr int HN_DCY = 16;           // dcut: workgroups along the sample tiles
static_assert(HN_PST % 256 == 64 && HN_RST % 16 == 0 && (NP * HN_RST) % 1024 == 0, "LDS geometry");

__host__ __device__ constexpr int headn_bp(int B) { return (B + HN_SHARE - 1) / HN_SHARE * HN_SHARE; }
}  // namespace

// the cut chunk v with its dropped elements replaced by +0 (element 2 i is the low half of word i)
__device__ __forceinline__ uint32_t headn_mask2(uint32_t w, uint32_t two) {
    return w & ((two & 1u ? 0xFFFFu : 0u) | (two & 2u ? 0xFFFF0000u : 0u));
}
__device__ __forceinline__ u32x4 headn_mask8(u32x4 v, uint32_t kb) {
    return u32x4{headn_mask2(v[0], kb), headn_mask2(v[1], kb >> 2), headn_mask2(v[2], kb >> 4), headn_mask2(v[3], kb >> 6)};
}
// keep_threshold 0 keeps everything (hash >= 0): evaluation skips the hash
__device__ __forceinline__ uint32_t headn_bits(int b, int fc, uint32_t step, uint32_t seed, uint32_t thresh) {
    return thresh ? keep_bits((uint32_t)b, fc, step, seed, thresh) : 0xFFu;
}

// wq[j][f] (first half of the grid) and wqT[f][j] (second half), f the C8 index; each half writes coalesced
__global__ __launch_bounds__(256) void headn_shadow_kernel(const float* __restrict__ wf, int nc, uint16_t* __restrict__ wq) {
    constexpr int NBLK = NP * CUTF / 256;
    const bool tr = (int)blockIdx.x >= NBLK;
    const int e = ((int)blockIdx.x - (tr ? NBLK : 0)) * 256 + threadIdx.x;
    const int j = tr ? e & (NP - 1) : e / CUTF, f = tr ? e / NP : e & (CUTF - 1);
    const int k = f & 7, fc = f >> 3, plane = fc >> 6, pix = fc & 63;
    const __bf16 h = (__bf16)(j < nc ? wf[(size_t)j * CUTF + (plane * 8 + k) * 64 + pix] : 0.f);
    wq[(tr ? NP * CUTF : 0) + e] = __builtin_bit_cast(uint16_t, h);
}

// one stage of the logits tiles into registers: item = tid + 256 i is row item >> 3, chunk item & 7 of the stage (8
// lanes = 128 contiguous bytes of a row); the cut's chunk is masked here
__device__ __forceinline__ void headn_logits_fetch(u32x4 (&rw)[4], u32x4 (&rc)[4], const uint16_t* __restrict__ cut,
                                                   const uint16_t* __restrict__ wq, int f0, int s0, int b0, int B,
                                                   uint32_t step, uint32_t seed, uint32_t thresh) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = threadIdx.x + 256 * i, row = item >> 3, f = f0 + (item & 7) * 8, b = s0 + row;
        rw[i] = *reinterpret_cast<const u32x4*>(wq + (size_t)row * CUTF + f);
        // a row past the batch reads the last sample's chunk and keeps none of it
        rc[i] = headn_mask8(*reinterpret_cast<const u32x4*>(cut + (size_t)min(b, B - 1) * CUTF + f),
                            b < B ? headn_bits(b0 + b, f >> 3, step, seed, thresh) : 0u);
    }
}

__global__ __launch_bounds__(256) void headn_logits_kernel(const uint16_t* __restrict__ cut, const uint16_t* __restrict__ wq,
                                                           const int* __restrict__ step_ptr, uint32_t seed, uint32_t thresh,
                                                           float* __restrict__ part, int b0, int B) {
    __shared__ __attribute__((aligned(16))) char sm[2 * NP * HN_RST];
    char* const sw = sm;                 // wq tile [128 classes][64 features]
    char* const sc = sm + NP * HN_RST;   // masked cut tile [128 samples][64 features]
    const int tid = threadIdx.x, lane = tid & 63, ig = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int slice = blockIdx.x % HN_SLICES, s0 = (blockIdx.x / HN_SLICES) * HN_TM;
    const uint32_t step = (uint32_t)*step_ptr;
    const int kbase = slice * HN_KSL;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[i][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 rw[4], rc[4];
    headn_logits_fetch(rw, rc, cut, wq, kbase, s0, b0, B, step, seed, thresh);
#pragma unroll 1
    for (int s = 0; s < HN_KSL / HN_KC; ++s) {
        if (s) __syncthreads();   // every wave is done with the previous stage
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = tid + 256 * i, off = (item >> 3) * HN_RST + (item & 7) * 16;
            *reinterpret_cast<u32x4*>(sw + off) = rw[i];
            *reinterpret_cast<u32x4*>(sc + off) = rc[i];
        }
        __syncthreads();
        if (s + 1 < HN_KSL / HN_KC) headn_logits_fetch(rw, rc, cut, wq, kbase + (s + 1) * HN_KC, s0, b0, B, step, seed, thresh);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = *reinterpret_cast<const bf16x8*>(sw + (wm * 64 + i * 16 + ig) * HN_RST + ks * 64 + q * 16);
                bv[i] = *reinterpret_cast<const bf16x8*>(sc + (wn * 64 + i * 16 + ig) * HN_RST + ks * 64 + q * 16);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[u], acc[i][u], 0, 0, 0);
        }
    }
    // D[class 4 q + r][sample ig]: a lane's 4 registers are 4 consecutive classes of one sample
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int b = s0 + wn * 64 + u * 16 + ig;
        if (b < B) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<f32x4*>(part + ((size_t)slice * B + b) * NP + wm * 64 + i * 16 + 4 * q) = acc[i][u];
        }
    }
}

__global__ __launch_bounds__(256) void headn_ce_kernel(const float* __restrict__ part, const float* __restrict__ bf, int nc,
                                                       const int64_t* __restrict__ labels, float keep_scale,
                                                       float grad_scale, float* __restrict__ logits,
                                                       float* __restrict__ loss_i, float* __restrict__ dlogits,
                                                       int* __restrict__ err_flag, int B) {
    __shared__ float zl[16][NP + 4];
    __shared__ float lse_s[16];
    __shared__ int y_s[16];   // the row's label, -1: out of range
    const int tid = threadIdx.x, s = tid >> 4, g = tid & 15;
    const int b = blockIdx.x * 16 + s;
    if (b < B) {
        float S[8];
#pragma unroll
        for (int sl = 0; sl < HN_SLICES; ++sl) {
            const float* p = part + ((size_t)sl * B + b) * NP + g * 8;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                S[e] = sl ? S[e] + lo[e] : lo[e];
                S[4 + e] = sl ? S[4 + e] + hi[e] : hi[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = g * 8 + e;
            if (j < nc) {
                const float z = keep_scale * S[e] + bf[j];
                zl[s][j] = z;
                logits[(size_t)b * nc + j] = z;
            }
        }
    }
    if (!labels) return;
    __syncthreads();
    if (tid < 16) {
        const int bb = blockIdx.x * 16 + tid;
        if (bb < B) {
            float m = -__builtin_inff();
            for (int j = 0; j < nc; ++j) m = fmaxf(m, zl[tid][j]);
            float se = 0.f;
            for (int j = 0; j < nc; ++j) se += expf(zl[tid][j] - m);
            const float lse = m + logf(se);
            const int64_t y = labels[bb];
            const bool ok = y >= 0 && y < nc;
            if (!ok) atomicOr(err_flag, 1);
            loss_i[bb] = ok ? lse - zl[tid][ok ? (int)y : 0] : __builtin_nanf("");
            lse_s[tid] = lse;
            y_s[tid] = ok ? (int)y : -1;
        }
    }
    __syncthreads();
    if (b < B) {
        const float lse = lse_s[s];
        const int y = y_s[s];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = g * 8 + e;
            if (j < nc)
                dlogits[(size_t)b * nc + j] =
                    y >= 0 ? (expf(zl[s][j] - lse) - (j == y ? 1.f : 0.f)) * grad_scale : __builtin_nanf("");
        }
    }
}

// dlq [Bp][128] = bf16(dlogits), zero past the batch and past nc, and its transpose [128][Bp]
__global__ __launch_bounds__(256) void headn_dlq_kernel(const float* __restrict__ dlogits, int nc, int B, int Bp,
                                                        uint16_t* __restrict__ dlq, uint16_t* __restrict__ dlqT) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Bp * NP) return;
    const int b = e / NP, j = e & (NP - 1);
    const __bf16 h = (__bf16)(b < B && j < nc ? dlogits[(size_t)b * nc + j] : 0.f);
    const uint16_t u = __builtin_bit_cast(uint16_t, h);
    dlq[e] = u;
    dlqT[(size_t)j * Bp + b] = u;
}

__global__ __launch_bounds__(256) void headn_dcut_kernel(const uint16_t* __restrict__ wqT, const uint16_t* __restrict__ dlq,
                                                         const int* __restrict__ step_ptr, uint32_t seed, uint32_t thresh,
                                                         float keep_scale, uint16_t* __restrict__ dcut, int b0, int B) {
    const int tid = threadIdx.x, lane = tid & 63, ig = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t step = (uint32_t)*step_ptr;
    const int fbase = blockIdx.x * 256 + wave * 64;   // the wave's first feature (C8 index)
    // M tile (p, t), row i <-> feature fbase + 32 p + 8 (i >> 2) + 4 t + (i & 3): D row 4 q + r of tiles t = 0, 1 is
    // element 4 t + r of chunk fbase / 8 + 4 p + q
    bf16x8 av[2][2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                av[p][t][ks] = *reinterpret_cast<const bf16x8*>(
                    wqT + (size_t)(fbase + 32 * p + 8 * (ig >> 2) + 4 * t + (ig & 3)) * NP + ks * 32 + q * 8);
    const int ntile = (B + 15) / 16;
    int st = blockIdx.y;
    bf16x8 bn[4];
    if (st < ntile) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bn[ks] = *reinterpret_cast<const bf16x8*>(dlq + (size_t)(st * 16 + ig) * NP + ks * 32 + q * 8);
    }
#pragma unroll 1
    for (; st < ntile; st += gridDim.y) {
        const int b = st * 16 + ig;   // rows of dlq are padded to a multiple of 256: always in bounds
        bf16x8 bv[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bv[ks] = bn[ks];
        if (st + (int)gridDim.y < ntile) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                bn[ks] = *reinterpret_cast<const bf16x8*>(dlq + (size_t)((st + gridDim.y) * 16 + ig) * NP + ks * 32 + q * 8);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[p][0][ks], bv[ks], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[p][1][ks], bv[ks], a1, 0, 0, 0);
            }
            if (b < B) {
                const int chunk = (fbase >> 3) + 4 * p + q;
                const uint32_t kb = headn_bits(b0 + b, chunk, step, seed, thresh);
                float o[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o[r] = (kb >> r) & 1u ? a0[r] * keep_scale : 0.f;
                    o[4 + r] = (kb >> (4 + r)) & 1u ? a1[r] * keep_scale : 0.f;
                }
                *reinterpret_cast<uint4*>(dcut + ((size_t)b * NCH + chunk) * 8) =
                    make_uint4(pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7]));
            }
        }
    }
}

// one stage of the wgrad tiles into registers: dlq's transpose rows (item >> 3, 16-byte piece item & 7) and the cut's
// chunk item & 15 of sample item >> 4 of the stage (16 lanes = 256 contiguous bytes of a sample), masked here
__device__ __forceinline__ void headn_wgrad_fetch(u32x4 (&ra)[4], u32x4 (&rb)[4], const uint16_t* __restrict__ cut,
                                                  const uint16_t* __restrict__ dlqT, int Bp, int bs, int fb, int b0, int B,
                                                  uint32_t step, uint32_t seed, uint32_t thresh) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = threadIdx.x + 256 * i;
        ra[i] = *reinterpret_cast<const u32x4*>(dlqT + (size_t)(item >> 3) * Bp + bs + (item & 7) * 8);
        const int b = bs + (item >> 4), fc = fb * 16 + (item & 15);
        // a sample past the batch reads the last sample's chunk and keeps none of it
        rb[i] = headn_mask8(*reinterpret_cast<const u32x4*>(cut + ((size_t)min(b, B - 1) * NCH + fc) * 8),
                            b < B ? headn_bits(b0 + b, fc, step, seed, thresh) : 0u);
    }
}

__global__ __launch_bounds__(256) void headn_wgrad_kernel(const uint16_t* __restrict__ cut, const uint16_t* __restrict__ dlqT,
                                                          int Bp, int nc, const int* __restrict__ step_ptr, uint32_t seed,
                                                          uint32_t thresh, float keep_scale, float* __restrict__ slabs,
                                                          int b0, int B) {
    __shared__ __attribute__((aligned(1024))) char sm[NP * HN_RST + 16 * HN_PST];
    char* const sa = sm;                 // dlq's transpose tile [128 classes][64 samples]
    char* const sb = sm + NP * HN_RST;   // masked cut tile [16 chunks][64 samples (swizzled)][8 features]
    const int tid = threadIdx.x, lane = tid & 63, ig = lane & 15, q = lane >> 4, a = ig >> 2, p = ig & 3;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fb = blockIdx.x, bs = blockIdx.y * HN_SHARE, nb = min(B - bs, HN_SHARE);
    const uint32_t step = (uint32_t)*step_ptr;
    const bool do_db = fb == 0;
    f32x4 acc[8][2], accb[2];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[i][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    accb[0] = accb[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const short one = 0x3F80;  // bf16 1.0
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (__attribute__((ext_vector_type(8))) short){one, one, one, one, one, one, one, one});
    // B fragment of N tile u at K step ks: chunk plane 4 wave + 2 u + (p >> 1), samples 32 ks + 8 q + (a ^ x) (+ 4),
    // 8-byte half p & 1; x = the plane pair's swizzle
    int b_off[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
        b_off[u] = (4 * wave + 2 * u + (p >> 1)) * HN_PST + (8 * q + (a ^ ((2 * wave + u) & 3))) * 16 + (p & 1) * 8;
    u32x4 ra[4], rb[4];
    const int nstage = (nb + HN_KC - 1) / HN_KC;
    headn_wgrad_fetch(ra, rb, cut, dlqT, Bp, bs, fb, b0, B, step, seed, thresh);
#pragma unroll 1
    for (int s = 0; s < nstage; ++s) {
        if (s) __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int item = tid + 256 * i, c = item & 15, smp = item >> 4;
            *reinterpret_cast<u32x4*>(sa + (item >> 3) * HN_RST + (item & 7) * 16) = ra[i];
            *reinterpret_cast<u32x4*>(sb + c * HN_PST + (smp ^ ((c >> 1) & 3)) * 16) = rb[i];
        }
        __syncthreads();
        if (s + 1 < nstage) headn_wgrad_fetch(ra, rb, cut, dlqT, Bp, bs + (s + 1) * HN_KC, fb, b0, B, step, seed, thresh);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 av[8], bv[2];
#pragma unroll
            for (int i = 0; i < 8; ++i) av[i] = *reinterpret_cast<const bf16x8*>(sa + (i * 16 + ig) * HN_RST + ks * 64 + q * 16);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const char* pb = sb + b_off[u] + ks * 32 * 16;
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)pb);
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(pb + 64));
                bv[u] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[u], acc[i][u], 0, 0, 0);
                if (do_db && (i >> 1) == wave)   // wave w sums the samples of M tiles 2 w, 2 w + 1
                    accb[i & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], ones, accb[i & 1], 0, 0, 0);
            }
        }
    }
    // D[class 16 i + 4 q + r][feature ig of N tile u]: chunk fb * 16 + 4 wave + 2 u + (ig >> 3), element ig & 7
    float* slab = slabs + (size_t)blockIdx.y * ((size_t)nc * CUTF + nc);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int fc = fb * 16 + 4 * wave + 2 * u + (ig >> 3), plane = fc >> 6, pix = fc & 63;
        const int ft = (plane * 8 + (ig & 7)) * 64 + pix;   // torch's feature index
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * i + 4 * q + r;
                if (j < nc) slab[(size_t)j * CUTF + ft] = acc[i][u][r] * keep_scale;
            }
    }
    if (do_db && ig == 0) {   // the 16 columns of the ones product are equal: column 0 stores
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * (2 * wave + u) + 4 * q + r;
                if (j < nc) slab[(size_t)nc * CUTF + j] = accb[u][r];
            }
    }
}

// ---------------------------------------------------------------------------- evaluation for nc classes
// slk_eval_row (slk_eval.h) over nc classes, the same expressions in the same order: one thread per sample
__global__ __launch_bounds__(256) void eval_logits_n_kernel(const float* __restrict__ logits, int nc,
                                                            const int64_t* __restrict__ labels, int B,
                                                            float* __restrict__ loss_i, int64_t* __restrict__ pred,
                                                            int* err_flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const float* z = logits + (size_t)i * nc;
    int best = 0;
    float bv = z[0];
    for (int jj = 1; jj < nc; ++jj) {
        const float v = z[jj];
        const bool take = !(bv != bv) && (v > bv || v != v);
        bv = take ? v : bv;
        best = take ? jj : best;
    }
    pred[i] = (int64_t)best;
    if (labels) {
        float m = z[0];
        for (int jj = 1; jj < nc; ++jj) m = fmaxf(m, z[jj]);
        float se = 0.f;
        for (int jj = 0; jj < nc; ++jj) se += expf(z[jj] - m);
        const float lse = m + logf(se);
        const int64_t y = labels[i];
        const bool ok = (y >= 0 && y < nc);
        if (!ok) atomicOr(err_flag, 1);
        loss_i[i] = ok ? (lse - z[ok ? (int)y : 0]) : __builtin_nanf("");
    }
}

// eval_accumulate_kernel's counters and float64 loss sum (the same order) for nc classes. The confusion counts need
// no atomics: thread y < nc owns confusion row y and walks the batch, adding its row's counts in place.
__global__ __launch_bounds__(256) void eval_accumulate_n_kernel(const float* __restrict__ loss_i,
                                                                const int64_t* __restrict__ pred,
                                                                const int64_t* __restrict__ labels, int nc, int B,
                                                                int64_t* __restrict__ acc) {
    __shared__ unsigned int cnt[2];  // correct, bad labels
    __shared__ double wsum[4];
    const int tid = threadIdx.x;
    if (tid < 2) cnt[tid] = 0u;
    __syncthreads();
    double ls = 0.0;
    unsigned int good = 0u, bad = 0u;
    for (int64_t i = tid; i < B; i += 256) {
        const int64_t y = labels[i], p = pred[i];
        if (y >= 0 && y < nc) {
            ls += (double)loss_i[i];
            good += p == y ? 1u : 0u;
        } else {
            bad += 1u;
        }
    }
    if (good) atomicAdd(&cnt[0], good);
    if (bad) atomicAdd(&cnt[1], bad);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) ls += __shfl_xor(ls, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = ls;
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) t += wsum[w];
        acc[0] += (int64_t)B;
        acc[1] += (int64_t)cnt[0];
        acc[2] += (int64_t)cnt[1];
        double* lsum = reinterpret_cast<double*>(acc + 3);
        *lsum = *lsum + t;
    }
    if (tid < nc) {
        int64_t* row = acc + 4 + (size_t)tid * nc;
        for (int i = 0; i < B; ++i) {
            const int64_t p = pred[i];
            if (labels[i] == tid && p >= 0 && p < nc) row[p] += 1;
        }
    }
}

static inline bool headn_nc_ok(int nc) { return nc >= 1 && nc <= NP; }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int slk_wide_headn_nslab(int B) { return B > 0 ? (B + HN_SHARE - 1) / HN_SHARE : 0; }
extern "C" int slk_wide_headn_work(int B) { return B > 0 ? headn_bp(B) * (HN_SLICES * NP) : 0; }

extern "C" int slk_wide_fcn_shadow(const float* wf, int nc, uint16_t* wq, void* stream) {
    SLK_CHECK_ARG(nc >= 0 && nc <= NP);
    if (nc == 0) return 0;
    SLK_CHECK_ARG(wf && wq && aligned16(wq));
    hipLaunchKernelGGL(headn_shadow_kernel, dim3(2 * NP * CUTF / 256), dim3(256), 0, slk_stream(stream), wf, nc, wq);
    return slk_launch_status();
}

extern "C" int slk_wide_headn_fwd(const uint16_t* cut, const uint16_t* wq, const float* bf, int nc, const int64_t* labels,
                                  const int* step, unsigned seed, unsigned keep_threshold, float keep_scale,
                                  float grad_scale, float* logits, float* loss_i, float* dlogits, float* work,
                                  int* err_flag, int b0, int B, void* stream) {
    SLK_CHECK_ARG(B >= 0 && b0 >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(headn_nc_ok(nc) && cut && wq && bf && step && logits && work);
    SLK_CHECK_ARG(aligned16(cut) && aligned16(wq) && aligned16(work));
    // training: labels, loss_i, dlogits and err_flag all given; logits only: all four NULL
    SLK_CHECK_ARG(labels ? (loss_i && dlogits && err_flag) : (!loss_i && !dlogits && !err_flag));
    hipStream_t st = slk_stream(stream);
    hipLaunchKernelGGL(headn_logits_kernel, dim3(HN_SLICES * ((B + HN_TM - 1) / HN_TM)), dim3(256), 0, st, cut, wq, step,
                       seed, keep_threshold, work, b0, B);
    hipLaunchKernelGGL(headn_ce_kernel, dim3((B + 15) / 16), dim3(256), 0, st, (const float*)work, bf, nc, labels,
                       keep_scale, grad_scale, logits, loss_i, dlogits, err_flag, B);
    return slk_launch_status();
}

extern "C" int slk_wide_headn_bwd(const uint16_t* cut, const uint16_t* wq, const float* dlogits, int nc, const int* step,
                                  unsigned seed, unsigned keep_threshold, float keep_scale, uint16_t* dcut, float* slabs,
                                  float* work, int b0, int B, void* stream) {
    SLK_CHECK_ARG(B >= 0 && b0 >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(headn_nc_ok(nc) && cut && wq && dlogits && step && dcut && slabs && work);
    SLK_CHECK_ARG(aligned16(cut) && aligned16(wq) && aligned16(dcut) && aligned16(work));
    hipStream_t st = slk_stream(stream);
    const int Bp = headn_bp(B);
    uint16_t* dlq = reinterpret_cast<uint16_t*>(work);
    uint16_t* dlqT = dlq + (size_t)Bp * NP;
    hipLaunchKernelGGL(headn_dlq_kernel, dim3(Bp * NP / 256), dim3(256), 0, st, dlogits, nc, B, Bp, dlq, dlqT);
    const int ntile = (B + 15) / 16;
    hipLaunchKernelGGL(headn_dcut_kernel, dim3(CUTF / 256, ntile < HN_DCY ? ntile : HN_DCY), dim3(256), 0, st,
                       wq + (size_t)NP * CUTF, (const uint16_t*)dlq, step, seed, keep_threshold, keep_scale, dcut, b0, B);
    hipLaunchKernelGGL(headn_wgrad_kernel, dim3(CUTF / HN_NF, slk_wide_headn_nslab(B)), dim3(256), 0, st, cut,
                       (const uint16_t*)dlqT, Bp, nc, step, seed, keep_threshold, keep_scale, slabs, b0, B);
    return slk_launch_status();
}

extern "C" int slk_eval_logits_n(const float* logits, int nc, const int64_t* labels, int B, float* loss_i, int64_t* pred,
                                 int* err_flag, void* stream) {
    SLK_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(headn_nc_ok(nc) && logits && pred);
    SLK_CHECK_ARG(labels ? (loss_i && err_flag) : (!loss_i && !err_flag));
    hipLaunchKernelGGL(eval_logits_n_kernel, dim3((B + 255) / 256), dim3(256), 0, slk_stream(stream), logits, nc, labels,
                       B, loss_i, pred, err_flag);
    return slk_launch_status();
}

extern "C" int slk_eval_accumulate_n(const float* loss_i, const int64_t* pred, const int64_t* labels, int nc, int B,
                                     int64_t* acc, void* stream) {
    SLK_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(headn_nc_ok(nc) && loss_i && pred && labels && acc && ((uintptr_t)acc & 7) == 0);
    hipLaunchKernelGGL(eval_accumulate_n_kernel, dim3(1), dim3(256), 0, slk_stream(stream), loss_i, pred, labels, nc, B,
                       acc);
    return slk_launch_status();
}
