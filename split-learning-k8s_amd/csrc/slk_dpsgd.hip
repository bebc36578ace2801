// slk_dpsgd.hip — DP-SGD on the K5 client (include/slk.h, "DP-SGD on the K5 client"): the squared norm of every
// sample's own client gradient, the clip coefficient from it, and the Gaussian noise row of the optimizer's slab sets.
//
// slk_wide_grad_sqnorm. The sparse weight gradients (slk_wide.hip) sum over samples inside their K shares, so a
// sample's own dW_b never exists. Here a workgroup owns ONE sample and a 128-co x 64-ci block of its dW (all 9 taps):
// GEMM M = co, N = (tap, ci), K = the sample's pixels, bf16 operands, v_mfma_f32_16x16x32_bf16. The sample is walked in
// bands of 256 pixels (conv3: the whole 16 x 16 image, conv2: 8 rows of 32) staged once each in LDS:
//   A  the routed dY of the band, [128 co][256 px] bf16, rows 528 B apart (16 lanes x 16 B of one read cover all 64
//      banks). It is built from the pooled gradient and its routing codes while staging: a pooled element writes the
//      2 x 2 window it owns (its value at the code's position, zeros elsewhere), two 4-byte stores, so the band is
//      written completely and no unpooled gradient exists anywhere else. A lane's A fragment (8 consecutive pixels
//      of one co) is one aligned 16-byte read.
//   B  the band's input halo tile in the C8 layout of HBM, [8 chunks][(rows + 2) x (W + 2) px][8 ci], chunk planes
//      a multiple of 256 B + 64 apart. A lane's B fragment (8 consecutive pixels of one ci, shifted by the tap) is two
//      ds_read_b64_tr_b16 transposed reads, as in the sparse wgrads.
// Wave (wm, wn) of 8 holds co 64 wm .. + 63 x ci 16 wn .. + 15 x 9 taps: 4 x 9 accumulator tiles (144 VGPRs) that
// live across the bands; per K32 step 4 A reads, 18 transposed reads, 36 MFMAs (+ 1 against a ones fragment for db in
// the workgroups of ci block 0). The epilogue never stores a tile: every lane squares and adds its 144 (+ 4)
// accumulator elements in f32, in the order slk.h documents, the wave and the workgroup reduce in fixed order, and
// one float per (sample, block) lands in the caller's work buffer. conv1 (M = 64, N = 27 + the bias column, K = 1024)
// is one workgroup of 4 waves per sample on the same MFMA: da1m's band through transposed reads, the im2col band of
// bf16(x) built in LDS. No atomics; every partial is a fixed function of its own sample.
#include "slk_common.h"

#pragma clang fp contract(off)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {
constexpr int NPART = 6;       // partials of one sample: [conv1 | conv2 | conv3 blocks (cob, cib) = 00, 01, 10, 11]
constexpr int BPX = 256;       // pixels of a band
constexpr int AST = 2 * BPX + 16;   // bytes between two co rows of A

template <int CI_, int CO_, int HW_, int SLOT_>
struct SqCfg {
    static constexpr int CI = CI_, CO = CO_, HW = HW_, SLOT = SLOT_;
    static constexpr int COB = 128, CIB = 64;
    static constexpr int NCIB = CI / CIB, NBLK = (CO / COB) * NCIB;
    static constexpr int TR = BPX / HW, NBAND = HW / TR;     // rows of a band, bands of a sample
    static constexpr int PH = HW / 2, PR = TR / 2;           // pooled width, pooled rows of a band
    static constexpr int PW = HW + 2, NP = (TR + 2) * PW;    // the halo tile
    static constexpr int NPI = (NP + 11) / 16 * 16 + 4;      // plane stride in pixels: 64 mod 256 bytes
    static constexpr int A_BYTES = COB * AST, IN_BYTES = (CIB / 8) * NPI * 16;
    static_assert(PR * PH == 64 && NPI >= NP && NPI % 16 == 4, "band geometry");
};
using Sq2 = SqCfg<64, 128, 32, 1>;    // dW2_b: a1_b x (dp2_b routed by code2_b)
using Sq3 = SqCfg<128, 256, 16, 2>;   // dW3_b: p2_b x (dcut_b routed by code3_b)

// The end of every kernel here: lane totals -> one float. The xor butterfly inside the wave (offsets 32, 16, .. 1),
// lane 0 of wave w leaves its sum in red[w], thread 0 adds red[0 .. NW - 1] in ascending order from red[0].
template <int NW>
__device__ __forceinline__ void block_partial(float t, float* red, float* out) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t = t + __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = red[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) s = s + red[w];
        *out = s;
    }
}

template <class C>
__global__ __launch_bounds__(512, 1) void grad_sqnorm_kernel(const uint16_t* __restrict__ dc,
                                                             const uint8_t* __restrict__ dcode,
                                                             const uint16_t* __restrict__ in,
                                                             float* __restrict__ work) {
    __shared__ __attribute__((aligned(1024))) char smem[C::A_BYTES + C::IN_BYTES];
    __shared__ float red[8];
    char* const sa = smem;
    char* const sb = smem + C::A_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int n = blockIdx.x / C::NBLK, blk = blockIdx.x - n * C::NBLK;
    const int cob = blk / C::NCIB, cib = blk - cob * C::NCIB;
    const bool do_db = cib == 0;
    const int q = lane >> 4, ig = lane & 15, a = ig >> 2, p = ig & 3;

    f32x4 acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 9; ++u) acc[i][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 accb = f32x4{0.f, 0.f, 0.f, 0.f};
    const short one = 0x3F80;  // bf16 1.0
    const bf16x8 ones = __builtin_bit_cast(bf16x8, (__attribute__((ext_vector_type(8))) short){one, one, one, one, one, one, one, one});

    // A fragment of M tile i at K step s: row (64 wm + 16 i + ig), pixels 32 s + 8 q .. + 7
    const int a_off = (wm * 64 + ig) * AST + q * 16;
    // B fragment at K step s, tap (ky, kx): band pixel 32 s + 8 q + a (+ 4), chunk plane 2 wn + (p >> 1), half p & 1
    const int b_y = C::HW == 32 ? 0 : (q >> 1), b_x = (C::HW == 32 ? 8 * q : 8 * (q & 1)) + a;
    const int b_off = ((2 * wn + (p >> 1)) * C::NPI + b_y * C::PW + b_x) * 16 + (p & 1) * 8;
    constexpr int B_STEP = (C::HW == 32 ? C::PW : 2 * C::PW) * 16;   // a K step is one row of 32 or two rows of 16

#pragma unroll 1
    for (int band = 0; band < C::NBAND; ++band) {
        if (band) __syncthreads();   // every wave is done with the previous band
        // A: 16 chunk planes x 64 pooled pixels = 1,024 chunks (8 co each), two per thread
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int item = tid + 512 * k, c = item >> 6, rem = item & 63, pr = rem / C::PH, px = rem - pr * C::PH;
            const size_t idx = ((size_t)(n * (C::CO / 8) + cob * 16 + c) * C::PH + band * C::PR + pr) * C::PH + px;
            const uint4 v = *reinterpret_cast<const uint4*>(dc + idx * 8);
            const uint2 cw = *reinterpret_cast<const uint2*>(dcode + idx * 8);
            const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
            char* dst = sa + (c * 8) * AST + ((2 * pr) * C::HW + 2 * px) * 2;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t val = (vw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                const uint32_t code = ((e < 4 ? cw.x : cw.y) >> (8 * (e & 3))) & 0xFFu;
                const uint32_t top = code == 0u ? val : code == 1u ? val << 16 : 0u;
                const uint32_t bot = code == 2u ? val : code == 3u ? val << 16 : 0u;
                *reinterpret_cast<uint32_t*>(dst + e * AST) = top;
                *reinterpret_cast<uint32_t*>(dst + e * AST + C::HW * 2) = bot;
            }
        }
        // B: 8 chunk planes of the halo tile, zeros outside the image
        for (int item = tid; item < 8 * C::NP; item += 512) {
            const int c = item / C::NP, P = item - c * C::NP, ry = P / C::PW, rx = P - ry * C::PW;
            const int y = band * C::TR - 1 + ry, x = rx - 1;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (y >= 0 && y < C::HW && x >= 0 && x < C::HW)
                v = *reinterpret_cast<const uint4*>(in + (((size_t)(n * (C::CI / 8) + cib * 8 + c) * C::HW + y) * C::HW + x) * 8);
            *reinterpret_cast<uint4*>(sb + (c * C::NPI + P) * 16) = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int s = 0; s < BPX / 32; ++s) {
            bf16x8 av[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const bf16x8*>(sa + a_off + i * 16 * AST + s * 64);
            if (do_db) {   // wave (wm, wn) sums the pixels of M tile wn of its 4
                bf16x8 adb = av[0];
#pragma unroll
                for (int i = 1; i < 4; ++i) adb = wn == i ? av[i] : adb;
                accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adb, ones, accb, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 9; ++u) {
                const char* pb = sb + b_off + s * B_STEP + ((u / 3) * C::PW + (u % 3)) * 16;
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)pb);
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(pb + 64));
                const bf16x8 bv = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv, acc[i][u], 0, 0, 0);
            }
        }
    }
    // the lane's squares: M tile, then tap, then accumulator register, each product rounded, added one at a time
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 9; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) t = t + acc[i][u][r] * acc[i][u][r];
    if (do_db && ig == 0) {   // the 16 columns of the ones product are equal: column 0 counts
#pragma unroll
        for (int r = 0; r < 4; ++r) t = t + accb[r] * accb[r];
    }
    block_partial<8>(t, red, work + (size_t)n * NPART + C::SLOT + blk);
}

// conv1: dW1_b [64][27] | db1_b [64] as one 64 x 32 product (column 27 is the constant 1: db; 28 .. 31 are zero).
constexpr int C1_NPXP = BPX + 4;                   // da1m band plane stride in pixels: 64 mod 256 bytes
constexpr int C1_A = 8 * C1_NPXP * 16, C1_B = 32 * AST;

__global__ __launch_bounds__(256) void grad_sqnorm_conv1_kernel(const float* __restrict__ x,
                                                                const uint16_t* __restrict__ da1m,
                                                                float* __restrict__ work) {
    __shared__ __attribute__((aligned(1024))) char smem[C1_A + C1_B];
    __shared__ float red[4];
    char* const sa = smem;
    char* const sb = smem + C1_A;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.x;
    const int q = lane >> 4, ig = lane & 15, a = ig >> 2, p = ig & 3;
    const float* img = x + (size_t)n * 3 * 1024;
    // wave w owns co 16 w .. + 15: chunk planes 2 w, 2 w + 1
    const int a_off = ((2 * wave + (p >> 1)) * C1_NPXP + 8 * q + a) * 16 + (p & 1) * 8;
    const int b_off = ig * AST + q * 16;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
    for (int band = 0; band < 4; ++band) {
        if (band) __syncthreads();
        // da1m's band: 8 planes x 256 pixels x 16 B, 8 chunks per thread
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int item = tid + 256 * k, c = item >> 8, px = item & 255;
            *reinterpret_cast<uint4*>(sa + (c * C1_NPXP + px) * 16) =
                *reinterpret_cast<const uint4*>(da1m + ((size_t)(n * 8 + c) * 1024 + band * BPX + px) * 8);
        }
        // the im2col band [32 columns][256 px] of bf16(x): thread = pixel
        {
            const int y = band * 8 + (tid >> 5), xx = tid & 31;
#pragma unroll
            for (int col = 0; col < 32; ++col) {
                float g = col == 27 ? 1.f : 0.f;
                if (col < 27) {
                    const int ci = col / 9, ky = (col % 9) / 3, kx = col % 3;
                    const int yy = y + ky - 1, xc = xx + kx - 1;
                    if (yy >= 0 && yy < 32 && xc >= 0 && xc < 32) g = img[ci * 1024 + yy * 32 + xc];
                }
                *reinterpret_cast<__bf16*>(sb + col * AST + tid * 2) = (__bf16)g;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BPX / 32; ++s) {
            const char* pa = sa + a_off + s * 32 * 16;
            const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)pa);
            const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(pa + 64));
            const bf16x8 av = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int kf = 0; kf < 2; ++kf) {
                const bf16x8 bv = *reinterpret_cast<const bf16x8*>(sb + b_off + kf * 16 * AST + s * 64);
                acc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[kf], 0, 0, 0);
            }
        }
    }
    float t = 0.f;
#pragma unroll
    for (int kf = 0; kf < 2; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) t = t + acc[kf][r] * acc[kf][r];
    block_partial<4>(t, red, work + (size_t)n * NPART);
}

// stats[b] = (norm, coef): the sample's partials added in ascending order in float64, rounded to f32 once.
__global__ __launch_bounds__(256) void dp_coef_kernel(const float* __restrict__ work, int n, float unit,
                                                      const float* __restrict__ max_norm, float* __restrict__ stats) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NPART; ++j) s = s + (double)work[(size_t)b * NPART + j];
    const float norm = unit * sqrtf((float)s);
    const float qv = *max_norm / (norm + 1e-6f);
    const f32x2 pair = {norm, qv < 1.f ? qv : 1.f};   // a compare: a NaN norm gives 1
    *reinterpret_cast<f32x2*>(stats + 2 * (size_t)b) = pair;
}

__global__ __launch_bounds__(256) void dp_noise_kernel(float* __restrict__ out, int n, uint32_t i0,
                                                       const float* __restrict__ sigma,
                                                       const float* __restrict__ max_norm, float grad_scale,
                                                       uint32_t seed, const int* __restrict__ step) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float sg = *sigma;
    float sd = sg * *max_norm;
    sd = sd * grad_scale;
    const uint32_t h0 = lowbias32((i0 + (uint32_t)i) * 0x9E3779B1u + (uint32_t)*step * 0x85EBCA77u + seed * 0xC2B2AE3Du);
    const uint32_t h1 = lowbias32(h0 + 0x9E3779B9u);
    const float u1 = ((float)(h0 >> 9) + 0.5f) * 0x1p-23f, u2 = (float)(h1 >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.f * logf(u1));
    const float z = rad * cospif(2.f * u2);
    out[i] = sg == 0.f ? 0.f : sd * z;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" int slk_wide_grad_sqnorm_work(int B) { return B >= 0 && B <= 0x7FFFFFFF / NPART ? NPART * B : 0; }

extern "C" int slk_wide_grad_sqnorm(const float* x, const uint16_t* da1m, const uint16_t* a1, const uint16_t* dp2,
                                    const uint8_t* code2, const uint16_t* p2, const uint16_t* dcut,
                                    const uint8_t* code3, float* work, int layers, int B, void* stream) {
    SLK_CHECK_ARG(B >= 0 && B <= 0x7FFFFFFF / 64 && layers >= 0 && layers <= 7);
    if (B == 0) return 0;
    SLK_CHECK_ARG(x && da1m && a1 && dp2 && code2 && p2 && dcut && code3 && work);
    SLK_CHECK_ARG(aligned(x, 4) && aligned(da1m, 16) && aligned(a1, 16) && aligned(dp2, 16) && aligned(code2, 8) &&
                  aligned(p2, 16) && aligned(dcut, 16) && aligned(code3, 8) && aligned(work, 4));
    hipStream_t st = slk_stream(stream);
    if (layers & 1) grad_sqnorm_conv1_kernel<<<(unsigned)B, 256, 0, st>>>(x, da1m, work);
    if (layers & 2) grad_sqnorm_kernel<Sq2><<<(unsigned)(B * Sq2::NBLK), 512, 0, st>>>(dp2, code2, a1, work);
    if (layers & 4) grad_sqnorm_kernel<Sq3><<<(unsigned)(B * Sq3::NBLK), 512, 0, st>>>(dcut, code3, p2, work);
    return slk_launch_status();
}

extern "C" int slk_dp_coef(const float* work, int n, float unit, const float* max_norm, float* stats, void* stream) {
    SLK_CHECK_ARG(n >= 0 && n <= 0x7FFFFFFF / NPART);
    if (n == 0) return 0;
    SLK_CHECK_ARG(work && max_norm && stats && aligned(work, 4) && aligned(max_norm, 4) && aligned(stats, 8));
    dp_coef_kernel<<<(unsigned)((n + 255) / 256), 256, 0, slk_stream(stream)>>>(work, n, unit, max_norm, stats);
    return slk_launch_status();
}

extern "C" int slk_dp_noise(float* out, int n, int64_t i0, const float* sigma, const float* max_norm,
                            float grad_scale, unsigned seed, const int* step, void* stream) {
    SLK_CHECK_ARG(n >= 0 && i0 >= 0 && i0 + (int64_t)n <= ((int64_t)1 << 32));
    if (n == 0) return 0;
    SLK_CHECK_ARG(out && sigma && max_norm && step && aligned(out, 4) && aligned(sigma, 4) && aligned(max_norm, 4) &&
                  aligned(step, 4));
    dp_noise_kernel<<<(unsigned)((n + 255) / 256), 256, 0, slk_stream(stream)>>>(out, n, (uint32_t)i0, sigma, max_norm,
                                                                               grad_scale, seed, step);
    return slk_launch_status();
}
