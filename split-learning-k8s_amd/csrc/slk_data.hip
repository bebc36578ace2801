// slk_data.hip — the batch loaders as one HBM-resident gather each: slk_mnist_batch (K2) and
// slk_image_batch (K5's CIFAR-10 path with crop + flip augmentation, and MNIST with a crop), plus
// slk_image_batch_mix, the same gather with CutMix and mixed labels, and slk_image_batch_blend, which draws the box
// side or a MixUp weight from a Beta(alpha, alpha) quantile table per sample.
//
// The reference builds batches with DataLoader(train_dataset, batch_size=64, shuffle=True)
// (client_part.py:98) over torchvision MNIST with ToTensor() + Normalize((0.1307,), (0.3081,))
// (client_part.py:61-64): per sample, u8 -> float32 /255, then (v - mean) / std, all in float32.
// Here the whole u8 dataset (47 MB for the 60k training set) stays resident in HBM, and a batch
// is one launch: gather the shuffled rows, normalise, write x [B,1,28,28] f32 and y [B] i64.
// Division is IEEE-correct (hipcc's default for f32 '/'), so x is bit-identical to the torchvision
// transform. HBM-bound: 784 B read + 3,136 B written per sample.
#include "slk_common.h"

namespace {
constexpr int IMG = 28 * 28;        // bytes per image
constexpr int CHUNKS = IMG / 4;     // 196 u32 words per image
}

__global__ __launch_bounds__(256) void mnist_batch_kernel(const uint32_t* __restrict__ images,
                                                          const uint8_t* __restrict__ labels,
                                                          int n_images, const int64_t* __restrict__ idx,
                                                          int B, float mean, float stdv,
                                                          float4* __restrict__ x, int64_t* __restrict__ y,
                                                          int* __restrict__ err) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= B * CHUNKS) return;
    const int s = g / CHUNKS, c = g - s * CHUNKS;
    int64_t i = idx[s];
    if (i < 0 || i >= n_images) {     // out-of-range index: flag it, read row 0 instead of faulting
        if (c == 0 && err) *err = 1;
        i = 0;
    }
    const uint32_t w = images[(size_t)i * CHUNKS + c];
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = (float)((w >> (8 * k)) & 0xffu) / 255.0f;   // ToTensor
        v[k] = (t - mean) / stdv;                                     // Normalize
    }
    x[g] = make_float4(v[0], v[1], v[2], v[3]);
    if (c == 0) y[s] = (int64_t)labels[i];
}

extern "C" int slk_mnist_batch(const uint8_t* images, const uint8_t* labels, int n_images,
                               const int64_t* idx, int B, float mean, float stdv, float* x,
                               int64_t* y, int* err_flag, void* stream) {
    SLK_CHECK_ARG(B >= 0 && n_images > 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(images && labels && idx && x && y);
    SLK_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)x & 15) == 0);
    const int total = B * CHUNKS;
    mnist_batch_kernel<<<(total + 255) / 256, 256, 0, slk_stream(stream)>>>(
        reinterpret_cast<const uint32_t*>(images), labels, n_images, idx, B, mean, stdv,
        reinterpret_cast<float4*>(x), y, err_flag);
    return slk_launch_status();
}

// ---------------------------------------------------------------------------------- slk_image_batch
// RandomCrop(H, padding=pad, fill 0) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize(mean[C], std[C])
// of the rows idx[b] of a u8 dataset [N][C][H][W], one launch per batch. The per-sample draws come from
// lowbias32 keyed on the DATASET index (slk.h), so they do not depend on the batch a sample lands in.
//
// A quad is four consecutive output pixels of one row, stored as one aligned float4. A thread makes
// U quads of one sample, 1/U of the sample apart (the lanes of a wave stay on consecutive quads), so the
// sample's draws are hashed once and 2U loads are in flight per thread. A quad's four
// source bytes are consecutive too (read backwards when flipped), start at any byte offset and may hang
// over either edge of the row: the thread loads the two aligned words around them, v_alignbyte cuts the
// four bytes out, v_perm reverses them for a flip, and the columns outside the row are masked to the
// padding value 0. A word index is clamped into the dataset BEFORE the load; a clamped word only ever
// supplies masked columns, since a byte in a column inside the row lies inside the dataset and so does
// its word. Rows above or below the image, and quads entirely beside it, issue no load.
// HBM-bound like mnist_batch: C*H*W bytes read, 4*C*H*W written per sample.

// Quads per thread (A/B switches): 4 for CIFAR; 1 for MNIST, whose B = 4096 batch has too few quads to fill
// the device four to a thread.
#ifndef SLK_IMAGE_QUADS_CIFAR
#define SLK_IMAGE_QUADS_CIFAR 4
#endif
#ifndef SLK_IMAGE_QUADS_MNIST
#define SLK_IMAGE_QUADS_MNIST 1
#endif

namespace {
constexpr int IMAGE_MAX_C = 3;
constexpr int IMAGE_MAX_PAD = 8;
struct ImageNorm {
    float mean[IMAGE_MAX_C], stdv[IMAGE_MAX_C];
};
}  // namespace

template <int C, int H, int W, int U>
__global__ __launch_bounds__(256) void image_batch_kernel(const uint32_t* __restrict__ words,
                                                          const uint8_t* __restrict__ labels, int n_images,
                                                          const int64_t* __restrict__ idx, int B, ImageNorm nrm,
                                                          int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                                          float4* __restrict__ x, int64_t* __restrict__ y,
                                                          int* __restrict__ err) {
    static_assert(W % 4 == 0 && (C * H * W) % 4 == 0 && C <= IMAGE_MAX_C, "quads of one row, whole words per image");
    constexpr int QW = W / 4;            // quads per row
    constexpr int QS = C * H * QW;       // quads per sample
    constexpr int TS = QS / U;           // threads per sample; thread r0 makes quads r0 + u * TS
    static_assert(QS % U == 0, "every thread of a sample makes U quads");
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * TS) return;
    const int s = (int)(t / TS), r0 = (int)(t - (int64_t)s * TS);
    int64_t i = idx[s];
    if (i < 0 || i >= n_images) {        // out-of-range index: flag it, read row 0 (with row 0's draws)
        if (r0 == 0 && err) *err = 1;
        i = 0;
    }
    // loaded by every thread (one address per sample) and stored last by one: a load under `r0 == 0` would be
    // waited for at the end of its branch, in front of the pixel loads
    const int64_t label = (int64_t)labels[i];

    const uint32_t h0 = lowbias32((uint32_t)i * 0x9E3779B1u + epoch * 0x85EBCA77u + seed * 0xC2B2AE3Du);
    const uint32_t h1 = lowbias32(h0 + 0x9E3779B9u);
    const uint32_t h2 = lowbias32(h1 + 0x9E3779B9u);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    const int dy = (int)(((uint64_t)h0 * span) >> 32), dx = (int)(((uint64_t)h1 * span) >> 32);
    const bool flip = flip_enabled && (h2 >> 31);
    const int64_t last = (int64_t)n_images * (C * H * W / 4) - 1;   // the dataset's last word

    // Quad u: the four source bytes are columns x0 .. x0+3 of row ys, output pixel k taking x0+k (x0+3-k if
    // flipped). All loads of the thread are issued before the first is used: the launch is bound by how many
    // loads are in flight, not by arithmetic.
    int x0[U], sh[U];
    uint32_t lo[U], hi[U];
    bool ld[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW), yo = (r / QW) % H, q = r % QW;
        const int ys = yo + dy - pad;
        x0[u] = (flip ? W - 4 - 4 * q : 4 * q) + dx - pad;
        ld[u] = (unsigned)ys < (unsigned)H && x0[u] > -4 && x0[u] < W;
        lo[u] = hi[u] = 0;
        sh[u] = 0;
        if (ld[u]) {
            const int64_t a = (((int64_t)i * C + c) * H + ys) * W + x0[u];     // byte address, may be < 0
            const int64_t wi = a >> 2;
            sh[u] = (int)(a & 3);
            lo[u] = words[min(max(wi, (int64_t)0), last)];
            hi[u] = words[min(max(wi + 1, (int64_t)0), last)];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW);
        uint32_t w = 0;
        if (ld[u]) {
            w = __builtin_amdgcn_alignbyte(hi[u], lo[u], (uint32_t)sh[u]);
            uint32_t keep = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) keep |= (unsigned)(x0[u] + k) < (unsigned)W ? 0xffu << (8 * k) : 0u;
            w &= keep;
            if (flip) w = __builtin_amdgcn_perm(w, w, 0x00010203u);             // byte k <- byte 3-k
        }
        // selects, not an index: a per-lane index into the by-value struct would move it to scratch
        const float mean = c == 0 ? nrm.mean[0] : c == 1 ? nrm.mean[1] : nrm.mean[2];
        const float stdv = c == 0 ? nrm.stdv[0] : c == 1 ? nrm.stdv[1] : nrm.stdv[2];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float f = (float)((w >> (8 * k)) & 0xffu) / 255.0f;   // ToTensor
            v[k] = (f - mean) / stdv;                                     // Normalize
        }
        x[(int64_t)s * QS + r] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (r0 == 0) y[s] = label;
}

template <int C, int H, int W, int U>
static int image_batch_launch(const uint8_t* images, const uint8_t* labels, int n_images, const int64_t* idx, int B,
                              const ImageNorm& nrm, int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                              float* x, int64_t* y, int* err_flag, void* stream) {
    const int64_t total = (int64_t)B * (C * H * (W / 4) / U);
    SLK_CHECK_ARG((total + 255) / 256 <= 0x7fffffff);
    image_batch_kernel<C, H, W, U><<<(unsigned)((total + 255) / 256), 256, 0, slk_stream(stream)>>>(
        reinterpret_cast<const uint32_t*>(images), labels, n_images, idx, B, nrm, pad, flip_enabled, seed, epoch,
        reinterpret_cast<float4*>(x), y, err_flag);
    return slk_launch_status();
}

extern "C" int slk_image_batch(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                               const int64_t* idx, int B, const float* mean, const float* stdv, int pad,
                               int flip_enabled, uint32_t seed, uint32_t epoch, float* x, int64_t* y,
                               int* err_flag, void* stream) {
    const bool cifar = C == 3 && H == 32 && W == 32, mnist = C == 1 && H == 28 && W == 28;
    SLK_CHECK_ARG(cifar || mnist);
    SLK_CHECK_ARG(B >= 0 && n_images > 0 && pad >= 0 && pad <= IMAGE_MAX_PAD);
    if (B == 0) return 0;
    SLK_CHECK_ARG(images && labels && idx && x && y && mean && stdv);
    SLK_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)x & 15) == 0);
    ImageNorm nrm = {};
    for (int c = 0; c < C; ++c) {
        nrm.mean[c] = mean[c];
        nrm.stdv[c] = stdv[c];
    }
    if (cifar)
        return image_batch_launch<3, 32, 32, SLK_IMAGE_QUADS_CIFAR>(images, labels, n_images, idx, B, nrm, pad, flip_enabled, seed, epoch, x,
                                             y, err_flag, stream);
    return image_batch_launch<1, 28, 28, SLK_IMAGE_QUADS_MNIST>(images, labels, n_images, idx, B, nrm, pad, flip_enabled, seed, epoch, x, y,
                                         err_flag, stream);
}

// ---------------------------------------------------------------------------------- slk_image_batch_mix
// slk_image_batch with CutMix (Yun et al. 2019, lam ~ Beta(1, 1)): batch position s shows sample i = idx[s] with a
// box of sample i2 = idx2[s] pasted in, each under its OWN crop and flip draws, and y[s] is the mixed label
// a | b << 8 | bits(wb) << 32 (slk.h). The box comes from the primary sample's hash chain continued (h3..h7), all
// in integers. The selection is made on the u8 pixels, then the same ToTensor / Normalize arithmetic runs.
//
// The quad gather is image_batch_kernel's, once per source: a quad on a row outside the box, or with its four
// columns all outside it, loads only source i; a quad wholly inside loads only source i2; only the at most two
// quads of a box row that straddle an edge load both, and take their bytes by a mask AFTER each source's own
// alignbyte / column mask / flip permute (byte k of either word is output pixel k by then). All of a thread's
// loads are issued before the first use. The clamped-word argument holds per source: each source's word indices
// are clamped into the dataset before the load, and a clamped word only ever supplies columns that source masks.
namespace {
struct ImageDraws {
    int dy, dx;
    bool flip;
    uint32_t h2;
};
__device__ __forceinline__ ImageDraws image_draws(int64_t i, uint32_t seed, uint32_t epoch, int pad, int flip_enabled) {
    const uint32_t h0 = lowbias32((uint32_t)i * 0x9E3779B1u + epoch * 0x85EBCA77u + seed * 0xC2B2AE3Du);
    const uint32_t h1 = lowbias32(h0 + 0x9E3779B9u);
    const uint32_t h2 = lowbias32(h1 + 0x9E3779B9u);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    ImageDraws d;
    d.dy = (int)(((uint64_t)h0 * span) >> 32);
    d.dx = (int)(((uint64_t)h1 * span) >> 32);
    d.flip = flip_enabled && (h2 >> 31);
    d.h2 = h2;
    return d;
}
// the four source bytes of one quad after alignbyte, the column mask and the flip permute: byte k = output pixel k
__device__ __forceinline__ uint32_t quad_bytes(uint32_t lo, uint32_t hi, int sh, int x0, int W, bool flip) {
    uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
    uint32_t keep = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) keep |= (unsigned)(x0 + k) < (unsigned)W ? 0xffu << (8 * k) : 0u;
    w &= keep;
    return flip ? __builtin_amdgcn_perm(w, w, 0x00010203u) : w;
}
}  // namespace

template <int C, int H, int W, int U>
__global__ __launch_bounds__(256) void image_batch_mix_kernel(const uint32_t* __restrict__ words,
                                                              const uint8_t* __restrict__ labels, int n_images,
                                                              const int64_t* __restrict__ idx,
                                                              const int64_t* __restrict__ idx2, int B, ImageNorm nrm,
                                                              int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                                              uint64_t apply_below, float4* __restrict__ x,
                                                              int64_t* __restrict__ y, int* __restrict__ err) {
    static_assert(W % 4 == 0 && (C * H * W) % 4 == 0 && C <= IMAGE_MAX_C, "quads of one row, whole words per image");
    constexpr int QW = W / 4, QS = C * H * QW, TS = QS / U;
    static_assert(QS % U == 0, "every thread of a sample makes U quads");
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * TS) return;
    const int s = (int)(t / TS), r0 = (int)(t - (int64_t)s * TS);
    int64_t i = idx[s], i2 = idx2[s];
    if (i < 0 || i >= n_images) {        // out-of-range index: flag it, read row 0 (with row 0's draws)
        if (r0 == 0 && err) *err = 1;
        i = 0;
    }
    if (i2 < 0 || i2 >= n_images) {      // the partner likewise
        if (r0 == 0 && err) *err = 1;
        i2 = 0;
    }
    // both labels loaded by every thread and stored last by one (see image_batch_kernel)
    const int64_t la = (int64_t)labels[i], lb = (int64_t)labels[i2];

    const ImageDraws da = image_draws(i, seed, epoch, pad, flip_enabled);
    const ImageDraws db = image_draws(i2, seed, epoch, pad, flip_enabled);
    // the box: the primary sample's chain continued
    const uint32_t h3 = lowbias32(da.h2 + 0x9E3779B9u), h4 = lowbias32(h3 + 0x9E3779B9u);
    const uint32_t h5 = lowbias32(h4 + 0x9E3779B9u), h6 = lowbias32(h5 + 0x9E3779B9u);
    const uint32_t h7 = lowbias32(h6 + 0x9E3779B9u);
    const bool apply = (uint64_t)h3 < apply_below;
    const int side = max((int)(((uint64_t)h4 * H) >> 32), (int)(((uint64_t)h5 * H) >> 32)), half = side / 2;
    const int cy = (int)(((uint64_t)h6 * H) >> 32), cx = (int)(((uint64_t)h7 * W) >> 32);
    const int y1 = min(max(cy - half, 0), H), y2 = apply ? min(max(cy + half, 0), H) : y1;   // unapplied: empty
    const int x1 = min(max(cx - half, 0), W), x2 = min(max(cx + half, 0), W);
    const int area = (y2 - y1) * (x2 - x1);
    const int64_t last = (int64_t)n_images * (C * H * W / 4) - 1;   // the dataset's last word

    int xa[U], xb[U], sa[U], sb[U];
    uint32_t loa[U], hia[U], lob[U], hib[U], msk[U];   // msk: bytes of the quad that lie inside the box
    bool lda[U], ldb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW), yo = (r / QW) % H, q = r % QW;
        uint32_t m = 0;
        if (yo >= y1 && yo < y2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= (4 * q + k >= x1 && 4 * q + k < x2) ? 0xffu << (8 * k) : 0u;
        }
        msk[u] = m;
        const int ysa = yo + da.dy - pad, ysb = yo + db.dy - pad;
        xa[u] = (da.flip ? W - 4 - 4 * q : 4 * q) + da.dx - pad;
        xb[u] = (db.flip ? W - 4 - 4 * q : 4 * q) + db.dx - pad;
        lda[u] = m != 0xffffffffu && (unsigned)ysa < (unsigned)H && xa[u] > -4 && xa[u] < W;
        ldb[u] = m != 0u && (unsigned)ysb < (unsigned)H && xb[u] > -4 && xb[u] < W;
        loa[u] = hia[u] = lob[u] = hib[u] = 0;
        sa[u] = sb[u] = 0;
        if (lda[u]) {
            const int64_t a = (((int64_t)i * C + c) * H + ysa) * W + xa[u];    // byte address, may be < 0
            const int64_t wi = a >> 2;
            sa[u] = (int)(a & 3);
            loa[u] = words[min(max(wi, (int64_t)0), last)];
            hia[u] = words[min(max(wi + 1, (int64_t)0), last)];
        }
        if (ldb[u]) {
            const int64_t a = (((int64_t)i2 * C + c) * H + ysb) * W + xb[u];
            const int64_t wi = a >> 2;
            sb[u] = (int)(a & 3);
            lob[u] = words[min(max(wi, (int64_t)0), last)];
            hib[u] = words[min(max(wi + 1, (int64_t)0), last)];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW);
        const uint32_t wa = lda[u] ? quad_bytes(loa[u], hia[u], sa[u], xa[u], W, da.flip) : 0u;
        const uint32_t wb = ldb[u] ? quad_bytes(lob[u], hib[u], sb[u], xb[u], W, db.flip) : 0u;
        const uint32_t w = (wa & ~msk[u]) | (wb & msk[u]);
        const float mean = c == 0 ? nrm.mean[0] : c == 1 ? nrm.mean[1] : nrm.mean[2];
        const float stdv = c == 0 ? nrm.stdv[0] : c == 1 ? nrm.stdv[1] : nrm.stdv[2];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float f = (float)((w >> (8 * k)) & 0xffu) / 255.0f;   // ToTensor
            v[k] = (f - mean) / stdv;                                     // Normalize
        }
        x[(int64_t)s * QS + r] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (r0 == 0) {
        const float wgt = (float)area / (float)(H * W);                   // IEEE division; 0 for an empty box
        y[s] = area > 0 ? (int64_t)((uint64_t)la | ((uint64_t)lb << 8) | ((uint64_t)__float_as_uint(wgt) << 32)) : la;
    }
}

template <int C, int H, int W, int U>
static int image_batch_mix_launch(const uint8_t* images, const uint8_t* labels, int n_images, const int64_t* idx,
                                  const int64_t* idx2, int B, const ImageNorm& nrm, int pad, int flip_enabled,
                                  uint32_t seed, uint32_t epoch, uint64_t apply_below, float* x, int64_t* y,
                                  int* err_flag, void* stream) {
    const int64_t total = (int64_t)B * (C * H * (W / 4) / U);
    SLK_CHECK_ARG((total + 255) / 256 <= 0x7fffffff);
    image_batch_mix_kernel<C, H, W, U><<<(unsigned)((total + 255) / 256), 256, 0, slk_stream(stream)>>>(
        reinterpret_cast<const uint32_t*>(images), labels, n_images, idx, idx2, B, nrm, pad, flip_enabled, seed, epoch,
        apply_below, reinterpret_cast<float4*>(x), y, err_flag);
    return slk_launch_status();
}

extern "C" int slk_image_batch_mix(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                                   const int64_t* idx, const int64_t* idx2, int B, const float* mean,
                                   const float* stdv, int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                   double prob, float* x, int64_t* y, int* err_flag, void* stream) {
    const bool cifar = C == 3 && H == 32 && W == 32, mnist = C == 1 && H == 28 && W == 28;
    SLK_CHECK_ARG(cifar || mnist);
    SLK_CHECK_ARG(B >= 0 && n_images > 0 && pad >= 0 && pad <= IMAGE_MAX_PAD);
    SLK_CHECK_ARG(prob >= 0.0 && prob <= 1.0);   // NaN fails both compares
    if (B == 0) return 0;
    SLK_CHECK_ARG(images && labels && idx && idx2 && x && y && mean && stdv);
    SLK_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)x & 15) == 0);
    ImageNorm nrm = {};
    for (int c = 0; c < C; ++c) {
        nrm.mean[c] = mean[c];
        nrm.stdv[c] = stdv[c];
    }
    const uint64_t apply_below = (uint64_t)(prob * 4294967296.0);   // apply iff h3 < prob * 2^32 (1.0: always)
    if (cifar)
        return image_batch_mix_launch<3, 32, 32, SLK_IMAGE_QUADS_CIFAR>(images, labels, n_images, idx, idx2, B, nrm, pad,
                                                                      flip_enabled, seed, epoch, apply_below, x, y,
                                                                      err_flag, stream);
    return image_batch_mix_launch<1, 28, 28, SLK_IMAGE_QUADS_MNIST>(images, labels, n_images, idx, idx2, B, nrm, pad,
                                                                  flip_enabled, seed, epoch, apply_below, x, y, err_flag,
                                                                  stream);
}

// -------------------------------------------------------------------------------- slk_image_batch_blend
// slk_image_batch_mix with the mixing weight drawn from a 1024-entry quantile table of Beta(alpha, alpha) instead of
// the two-uniforms trick, and with MixUp (Zhang et al. 2018) as a second mode, chosen per sample (slk.h has the rule).
// The primary's chain h3..h7 is read as apply (h3, as in the mix kernel), the mode (h4), the table index k = h5 >> 22
// and the box centre (h6, h7, as in the mix kernel). The host folds "only one table given" into the mode threshold
// (0: never CutMix, 2^32: always), so the table a sample's mode names is never NULL.
//
//   CutMix sample: side = (cut_table[k] * H) >> 32, then the mix kernel's box, masks and loads word for word.
//   MixUp sample:  both sources are loaded for every quad; each goes through quad_bytes on its own, and the blend is
//                  made in float32 on the two ToTensor values, every operation rounded on its own (blend_rn:
//                  hipcc would contract a*b + c into an fma, which rounds once and differs).
//   unapplied:     only source i is loaded (an empty box).
//
// The mode is uniform over a sample: whole waves at <3,32,32,4> (192 threads per sample), so neither branch below
// diverges there; a <1,28,28,1> wave can hold the end of one sample and the start of the next, and the two branches
// are kept to one table read and the partner's blend arithmetic. The table reads sit INSIDE their branches, one dword
// per thread at one address per sample: a CutMix sample needs its side before it knows which loads to issue, so its
// read is in front of them (one more L2 round trip in that sample's chain idx -> hash -> table -> pixels); a MixUp
// sample's read is issued after all its pixel loads, and an unapplied sample reads no table.
namespace {
// om * fa + lam * fb as two rounded products and one rounded sum. HIP's __fmul_rn / __fadd_rn are plain '*' and '+',
// which hipcc's default -ffp-contract=fast fuses into an fma like any other; the pragma takes the contract flag off
// these three operations, and it stays off when the function is inlined.
__device__ __forceinline__ float blend_rn(float om, float fa, float lam, float fb) {
#pragma clang fp contract(off)
    const float pa = om * fa, pb = lam * fb;
    return pa + pb;
}
}  // namespace

template <int C, int H, int W, int U>
__global__ __launch_bounds__(256) void image_batch_blend_kernel(const uint32_t* __restrict__ words,
                                                                const uint8_t* __restrict__ labels, int n_images,
                                                                const int64_t* __restrict__ idx,
                                                                const int64_t* __restrict__ idx2, int B, ImageNorm nrm,
                                                                int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                                                uint64_t apply_below, uint64_t cut_below,
                                                                const uint32_t* __restrict__ cut_table,
                                                                const float* __restrict__ lam_table,
                                                                float4* __restrict__ x, int64_t* __restrict__ y,
                                                                int* __restrict__ err) {
    static_assert(W % 4 == 0 && (C * H * W) % 4 == 0 && C <= IMAGE_MAX_C, "quads of one row, whole words per image");
    constexpr int QW = W / 4, QS = C * H * QW, TS = QS / U;
    static_assert(QS % U == 0, "every thread of a sample makes U quads");
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * TS) return;
    const int s = (int)(t / TS), r0 = (int)(t - (int64_t)s * TS);
    int64_t i = idx[s], i2 = idx2[s];
    if (i < 0 || i >= n_images) {        // out-of-range index: flag it, read row 0 (with row 0's draws)
        if (r0 == 0 && err) *err = 1;
        i = 0;
    }
    if (i2 < 0 || i2 >= n_images) {      // the partner likewise
        if (r0 == 0 && err) *err = 1;
        i2 = 0;
    }
    // both labels loaded by every thread and stored last by one (see image_batch_kernel)
    const int64_t la = (int64_t)labels[i], lb = (int64_t)labels[i2];

    const ImageDraws da = image_draws(i, seed, epoch, pad, flip_enabled);
    const ImageDraws db = image_draws(i2, seed, epoch, pad, flip_enabled);
    const uint32_t h3 = lowbias32(da.h2 + 0x9E3779B9u), h4 = lowbias32(h3 + 0x9E3779B9u);
    const uint32_t h5 = lowbias32(h4 + 0x9E3779B9u), h6 = lowbias32(h5 + 0x9E3779B9u);
    const uint32_t h7 = lowbias32(h6 + 0x9E3779B9u);
    const bool apply = (uint64_t)h3 < apply_below;
    const bool cut = apply && (uint64_t)h4 < cut_below, blend = apply && !cut;
    const uint32_t k = h5 >> 22;         // table index, 0 .. 1023
    int half = 0;
    if (cut) half = (int)(((uint64_t)cut_table[k] * H) >> 32) / 2;
    const int cy = (int)(((uint64_t)h6 * H) >> 32), cx = (int)(((uint64_t)h7 * W) >> 32);
    const int y1 = min(max(cy - half, 0), H), y2 = cut ? min(max(cy + half, 0), H) : y1;   // no box: empty
    const int x1 = min(max(cx - half, 0), W), x2 = min(max(cx + half, 0), W);
    const int area = (y2 - y1) * (x2 - x1);
    const int64_t last = (int64_t)n_images * (C * H * W / 4) - 1;   // the dataset's last word

    int xa[U], xb[U], sa[U], sb[U];
    uint32_t loa[U], hia[U], lob[U], hib[U], msk[U];   // msk: bytes of the quad that lie inside the box
    bool lda[U], ldb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW), yo = (r / QW) % H, q = r % QW;
        uint32_t m = 0;
        if (yo >= y1 && yo < y2) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) m |= (4 * q + kk >= x1 && 4 * q + kk < x2) ? 0xffu << (8 * kk) : 0u;
        }
        msk[u] = m;
        const int ysa = yo + da.dy - pad, ysb = yo + db.dy - pad;
        xa[u] = (da.flip ? W - 4 - 4 * q : 4 * q) + da.dx - pad;
        xb[u] = (db.flip ? W - 4 - 4 * q : 4 * q) + db.dx - pad;
        lda[u] = m != 0xffffffffu && (unsigned)ysa < (unsigned)H && xa[u] > -4 && xa[u] < W;
        ldb[u] = (blend || m != 0u) && (unsigned)ysb < (unsigned)H && xb[u] > -4 && xb[u] < W;
        loa[u] = hia[u] = lob[u] = hib[u] = 0;
        sa[u] = sb[u] = 0;
        if (lda[u]) {
            const int64_t a = (((int64_t)i * C + c) * H + ysa) * W + xa[u];    // byte address, may be < 0
            const int64_t wi = a >> 2;
            sa[u] = (int)(a & 3);
            loa[u] = words[min(max(wi, (int64_t)0), last)];
            hia[u] = words[min(max(wi + 1, (int64_t)0), last)];
        }
        if (ldb[u]) {
            const int64_t a = (((int64_t)i2 * C + c) * H + ysb) * W + xb[u];
            const int64_t wi = a >> 2;
            sb[u] = (int)(a & 3);
            lob[u] = words[min(max(wi, (int64_t)0), last)];
            hib[u] = words[min(max(wi + 1, (int64_t)0), last)];
        }
    }
    float lam = 0.0f;                    // the partner's weight of a MixUp sample; read behind the pixel loads
    if (blend) lam = lam_table[k];
    const float om = 1.0f - lam;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW);
        const uint32_t wa = lda[u] ? quad_bytes(loa[u], hia[u], sa[u], xa[u], W, da.flip) : 0u;
        const uint32_t wb = ldb[u] ? quad_bytes(lob[u], hib[u], sb[u], xb[u], W, db.flip) : 0u;
        const uint32_t w = blend ? wa : (wa & ~msk[u]) | (wb & msk[u]);
        const float mean = c == 0 ? nrm.mean[0] : c == 1 ? nrm.mean[1] : nrm.mean[2];
        const float stdv = c == 0 ? nrm.stdv[0] : c == 1 ? nrm.stdv[1] : nrm.stdv[2];
        float f[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) f[kk] = (float)((w >> (8 * kk)) & 0xffu) / 255.0f;   // ToTensor
        if (blend) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float fb = (float)((wb >> (8 * kk)) & 0xffu) / 255.0f;
                f[kk] = blend_rn(om, f[kk], lam, fb);
            }
        }
        float v[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) v[kk] = (f[kk] - mean) / stdv;                       // Normalize
        x[(int64_t)s * QS + r] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (r0 == 0) {
        const float wgt = cut ? (float)area / (float)(H * W) : lam;       // IEEE division; 0 for an empty box
        const bool mixed = cut ? area > 0 : lam > 0.0f;                   // lam is 0 unless blend
        y[s] = mixed ? (int64_t)((uint64_t)la | ((uint64_t)lb << 8) | ((uint64_t)__float_as_uint(wgt) << 32)) : la;
    }
}

template <int C, int H, int W, int U>
static int image_batch_blend_launch(const uint8_t* images, const uint8_t* labels, int n_images, const int64_t* idx,
                                    const int64_t* idx2, int B, const ImageNorm& nrm, int pad, int flip_enabled,
                                    uint32_t seed, uint32_t epoch, uint64_t apply_below, uint64_t cut_below,
                                    const uint32_t* cut_table, const float* lam_table, float* x, int64_t* y,
                                    int* err_flag, void* stream) {
    const int64_t total = (int64_t)B * (C * H * (W / 4) / U);
    SLK_CHECK_ARG((total + 255) / 256 <= 0x7fffffff);
    image_batch_blend_kernel<C, H, W, U><<<(unsigned)((total + 255) / 256), 256, 0, slk_stream(stream)>>>(
        reinterpret_cast<const uint32_t*>(images), labels, n_images, idx, idx2, B, nrm, pad, flip_enabled, seed, epoch,
        apply_below, cut_below, cut_table, lam_table, reinterpret_cast<float4*>(x), y, err_flag);
    return slk_launch_status();
}

extern "C" int slk_image_batch_blend(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                                     const int64_t* idx, const int64_t* idx2, int B, const float* mean,
                                     const float* stdv, int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                     double prob, const uint32_t* cut_table, const float* lam_table, double switch_prob,
                                     float* x, int64_t* y, int* err_flag, void* stream) {
    const bool cifar = C == 3 && H == 32 && W == 32, mnist = C == 1 && H == 28 && W == 28;
    SLK_CHECK_ARG(cifar || mnist);
    SLK_CHECK_ARG(B >= 0 && n_images > 0 && pad >= 0 && pad <= IMAGE_MAX_PAD);
    SLK_CHECK_ARG(prob >= 0.0 && prob <= 1.0);                 // NaN fails both compares
    SLK_CHECK_ARG(switch_prob >= 0.0 && switch_prob <= 1.0);
    SLK_CHECK_ARG(cut_table || lam_table);
    SLK_CHECK_ARG(((uintptr_t)cut_table & 3) == 0 && ((uintptr_t)lam_table & 3) == 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(images && labels && idx && idx2 && x && y && mean && stdv);
    SLK_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)x & 15) == 0);
    ImageNorm nrm = {};
    for (int c = 0; c < C; ++c) {
        nrm.mean[c] = mean[c];
        nrm.stdv[c] = stdv[c];
    }
    const uint64_t apply_below = (uint64_t)(prob * 4294967296.0);   // apply iff h3 < prob * 2^32 (1.0: always)
    // CutMix iff h4 < switch_prob * 2^32 with both tables; one table alone names the mode (never / always)
    const uint64_t cut_below = cut_table && lam_table ? (uint64_t)(switch_prob * 4294967296.0)
                               : cut_table ? (uint64_t)1 << 32 : 0;
    if (cifar)
        return image_batch_blend_launch<3, 32, 32, SLK_IMAGE_QUADS_CIFAR>(images, labels, n_images, idx, idx2, B, nrm,
                                                                        pad, flip_enabled, seed, epoch, apply_below,
                                                                        cut_below, cut_table, lam_table, x, y, err_flag,
                                                                        stream);
    return image_batch_blend_launch<1, 28, 28, SLK_IMAGE_QUADS_MNIST>(images, labels, n_images, idx, idx2, B, nrm, pad,
                                                                    flip_enabled, seed, epoch, apply_below, cut_below,
                                                                    cut_table, lam_table, x, y, err_flag, stream);
}
