// slk_data.hip — the batch loaders as one HBM-resident gather each: slk_mnist_batch (K2) and
// slk_image_batch (K5's CIFAR-10 path with crop + flip augmentation, and MNIST with a crop), plus
// slk_image_batch_mix, the same gather with CutMix and mixed labels, and slk_image_batch_blend, which draws the box
// side or a MixUp weight from a Beta(alpha, alpha) quantile table per sample: three modes of one kernel template.
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

// ------------------------------------------ slk_image_batch, slk_image_batch_mix, slk_image_batch_blend
// RandomCrop(H, padding=pad, fill 0) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize(mean[C], std[C])
// of the rows idx[b] of a u8 dataset [N][C][H][W], one launch per batch: ONE kernel template in three modes.
//   none   the plain gather (slk_image_batch).
//   box    CutMix (Yun et al. 2019, lam ~ Beta(1, 1)): batch position s shows sample i = idx[s] with a box of
//          sample i2 = idx2[s] pasted in, each under its OWN crop and flip draws, and y[s] is the mixed label
//          a | b << 8 | bits(wb) << 32 (slk.h). The box side is the larger of two uniforms (slk_image_batch_mix).
//   table  the mixing weight comes from a 1024-entry quantile table of Beta(alpha, alpha), and MixUp (Zhang et al.
//          2018) is a second way to mix, chosen per sample (slk_image_batch_blend; slk.h has the rule).
// The per-sample draws come from lowbias32 keyed on the DATASET index (slk.h), so they do not depend on the batch
// a sample lands in; the box comes from the primary sample's hash chain continued (h3..h7), all in integers: apply
// (h3), then the two side uniforms (box: h4, h5) or the way to mix and the table index k = h5 >> 22 (table: h4,
// h5), then the box centre (h6, h7). The host folds "only one table given" into the threshold on h4 (0: never
// CutMix, 2^32: always), so the table a sample's draw names is never NULL.
//
// A quad is four consecutive output pixels of one row, stored as one aligned float4. A thread makes
// U quads of one sample, 1/U of the sample apart (the lanes of a wave stay on consecutive quads), so the
// sample's draws are hashed once and 2U loads per source are in flight per thread. A quad's four
// source bytes are consecutive too (read backwards when flipped), start at any byte offset and may hang
// over either edge of the row: the thread loads the two aligned words around them, v_alignbyte cuts the
// four bytes out, v_perm reverses them for a flip, and the columns outside the row are masked to the
// padding value 0. A word index is clamped into the dataset BEFORE the load; a clamped word only ever
// supplies masked columns, since a byte in a column inside the row lies inside the dataset and so does
// its word. That argument holds per source: each source's indices are clamped and each source masks its own
// columns. Rows above or below the image, and quads entirely beside it, issue no load.
// HBM-bound like mnist_batch: C*H*W bytes read, 4*C*H*W written per sample.
//
// Mixing selects on the u8 pixels (CutMix) or blends the ToTensor values (MixUp), then the same Normalize runs:
//   CutMix sample: a quad on a row outside the box, or with its four columns all outside it, loads only source i; a
//                  quad wholly inside loads only source i2; only the at most two quads of a box row that straddle
//                  an edge load both, and take their bytes by a mask AFTER each source's own alignbyte / column
//                  mask / flip permute (byte k of either word is output pixel k by then).
//   MixUp sample:  both sources are loaded for every quad; each goes through quad_bytes on its own, and the blend is
//                  made in float32 on the two ToTensor values, every operation rounded on its own (blend_rn).
//   unapplied:     only source i is loaded (an empty box).
// The way a sample is mixed is uniform over the sample: whole waves at <3,32,32,4> (192 threads per sample), so no
// branch on it diverges there; a <1,28,28,1> wave can hold the end of one sample and the start of the next, and the
// branches are kept to one table read and the partner's blend arithmetic. The table reads sit INSIDE their branches,
// one dword per thread at one address per sample: a CutMix sample needs its side before it knows which loads to
// issue, so its read is in front of them (one more L2 round trip in that sample's chain idx -> hash -> table ->
// pixels); a MixUp sample's read is issued after all its pixel loads, and an unapplied sample reads no table.

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

enum class ImageMode { none, box, table };
// what a mode's kernel takes beyond the plain gather's arguments, by value
template <ImageMode M>
struct ImageModeArgs {};
template <>
struct ImageModeArgs<ImageMode::box> {
    const int64_t* idx2;
    uint64_t apply_below;
};
template <>
struct ImageModeArgs<ImageMode::table> {
    const int64_t* idx2;
    uint64_t apply_below, cut_below;
    const uint32_t* cut_table;
    const float* lam_table;
};

// an out-of-range index: flag it (thread r0 = 0 of the sample), read row 0 instead, with row 0's draws
__device__ __forceinline__ int64_t checked_row(int64_t i, int n_images, bool flagger, int* __restrict__ err) {
    if (i < 0 || i >= n_images) {
        if (flagger && err) *err = 1;
        i = 0;
    }
    return i;
}

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

// How sample i is mixed: rows [y1, y2) x columns [x1, x2) come from the partner (empty unless `cut`), or the whole
// image is blended with it at table entry k (`blend`). Mode none: neither, ever.
struct ImageBox {
    int y1, y2, x1, x2, area;
    bool cut, blend;
    uint32_t k;
};
template <int H, int W, ImageMode M>
__device__ __forceinline__ ImageBox image_box(uint32_t h2, const ImageModeArgs<M>& m) {
    if constexpr (M == ImageMode::none) {
        return {};
    } else {
        const uint32_t h3 = lowbias32(h2 + 0x9E3779B9u), h4 = lowbias32(h3 + 0x9E3779B9u);
        const uint32_t h5 = lowbias32(h4 + 0x9E3779B9u), h6 = lowbias32(h5 + 0x9E3779B9u);
        const uint32_t h7 = lowbias32(h6 + 0x9E3779B9u);
        const bool apply = (uint64_t)h3 < m.apply_below;
        const uint32_t k = h5 >> 22;     // table index, 0 .. 1023
        bool cut = apply;
        int half = 0;
        if constexpr (M == ImageMode::box) {
            half = max((int)(((uint64_t)h4 * H) >> 32), (int)(((uint64_t)h5 * H) >> 32)) / 2;
        } else {
            cut = apply && (uint64_t)h4 < m.cut_below;
            if (cut) half = (int)(((uint64_t)m.cut_table[k] * H) >> 32) / 2;
        }
        const int cy = (int)(((uint64_t)h6 * H) >> 32), cx = (int)(((uint64_t)h7 * W) >> 32);
        const int y1 = min(max(cy - half, 0), H), y2 = cut ? min(max(cy + half, 0), H) : y1;   // no box: empty
        const int x1 = min(max(cx - half, 0), W), x2 = min(max(cx + half, 0), W);
        return {y1, y2, x1, x2, (y2 - y1) * (x2 - x1), cut, apply && !cut, k};
    }
}

// One source's share of quad q of output row yo, channel c: the four source bytes are columns x0 .. x0+3 of row
// yo + dy - pad, output pixel k taking x0+k (x0+3-k if flipped). `want` is false where the other source supplies the
// whole quad. quad_load issues the two loads around the bytes and returns at once; quad_bytes is their first use.
// Rows are whole words (W % 4 == 0), so the bytes start x0 & 3 into the first word and no shift is kept.
struct QuadLoad {
    int x0;
    uint32_t lo, hi;
    bool ld;
};
template <int C, int H, int W>
__device__ __forceinline__ QuadLoad quad_load(const uint32_t* __restrict__ words, int64_t last, int64_t i, int c, int yo,
                                              int q, ImageDraws d, int pad, bool want) {
    const int ys = yo + d.dy - pad;
    QuadLoad l = {};
    l.x0 = (d.flip ? W - 4 - 4 * q : 4 * q) + d.dx - pad;
    l.ld = want && (unsigned)ys < (unsigned)H && l.x0 > -4 && l.x0 < W;
    if (l.ld) {
        const int64_t wi = ((((int64_t)i * C + c) * H + ys) * W + l.x0) >> 2;   // of a byte address that may be < 0
        l.lo = words[min(max(wi, (int64_t)0), last)];
        l.hi = words[min(max(wi + 1, (int64_t)0), last)];
    }
    return l;
}
// the four source bytes of one quad after alignbyte, the column mask and the flip permute: byte k = output pixel k
__device__ __forceinline__ uint32_t quad_bytes(const QuadLoad& l, int W, bool flip) {
    uint32_t w = 0;
    if (l.ld) {
        w = __builtin_amdgcn_alignbyte(l.hi, l.lo, (uint32_t)l.x0 & 3u);
        uint32_t keep = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) keep |= (unsigned)(l.x0 + k) < (unsigned)W ? 0xffu << (8 * k) : 0u;
        w &= keep;
        if (flip) w = __builtin_amdgcn_perm(w, w, 0x00010203u);             // byte k <- byte 3-k
    }
    return w;
}

// om * fa + lam * fb as two rounded products and one rounded sum. HIP's __fmul_rn / __fadd_rn are plain '*' and '+',
// which hipcc's default -ffp-contract=fast fuses into an fma like any other (it rounds once and differs); the pragma
// takes the contract flag off these three operations, and it stays off when the function is inlined.
__device__ __forceinline__ float blend_rn(float om, float fa, float lam, float fb) {
#pragma clang fp contract(off)
    const float pa = om * fa, pb = lam * fb;
    return pa + pb;
}

// ToTensor, the MixUp blend with the partner's bytes wb (table mode), Normalize with channel c's mean and std
template <ImageMode M>
__device__ __forceinline__ float4 quad_pixels(uint32_t w, uint32_t wb, bool blend, float om, float lam, int c,
                                              ImageNorm nrm) {
    // selects, not an index: a per-lane index into the by-value struct would move it to scratch
    const float mean = c == 0 ? nrm.mean[0] : c == 1 ? nrm.mean[1] : nrm.mean[2];
    const float stdv = c == 0 ? nrm.stdv[0] : c == 1 ? nrm.stdv[1] : nrm.stdv[2];
    float f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) f[k] = (float)((w >> (8 * k)) & 0xffu) / 255.0f;   // ToTensor
    if constexpr (M == ImageMode::table) {
        if (blend) {
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = blend_rn(om, f[k], lam, (float)((wb >> (8 * k)) & 0xffu) / 255.0f);
        }
    }
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (f[k] - mean) / stdv;                       // Normalize
    return make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ int64_t mixed_label(int64_t a, int64_t b, float wb) {
    return (int64_t)((uint64_t)a | ((uint64_t)b << 8) | ((uint64_t)__float_as_uint(wb) << 32));
}
}  // namespace

template <int C, int H, int W, int U, ImageMode M>
__global__ __launch_bounds__(256) void image_batch_kernel(const uint32_t* __restrict__ words,
                                                          const uint8_t* __restrict__ labels, int n_images,
                                                          const int64_t* __restrict__ idx, int B, ImageNorm nrm,
                                                          int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                                          ImageModeArgs<M> m, float4* __restrict__ x,
                                                          int64_t* __restrict__ y, int* __restrict__ err) {
    static_assert(W % 4 == 0 && (C * H * W) % 4 == 0 && C <= IMAGE_MAX_C, "quads of one row, whole words per image");
    constexpr int QW = W / 4;            // quads per row
    constexpr int QS = C * H * QW;       // quads per sample
    constexpr int TS = QS / U;           // threads per sample; thread r0 makes quads r0 + u * TS
    constexpr bool MIXED = M != ImageMode::none;
    static_assert(QS % U == 0, "every thread of a sample makes U quads");
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * TS) return;
    const int s = (int)(t / TS), r0 = (int)(t - (int64_t)s * TS);
    int64_t i = idx[s], i2 = 0;
    if constexpr (MIXED) i2 = m.idx2[s];
    i = checked_row(i, n_images, r0 == 0, err);
    if constexpr (MIXED) i2 = checked_row(i2, n_images, r0 == 0, err);
    // labels are loaded by every thread (one address per sample) and stored last by one: a load under `r0 == 0`
    // would be waited for at the end of its branch, in front of the pixel loads
    const int64_t la = (int64_t)labels[i];
    int64_t lb = 0;
    if constexpr (MIXED) lb = (int64_t)labels[i2];

    const ImageDraws da = image_draws(i, seed, epoch, pad, flip_enabled);
    ImageDraws db = {};
    if constexpr (MIXED) db = image_draws(i2, seed, epoch, pad, flip_enabled);
    const ImageBox box = image_box<H, W>(da.h2, m);
    const int64_t last = (int64_t)n_images * (C * H * W / 4) - 1;   // the dataset's last word

    // All loads of the thread are issued before the first is used: the launch is bound by how many loads are in
    // flight, not by arithmetic. The arrays are indexed by the unrolled u alone, so they stay in registers.
    QuadLoad qa[U], qb[U];
    uint32_t msk[U];                     // bytes of the quad that lie inside the box
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        const int c = r / (H * QW), yo = (r / QW) % H, q = r % QW;
        msk[u] = 0;
        if (MIXED && yo >= box.y1 && yo < box.y2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) msk[u] |= (4 * q + k >= box.x1 && 4 * q + k < box.x2) ? 0xffu << (8 * k) : 0u;
        }
        qa[u] = quad_load<C, H, W>(words, last, i, c, yo, q, da, pad, msk[u] != 0xffffffffu);
        if constexpr (MIXED) qb[u] = quad_load<C, H, W>(words, last, i2, c, yo, q, db, pad, box.blend || msk[u] != 0u);
    }
    float lam = 0.0f;                    // the partner's weight of a MixUp sample; read behind the pixel loads
    if constexpr (M == ImageMode::table) {
        if (box.blend) lam = m.lam_table[box.k];
    }
    const float om = 1.0f - lam;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = r0 + u * TS;
        uint32_t w = quad_bytes(qa[u], W, da.flip), wb = 0;
        if constexpr (MIXED) {
            wb = quad_bytes(qb[u], W, db.flip);
            if (!box.blend) w = (w & ~msk[u]) | (wb & msk[u]);
        }
        x[(int64_t)s * QS + r] = quad_pixels<M>(w, wb, box.blend, om, lam, r / (H * QW), nrm);
    }
    if (r0 == 0) {
        float wgt = (float)box.area / (float)(H * W);                    // IEEE division; 0 for an empty box
        bool mixed = box.area > 0;
        if constexpr (M == ImageMode::table) {
            if (!box.cut) {                                              // lam is 0 unless blend
                wgt = lam;
                mixed = lam > 0.0f;
            }
        }
        y[s] = mixed ? mixed_label(la, lb, wgt) : la;
    }
}

// The checks, the ImageNorm fill and the launch the three entries share. An entry checks its own arguments first;
// every refusal is the same invalid-argument code, and B == 0 returns 0 only after the checks that do not need B > 0.
template <ImageMode M>
static int image_batch_launch(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                              const int64_t* idx, int B, const float* mean, const float* stdv, int pad,
                              int flip_enabled, uint32_t seed, uint32_t epoch, const ImageModeArgs<M>& m, float* x,
                              int64_t* y, int* err_flag, void* stream) {
    const bool cifar = C == 3 && H == 32 && W == 32, mnist = C == 1 && H == 28 && W == 28;
    SLK_CHECK_ARG(cifar || mnist);
    SLK_CHECK_ARG(B >= 0 && n_images > 0 && pad >= 0 && pad <= IMAGE_MAX_PAD);
    if (B == 0) return 0;
    SLK_CHECK_ARG(images && labels && idx && x && y && mean && stdv);
    if constexpr (M != ImageMode::none) SLK_CHECK_ARG(m.idx2);
    SLK_CHECK_ARG(((uintptr_t)images & 3) == 0 && ((uintptr_t)x & 15) == 0);
    ImageNorm nrm = {};
    for (int c = 0; c < C; ++c) {
        nrm.mean[c] = mean[c];
        nrm.stdv[c] = stdv[c];
    }
    const int U = cifar ? SLK_IMAGE_QUADS_CIFAR : SLK_IMAGE_QUADS_MNIST;
    const int64_t total = (int64_t)B * (C * H * (W / 4) / U);           // threads
    SLK_CHECK_ARG((total + 255) / 256 <= 0x7fffffff);
    const auto launch = [&](auto kernel) {
        kernel<<<(unsigned)((total + 255) / 256), 256, 0, slk_stream(stream)>>>(
            reinterpret_cast<const uint32_t*>(images), labels, n_images, idx, B, nrm, pad, flip_enabled, seed, epoch, m,
            reinterpret_cast<float4*>(x), y, err_flag);
    };
    if (cifar)
        launch(image_batch_kernel<3, 32, 32, SLK_IMAGE_QUADS_CIFAR, M>);
    else
        launch(image_batch_kernel<1, 28, 28, SLK_IMAGE_QUADS_MNIST, M>);
    return slk_launch_status();
}

extern "C" int slk_image_batch(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                               const int64_t* idx, int B, const float* mean, const float* stdv, int pad,
                               int flip_enabled, uint32_t seed, uint32_t epoch, float* x, int64_t* y,
                               int* err_flag, void* stream) {
    return image_batch_launch<ImageMode::none>(images, labels, n_images, C, H, W, idx, B, mean, stdv, pad, flip_enabled,
                                               seed, epoch, {}, x, y, err_flag, stream);
}

extern "C" int slk_image_batch_mix(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                                   const int64_t* idx, const int64_t* idx2, int B, const float* mean,
                                   const float* stdv, int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                   double prob, float* x, int64_t* y, int* err_flag, void* stream) {
    SLK_CHECK_ARG(prob >= 0.0 && prob <= 1.0);   // NaN fails both compares
    const uint64_t apply_below = (uint64_t)(prob * 4294967296.0);   // apply iff h3 < prob * 2^32 (1.0: always)
    return image_batch_launch<ImageMode::box>(images, labels, n_images, C, H, W, idx, B, mean, stdv, pad, flip_enabled,
                                              seed, epoch, {idx2, apply_below}, x, y, err_flag, stream);
}

extern "C" int slk_image_batch_blend(const uint8_t* images, const uint8_t* labels, int n_images, int C, int H, int W,
                                     const int64_t* idx, const int64_t* idx2, int B, const float* mean,
                                     const float* stdv, int pad, int flip_enabled, uint32_t seed, uint32_t epoch,
                                     double prob, const uint32_t* cut_table, const float* lam_table, double switch_prob,
                                     float* x, int64_t* y, int* err_flag, void* stream) {
    SLK_CHECK_ARG(prob >= 0.0 && prob <= 1.0);                 // NaN fails both compares
    SLK_CHECK_ARG(switch_prob >= 0.0 && switch_prob <= 1.0);
    SLK_CHECK_ARG(cut_table || lam_table);
    SLK_CHECK_ARG(((uintptr_t)cut_table & 3) == 0 && ((uintptr_t)lam_table & 3) == 0);
    const uint64_t apply_below = (uint64_t)(prob * 4294967296.0);
    // CutMix iff h4 < switch_prob * 2^32 with both tables; one table alone names the way (never / always)
    const uint64_t cut_below = cut_table && lam_table ? (uint64_t)(switch_prob * 4294967296.0)
                               : cut_table ? (uint64_t)1 << 32 : 0;
    return image_batch_launch<ImageMode::table>(images, labels, n_images, C, H, W, idx, B, mean, stdv, pad, flip_enabled,
                                                seed, epoch, {idx2, apply_below, cut_below, cut_table, lam_table}, x, y,
                                                err_flag, stream);
}
