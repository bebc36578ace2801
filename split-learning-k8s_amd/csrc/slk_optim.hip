// slk_optim.hip — deterministic reductions, fused SGD and the device-side loss log.
//
// optim.SGD(lr=0.01) on both sides (client_part.py:17,133; server_part.py:15,52) is
// `p.add_(g, alpha=-lr)` per parameter. Here the parameters of a stage live in one flat block, so
// one launch updates all of them, and the weight-gradient slabs written by the wgrad kernels are
// summed (fixed order, bit-stable) in the same pass that applies the update.
#include "slk_common.h"
#include "slk_adam.h"

// Deterministic slab reduction (+ optional SGD). A 1024-thread block owns 64 columns; wave w sums
// slabs w, w+16, w+32, ... of those columns in order (8 loads in flight), then wave 0 adds the 16
// partials in wave order. The result is a fixed function of the inputs (no atomics).
constexpr int RS_WAVES = 16;
// Few slabs (<= RS_COLS_MAX) -> thread = column, slabs summed in ascending order with 8 loads in flight,
// 1024 columns per block; up to RS_MID_MAX (the fc wgrad set, 64 at B = 4096) -> 256 columns per block,
// 4 waves per 64 columns each summing every 4th slab, the 4 partials added in order (round 6: one thread
// per column walked 64 slabs in 8 dependent rounds on 91 blocks; 64-column blocks over 92,170 columns
// were ~1,400 dispatch-bound blocks); many slabs -> 64 columns per block, 16 waves over the slab range.
constexpr int RS_COLS_MAX = 16, RS_MID_MAX = 64;
__host__ __device__ constexpr int rs_cols_per_block(int nslab) {
    return nslab <= RS_COLS_MAX ? 1024 : (nslab <= RS_MID_MAX ? 256 : 64);
}
static inline int rs_blocks(int n, int nslab) { return (n + rs_cols_per_block(nslab) - 1) / rs_cols_per_block(nslab); }

// The per-element step of a reduced gradient t. SgdApply: p -= lr * t (optim.SGD(lr), the reference's
// recipe; param == NULL only reduces). SgdmApply: torch.optim.SGD with momentum / dampening / Nesterov /
// weight decay, the rate read from a device table at the stage's device step counter.
struct SgdApply {
    float* __restrict__ param;
    float* __restrict__ grad;
    float lr;
    __device__ __forceinline__ void operator()(int i, float t) const {
        if (grad) grad[i] = t;
        if (param) param[i] = param[i] - lr * t;
    }
};

struct SgdmHyper {
    const float* lr_table;
    int lr_len;
    const int* step;
    float momentum, dampening, weight_decay;
    int nesterov;
};
struct SgdmApply {
    float* __restrict__ param;
    float* __restrict__ grad;
    float* __restrict__ buf;
    SgdmHyper h;
    // torch/optim/sgd.py _single_tensor_sgd: grad.add(param, alpha=wd); buf = grad (first step) or
    // buf.mul_(momentum).add_(grad, alpha=1 - dampening); grad.add(buf, alpha=momentum) (Nesterov) or buf;
    // param.add_(grad, alpha=-lr). grad[i] receives the reduced gradient before weight decay.
    __device__ __forceinline__ void operator()(int i, float g) const {
        if (grad) grad[i] = g;
        const int st = *h.step;
        const float lr = slk_lr_at(h.lr_table, h.lr_len, st);
        const float p = param[i];
        if (h.weight_decay != 0.f) g = g + h.weight_decay * p;
        if (h.momentum != 0.f) {
            const float b = st == 0 ? g : h.momentum * buf[i] + (1.f - h.dampening) * g;
            buf[i] = b;
            g = h.nesterov ? g + h.momentum * b : b;
        }
        param[i] = p - lr * g;
    }
};

// The three reduction forms; `prior` (if non-null) is added to the sum (slk_reduce_slabs accumulate).
template <class Apply>
__device__ __forceinline__ void slab_reduce_cols(const float* __restrict__ prior, const float* __restrict__ slabs,
                                                 int nslab, int n, int blk, const Apply& apply) {
    const int i = blk * 1024 + threadIdx.x;
    if (i >= n) return;
    const float* s = slabs + i;
    float g = 0.f;
    int k = 0;
    for (; k + 8 <= nslab; k += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(k + u) * n];
#pragma unroll
        for (int u = 0; u < 8; ++u) g += v[u];
    }
    for (; k < nslab; ++k) g += s[(size_t)k * n];
    apply(i, prior ? prior[i] + g : g);
}

template <class Apply>
__device__ __forceinline__ void slab_reduce_rows(const float* __restrict__ prior, const float* __restrict__ slabs,
                                                 int nslab, int n, int blk, const Apply& apply) {
    __shared__ float part[RS_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blk * 64 + lane;
    float g = 0.f;
    if (i < n) {
        const float* s = slabs + i;
        int k = wave;
        for (; k + 7 * RS_WAVES < nslab; k += 8 * RS_WAVES) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(k + u * RS_WAVES) * n];
#pragma unroll
            for (int u = 0; u < 8; ++u) g += v[u];
        }
        for (; k < nslab; k += RS_WAVES) g += s[(size_t)k * n];
    }
    part[wave][lane] = g;
    __syncthreads();
    if (wave == 0 && i < n) {
        float t = prior ? prior[i] : 0.f;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) t += part[w][lane];
        apply(i, t);
    }
}

template <class Apply>
__device__ __forceinline__ void slab_reduce_mid(const float* __restrict__ prior, const float* __restrict__ slabs,
                                                int nslab, int n, int blk, const Apply& apply) {
    __shared__ float part[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (wave & 3) * 64 + lane, sg = wave >> 2;  // column within the block, slab group
    const int i = blk * 256 + c;
    float g = 0.f;
    if (i < n) {
        const float* s = slabs + i;
        int k = sg;
        for (; k + 7 * 4 < nslab; k += 8 * 4) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(k + 4 * u) * n];
#pragma unroll
            for (int u = 0; u < 8; ++u) g += v[u];
        }
        for (; k < nslab; k += 4) g += s[(size_t)k * n];
    }
    part[sg][c] = g;
    __syncthreads();
    if (sg == 0 && i < n) {
        float t = prior ? prior[i] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) t += part[q][c];
        apply(i, t);
    }
}

template <class Apply>
__device__ __forceinline__ void slab_reduce(const float* __restrict__ prior, const float* __restrict__ slabs,
                                            int nslab, int n, int blk, const Apply& apply) {
    if (rs_cols_per_block(nslab) == 1024)
        slab_reduce_cols(prior, slabs, nslab, n, blk, apply);
    else if (rs_cols_per_block(nslab) == 256)
        slab_reduce_mid(prior, slabs, nslab, n, blk, apply);
    else
        slab_reduce_rows(prior, slabs, nslab, n, blk, apply);
}

__global__ __launch_bounds__(1024) void sgd_from_slabs_kernel(float* __restrict__ param,
                                                              float* __restrict__ grad,
                                                              const float* __restrict__ slabs,
                                                              int nslab, int n, float lr, int acc) {
    slab_reduce(acc ? grad : nullptr, slabs, nslab, n, blockIdx.x, SgdApply{param, grad, lr});
}

__global__ __launch_bounds__(1024) void sgdm_from_slabs_kernel(float* __restrict__ param, float* __restrict__ grad,
                                                               float* __restrict__ buf,
                                                               const float* __restrict__ slabs, int nslab, int n,
                                                               const SgdmHyper h) {
    slab_reduce(nullptr, slabs, nslab, n, blockIdx.x, SgdmApply{param, grad, buf, h});
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ param,
                                                  const float* __restrict__ grad, int n, float lr) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        param[i] = param[i] - lr * grad[i];
}

__device__ __forceinline__ float block_sum_256(const float* __restrict__ v, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += v[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void loss_sum_kernel(const float* __restrict__ v, int n, float scale,
                                                       float* __restrict__ out) {
    const float s = block_sum_256(v, n);
    if (threadIdx.x == 0) out[0] = s * scale;
}

__global__ __launch_bounds__(256) void loss_log_kernel(const float* __restrict__ v, int n, float scale,
                                                       float* __restrict__ ring, int capacity,
                                                       int* __restrict__ counter) {
    const float s = block_sum_256(v, n);
    if (threadIdx.x == 0) {
        const int c = *counter;
        ring[c % capacity] = s * scale;
        *counter = c + 1;
    }
}

// Every optimizer step of one split step in ONE launch (the last launches of the step are latency,
// not bandwidth): block 0 (if loss.v) logs the loss, the next nblk0 blocks reduce + step segment 0,
// the next nblk1 segment 1, .... Each block runs exactly the code of sgd_from_slabs_kernel /
// sgdm_from_slabs_kernel / loss_log_kernel on its slice, so the results are bit-identical to the
// separate launches.
struct SgdSeg {
    float* param;
    float* grad;
    float* buf;  // momentum buffer (sgdm only)
    const float* slabs;
    int nslab, n, nblk;
};
constexpr int SGD_MAXSEG = 4;
struct LossLogArgs {
    const float* v;
    int n;
    float scale;
    float* ring;
    int capacity;
    int* counter;
};
struct SgdHyper {
    float lr;
    __device__ __forceinline__ SgdApply apply(const SgdSeg& g) const { return SgdApply{g.param, g.grad, lr}; }
};
struct SgdmMultiHyper {
    SgdmHyper h;
    __device__ __forceinline__ SgdmApply apply(const SgdSeg& g) const { return SgdmApply{g.param, g.grad, g.buf, h}; }
};
template <class Hyper>
struct SgdMulti {
    SgdSeg seg[SGD_MAXSEG];
    int nseg;
    Hyper hyper;
    LossLogArgs loss;
};

// slk_loss_log as one block of a 1024-thread launch: threads 0..255 sum exactly as block_sum_256 (the other
// waves add nothing).
__device__ __forceinline__ void loss_log_block(const LossLogArgs& l) {
    __shared__ float red[4];
    float v = 0.f;
    if (threadIdx.x < 256)
        for (int i = threadIdx.x; i < l.n; i += 256) v += l.v[i];
    v = wave_sum(v);
    if (threadIdx.x < 256 && (threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tot = ((red[0] + red[1]) + red[2]) + red[3];
        const int c = *l.counter;
        l.ring[c % l.capacity] = tot * l.scale;
        *l.counter = c + 1;
    }
}

template <class Hyper>
__global__ __launch_bounds__(1024) void sgd_multi_kernel(const SgdMulti<Hyper> a) {
    int blk = blockIdx.x;
    if (a.loss.v) {
        // block 0 logs the loss (dispatched first: its serial sum overlaps the segments' blocks)
        if (blk == 0) {
            loss_log_block(a.loss);
            return;
        }
        --blk;
    }
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            if (blk < a.seg[s].nblk) {
                slab_reduce(nullptr, a.seg[s].slabs, a.seg[s].nslab, a.seg[s].n, blk,
                                                               a.hyper.apply(a.seg[s]));
                return;
            }
            blk -= a.seg[s].nblk;
        }
    }
}

// ---------------------------------------------------------------------------- global-norm gradient clipping
// torch.nn.utils.clip_grad_norm_ needs a stage's whole norm before its first parameter moves, so the fused
// reduce + step becomes two launches, neither with atomics: reduce_sqnorm_multi_kernel (the slab reduction
// as above, plus one partial of the squared norm per block) and sgdm_clip_multi_kernel (every block sums its
// group's partials in one fixed order, forms the coefficient and steps from coef * grad).
//
// Pass 1, one block: slab_reduce on its columns (so `grad` gets the bits slk_sgdm_from_slabs writes), the
// applying thread of each column keeping q = t * t; every other thread — columns past n, and in the 256- and
// 64-column forms the waves that only sum slabs (waves 4..15 / 1..15) — keeps q = 0. Then
// slk_block_sum_1024(q): wave_sum inside each wave, the 16 wave sums added in ascending wave order; thread 0
// writes the block's partial. grad == NULL: the gradient block already holds the sum (nslab 1, in place).
struct SqApply {
    float* __restrict__ grad;
    float* q;
    __device__ __forceinline__ void operator()(int i, float t) const {
        if (grad) grad[i] = t;
        *q = t * t;
    }
};
struct RsqSeg {
    float* grad;
    const float* slabs;
    float* partials;  // this segment's slice of its group's partials
    int nslab, n, nblk;
};
struct RsqMulti {
    RsqSeg seg[SGD_MAXSEG];
    int nseg;
    LossLogArgs loss;
};

__global__ __launch_bounds__(1024) void reduce_sqnorm_multi_kernel(const RsqMulti a) {
    __shared__ float red[16];
    int blk = blockIdx.x;
    if (a.loss.v) {
        if (blk == 0) {
            loss_log_block(a.loss);
            return;
        }
        --blk;
    }
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            const RsqSeg& g = a.seg[s];
            if (blk < g.nblk) {
                float q = 0.f;
                slab_reduce(nullptr, g.slabs, g.nslab, g.n, blk, SqApply{g.grad, &q});
                slk_keep(q);  // the square is rounded on its own (never fused into the first add of wave_sum)
                const float tot = slk_block_sum_1024(q, red);
                if (threadIdx.x == 0) g.partials[blk] = tot;
                return;
            }
            blk -= g.nblk;
        }
    }
}

// Pass 2: thread = element, 1024 per block. SgdmApply's arithmetic on coef * grad[i], one f32 multiply
// rounded on its own (clipping comes before weight decay); grad keeps the unclipped gradient.
struct ClipSeg {
    float* param;
    const float* grad;
    float* buf;
    const float* partials;  // the group's partials
    float* out;             // the group's [norm, coef]
    int n, nblk, npart, first;
};
struct SgdmClipMulti {
    ClipSeg seg[SGD_MAXSEG];
    int nseg;
    const float* max_norm;
    SgdmHyper h;
};

__global__ __launch_bounds__(1024) void sgdm_clip_multi_kernel(const SgdmClipMulti a) {
    __shared__ float red[16];
    int blk = blockIdx.x;
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            const ClipSeg& g = a.seg[s];
            if (blk < g.nblk) {
                float norm;
                const float coef = slk_clip_coef(g.partials, g.npart, a.max_norm, red, norm);
                if (g.first && blk == 0 && threadIdx.x == 0) {
                    g.out[0] = norm;
                    g.out[1] = coef;
                }
                const int i = blk * 1024 + threadIdx.x;
                if (i < g.n) {
                    float cg = coef * g.grad[i];
                    slk_keep(cg);
                    SgdmApply{g.param, nullptr, g.buf, a.h}(i, cg);
                }
                return;
            }
            blk -= g.nblk;
        }
    }
}

// ---------------------------------------------------------------------------- layer-wise trust ratios
// LARS (on SgdmApply) and LAMB (on slk_adam.h's arithmetic): a segment is one [W | b] pair, elements [0, nw) the
// weight tensor and [nw, n) the bias, and each tensor's step is scaled by a ratio of two of its own norms. Two
// launches where the configured step runs one, as with clipping, neither with atomics.
//
// Pass 1, one block: slab_reduce on its columns (grad gets slk_sgdm_from_slabs' / slk_adamw_from_slabs' bits);
// the applying thread of column i forms x^2 and p^2, each rounded on its own, and holds them in the weight pair
// (i < nw) or the bias pair of [x2_W, p2_W, x2_b, p2_b]; every other thread holds four zeros. LAMB's thread
// first moves and stores m and v and forms x = u (lamb_direction). Then four block sums (slk_block_sum_1024's
// order each); thread 0 writes the block's four partials. A block that straddles nw contributes to both tensors.
struct TnormSeg {
    float* grad;  // NULL: in place (the one slab is the gradient block)
    const float* param;
    float* m;     // LAMB only
    float* v;
    const float* slabs;
    float* partials;  // this segment's [nblk][4]
    int nslab, n, nw, nblk;
};
// the owning thread's two squares into the weight pair or the bias pair (selects: a NaN stays in its own tensor)
__device__ __forceinline__ void trust_squares(bool w, float x2, float p2, float* q) {
    q[0] = w ? x2 : 0.f;
    q[1] = w ? p2 : 0.f;
    q[2] = w ? 0.f : x2;
    q[3] = w ? 0.f : p2;
}
struct LarsSqApply {
    float* __restrict__ grad;
    const float* __restrict__ param;
    int nw;
    float* q;  // the thread's [x2_W, p2_W, x2_b, p2_b]
    __device__ __forceinline__ void operator()(int i, float t) const {
        if (grad) grad[i] = t;
        const float p = param[i];
        trust_squares(i < nw, t * t, p * p, q);
    }
};
struct LambMomentsApply {
    float* __restrict__ grad;
    const float* __restrict__ param;
    float* __restrict__ m_;
    float* __restrict__ v_;
    int nw;
    AdamHyper h;
    int exclude_bias;
    float* q;
    __device__ __forceinline__ void operator()(int i, float t) const {
        if (grad) grad[i] = t;
        const float p = param[i];
        const AdamBias bc = adam_bias<true>(h.b1, h.b2, h.step, 0.f);
        float m = m_[i], v = v_[i];
        adam_moments(t, m, v, h.b1, h.b2);
        m_[i] = m;
        v_[i] = v;
        const bool w = i < nw;
        const float u = lamb_direction(m, v, p, bc, h.eps, (w || !exclude_bias) ? h.wd : 0.f);
        trust_squares(w, u * u, p * p, q);
    }
};
struct TnormMulti {
    TnormSeg seg[SGD_MAXSEG];
    int nseg;
    AdamHyper h;  // LAMB only
    int exclude_bias;
    LossLogArgs loss;
};

template <bool LAMB>
__global__ __launch_bounds__(1024) void reduce_tnorm_multi_kernel(const TnormMulti a) {
    __shared__ float red[4][16];
    int blk = blockIdx.x;
    if (a.loss.v) {
        if (blk == 0) {
            loss_log_block(a.loss);
            return;
        }
        --blk;
    }
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            const TnormSeg& g = a.seg[s];
            if (blk < g.nblk) {
                float q[4] = {0.f, 0.f, 0.f, 0.f};
                if (LAMB)
                    slab_reduce(nullptr, g.slabs, g.nslab, g.n, blk,
                                LambMomentsApply{g.grad, g.param, g.m, g.v, g.nw, a.h, a.exclude_bias, q});
                else
                    slab_reduce(nullptr, g.slabs, g.nslab, g.n, blk, LarsSqApply{g.grad, g.param, g.nw, q});
#pragma unroll
                for (int k = 0; k < 4; ++k) slk_keep(q[k]);  // every square is rounded on its own
                slk_block_sum4_1024(q, red);
                if (threadIdx.x == 0) *reinterpret_cast<f32x4*>(g.partials + 4 * (size_t)blk) = f32x4{q[0], q[1], q[2], q[3]};
                return;
            }
            blk -= g.nblk;
        }
    }
}

// Pass 2: thread = element, 1024 per block. Every block sums its segment's partials (slk_tensor_totals: one
// fixed order per component), forms the weight's and the bias's ratio and steps its elements; block 0 reports
// the weight tensor, the block that holds element nw the bias: [w_norm, x_norm, ratio] each.
struct TrustSeg {
    float* param;
    const float* grad;  // LARS only
    float* s1;          // LARS: momentum buffer; LAMB: m
    float* s2;          // LAMB: v
    const float* partials;
    float* out;  // this segment's [2][3]: the weight's row, then the bias's
    int n, nw, nblk, npart;
};
struct LarsMulti {
    TrustSeg seg[SGD_MAXSEG];
    int nseg;
    SgdmHyper h;
    float trust_coef, eps;
    int exclude_bias;
};
struct LambMulti {
    TrustSeg seg[SGD_MAXSEG];
    int nseg;
    AdamHyper h;
    int exclude_bias;
};
__device__ __forceinline__ void trust_report(const TrustSeg& g, int blk, const float (&w)[3], const float (&b)[3]) {
    if (threadIdx.x != 0) return;
    if (blk == 0 && g.nw > 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g.out[k] = w[k];
    }
    if (blk == g.nw / 1024 && g.nw < g.n) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g.out[3 + k] = b[k];
    }
}

// LARS: d = fl(ratio * (g + fl(wd * p))), then SgdmApply's momentum / dampening / Nesterov arithmetic on d
// at weight decay 0. An excluded bias runs at ratio 1 and weight decay 0: d = g, slk_sgdm_from_slabs' bits.
__global__ __launch_bounds__(1024) void lars_multi_kernel(const LarsMulti a) {
    __shared__ float red[4][16];
    int blk = blockIdx.x;
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            const TrustSeg& g = a.seg[s];
            if (blk < g.nblk) {
                float tot[4], w[3], b[3];
                slk_tensor_totals(g.partials, g.npart, red, tot);
                const float wd = a.h.weight_decay, wd_b = a.exclude_bias ? 0.f : wd;
                w[2] = slk_lars_ratio(tot[0], tot[1], a.trust_coef, wd, a.eps, w[0], w[1]);
                b[2] = slk_lars_ratio(tot[2], tot[3], a.trust_coef, wd_b, a.eps, b[0], b[1]);
                if (a.exclude_bias) b[2] = 1.f;
                trust_report(g, blk, w, b);
                const int i = blk * 1024 + threadIdx.x;
                if (i < g.n) {
                    const bool isw = i < g.nw;
                    const float ratio = isw ? w[2] : b[2], wde = isw ? wd : wd_b;
                    float d = g.grad[i];
                    if (wde != 0.f) {
                        float wp = wde * g.param[i];
                        slk_keep(wp);
                        d = d + wp;
                    }
                    d = ratio * d;
                    slk_keep(d);
                    SgdmHyper h0 = a.h;
                    h0.weight_decay = 0.f;
                    SgdmApply{g.param, nullptr, g.s1, h0}(i, d);
                }
                return;
            }
            blk -= g.nblk;
        }
    }
}

// LAMB: u from the stored m, v and the still unmodified p (pass 1's expression and bits), then
// p = p - fl(fl(lr * ratio) * u). An excluded bias, and a tensor whose parameters are all zero (w_norm = 0:
// ratio 1 and no decay term), step by adam_step: slk_adamw_from_slabs' bits at weight decay 0.
__global__ __launch_bounds__(1024) void lamb_multi_kernel(const LambMulti a) {
    __shared__ float red[4][16];
    int blk = blockIdx.x;
#pragma unroll
    for (int s = 0; s < SGD_MAXSEG; ++s) {
        if (s < a.nseg) {
            const TrustSeg& g = a.seg[s];
            if (blk < g.nblk) {
                float tot[4], w[3], b[3];
                slk_tensor_totals(g.partials, g.npart, red, tot);
                w[2] = slk_lamb_ratio(tot[0], tot[1], w[0], w[1]);
                b[2] = slk_lamb_ratio(tot[2], tot[3], b[0], b[1]);
                if (a.exclude_bias) b[2] = 1.f;
                trust_report(g, blk, w, b);
                const int i = blk * 1024 + threadIdx.x;
                if (i < g.n) {
                    const bool isw = i < g.nw;
                    const float lr = slk_lr_at(a.h.lr_table, a.h.lr_len, *a.h.step);
                    const AdamBias bc = adam_bias<true>(a.h.b1, a.h.b2, a.h.step, lr);
                    const float p = g.param[i], m = g.s1[i], v = g.s2[i];
                    const bool excluded = !isw && a.exclude_bias;
                    if (excluded || (isw ? w[0] : b[0]) == 0.f) {
                        // ratio 1 and no decay term (p = 0 throughout, or an excluded bias): the same update
                        // in slk_adamw_from_slabs' own expression, so its bits at weight decay 0
                        g.param[i] = adam_step(p, m, adam_denom(v, bc.bc2s, a.h.eps), bc.step_size);
                    } else {
                        const float u = lamb_direction(m, v, p, bc, a.h.eps, a.h.wd);
                        float r = lr * (isw ? w[2] : b[2]);
                        slk_keep(r);
                        float ru = r * u;
                        slk_keep(ru);
                        g.param[i] = p - ru;
                    }
                }
                return;
            }
            blk -= g.nblk;
        }
    }
}

static inline int grid_for(int n) {
    int g = (n + 255) / 256;
    return g > 2048 ? 2048 : (g < 1 ? 1 : g);
}

extern "C" int slk_reduce_slabs(const float* slabs, int nslab, int n, float* out, int accumulate,
                                void* stream) {
    SLK_CHECK_ARG(nslab >= 0 && n >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(out && (slabs || nslab == 0));
    sgd_from_slabs_kernel<<<rs_blocks(n, nslab), 1024, 0, slk_stream(stream)>>>(nullptr, out, slabs, nslab, n, 0.f,
                                                                           accumulate ? 1 : 0);
    return slk_launch_status();
}

extern "C" int slk_sgd_from_slabs(float* param, float* grad, const float* slabs, int nslab, int n,
                                  float lr, void* stream) {
    SLK_CHECK_ARG(nslab >= 0 && n >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(param && (slabs || nslab == 0));
    sgd_from_slabs_kernel<<<rs_blocks(n, nslab), 1024, 0, slk_stream(stream)>>>(param, grad, slabs, nslab, n, lr, 0);
    return slk_launch_status();
}

extern "C" int slk_sgd_multi_from_slabs(float* const* params, float* const* grads, const float* const* slabs,
                                        const int* nslab, const int* n, int nseg, float lr,
                                        const float* loss_values, int loss_n, float loss_scale, float* ring,
                                        int capacity, int* counter, void* stream) {
    SLK_CHECK_ARG(nseg >= 0 && nseg <= SGD_MAXSEG && (nseg == 0 || (params && slabs && nslab && n)));
    SLK_CHECK_ARG(!loss_values || (loss_n > 0 && capacity > 0 && ring && counter));
    SgdMulti<SgdHyper> a{};
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        // a segment with no param is a reduce only (grad = sum of slabs): the all-reduce bucket fill
        SLK_CHECK_ARG(n[s] >= 0 && nslab[s] >= 0 && (params[s] || (grads && grads[s])) && (slabs[s] || nslab[s] == 0));
        a.seg[s] = SgdSeg{params[s], grads ? grads[s] : nullptr, nullptr, slabs[s], nslab[s], n[s],
                          rs_blocks(n[s], nslab[s])};
        nblk += a.seg[s].nblk;
    }
    a.nseg = nseg;
    a.hyper.lr = lr;
    a.loss = LossLogArgs{loss_values, loss_n, loss_scale, ring, capacity, counter};
    if (loss_values) ++nblk;
    if (nblk == 0) return 0;
    sgd_multi_kernel<SgdHyper><<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

extern "C" int slk_sgdm_from_slabs(float* param, float* grad, float* buf, const float* slabs, int nslab, int n,
                                   const float* lr_table, int lr_len, const int* step, float momentum,
                                   float dampening, float weight_decay, int nesterov, void* stream) {
    SLK_CHECK_ARG(nslab > 0 && n >= 0 && lr_len >= 1);
    SLK_CHECK_ARG(param && slabs && lr_table && step && (buf || momentum == 0.f));
    if (n == 0) return 0;
    const SgdmHyper h{lr_table, lr_len, step, momentum, dampening, weight_decay, nesterov ? 1 : 0};
    sgdm_from_slabs_kernel<<<rs_blocks(n, nslab), 1024, 0, slk_stream(stream)>>>(param, grad, buf, slabs, nslab, n, h);
    return slk_launch_status();
}

extern "C" int slk_sgdm_multi_from_slabs(float* const* params, float* const* grads, float* const* bufs,
                                         const float* const* slabs, const int* nslab, const int* n, int nseg,
                                         const float* lr_table, int lr_len, const int* step, float momentum,
                                         float dampening, float weight_decay, int nesterov,
                                         const float* loss_values, int loss_n, float loss_scale, float* ring,
                                         int capacity, int* counter, void* stream) {
    SLK_CHECK_ARG(nseg >= 0 && nseg <= SGD_MAXSEG && lr_len >= 1 && lr_table && step);
    SLK_CHECK_ARG(nseg == 0 || (params && slabs && nslab && n && (bufs || momentum == 0.f)));
    SLK_CHECK_ARG(!loss_values || (loss_n > 0 && capacity > 0 && ring && counter));
    SgdMulti<SgdmMultiHyper> a{};
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        SLK_CHECK_ARG(n[s] >= 0 && nslab[s] > 0 && params[s] && slabs[s] && (momentum == 0.f || bufs[s]));
        a.seg[s] = SgdSeg{params[s], grads ? grads[s] : nullptr, bufs ? bufs[s] : nullptr, slabs[s], nslab[s], n[s],
                          rs_blocks(n[s], nslab[s])};
        nblk += a.seg[s].nblk;
    }
    a.nseg = nseg;
    a.hyper.h = SgdmHyper{lr_table, lr_len, step, momentum, dampening, weight_decay, nesterov ? 1 : 0};
    a.loss = LossLogArgs{loss_values, loss_n, loss_scale, ring, capacity, counter};
    if (loss_values) ++nblk;
    if (nblk == 0) return 0;
    sgd_multi_kernel<SgdmMultiHyper><<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

extern "C" int slk_reduce_sqnorm_nblk(int n, int nslab) { return n > 0 && nslab > 0 ? rs_blocks(n, nslab) : 0; }

extern "C" int slk_reduce_sqnorm_multi(float* const* grads, const float* const* slabs, const int* nslab,
                                       const int* n, const int* group, int nseg, float* const* partials,
                                       int ngroup, const float* loss_values, int loss_n, float loss_scale,
                                       float* ring, int capacity, int* counter, void* stream) {
    static_assert(SGD_MAXSEG == SLK_CLIP_MAXSEG, "clip layout");
    SLK_CHECK_ARG(grads && slabs && partials);
    SLK_CHECK_ARG(!loss_values || (loss_n > 0 && capacity > 0 && ring && counter));
    SlkClipLayout L;
    SLK_CHECK_ARG(slk_clip_layout(nslab, n, group, nseg, ngroup, L));
    RsqMulti a{};
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        SLK_CHECK_ARG(grads[s] && slabs[s] && partials[group[s]]);
        // in place: the gradient block is the one slab (after a reduce / all-reduce); nothing is written to it
        const bool in_place = grads[s] == slabs[s];
        SLK_CHECK_ARG(!in_place || nslab[s] == 1);
        a.seg[s] = RsqSeg{in_place ? nullptr : grads[s], slabs[s], partials[group[s]] + L.off[s], nslab[s], n[s],
                          L.nblk[s]};
        nblk += L.nblk[s];
    }
    a.nseg = nseg;
    a.loss = LossLogArgs{loss_values, loss_n, loss_scale, ring, capacity, counter};
    if (loss_values) ++nblk;
    if (nblk == 0) return 0;
    reduce_sqnorm_multi_kernel<<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

extern "C" int slk_sgdm_clip_multi(float* const* params, const float* const* grads, float* const* bufs,
                                   const int* nslab, const int* n, const int* group, int nseg,
                                   const float* const* partials, float* const* norm_out, int ngroup,
                                   const float* max_norm, const float* lr_table, int lr_len, const int* step,
                                   float momentum, float dampening, float weight_decay, int nesterov,
                                   void* stream) {
    SLK_CHECK_ARG(params && grads && partials && norm_out && max_norm && lr_table && lr_len >= 1 && step);
    SLK_CHECK_ARG(bufs || momentum == 0.f);
    SlkClipLayout L;
    SLK_CHECK_ARG(slk_clip_layout(nslab, n, group, nseg, ngroup, L));
    SgdmClipMulti a{};
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        SLK_CHECK_ARG(params[s] && grads[s] && partials[group[s]] && norm_out[group[s]] && (momentum == 0.f || bufs[s]));
        a.seg[s] = ClipSeg{params[s], grads[s], bufs ? bufs[s] : nullptr, partials[group[s]], norm_out[group[s]], n[s],
                           (n[s] + 1023) / 1024, L.npart[s], L.first[s]};
        nblk += a.seg[s].nblk;
    }
    a.nseg = nseg;
    a.max_norm = max_norm;
    a.h = SgdmHyper{lr_table, lr_len, step, momentum, dampening, weight_decay, nesterov ? 1 : 0};
    if (nblk == 0) return 0;
    sgdm_clip_multi_kernel<<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

// ---- layer-wise trust ratios: host side
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// pass 1 of either recipe (m, v NULL: LARS)
static int tnorm_launch(bool lamb, float* const* grads, const float* const* params, float* const* m, float* const* v,
                        const float* const* slabs, const int* nslab, const int* n, const int* nw, const int* group,
                        int nseg, float* const* partials, int ngroup, const AdamHyper& h, int exclude_bias,
                        const LossLogArgs& loss, void* stream) {
    SLK_CHECK_ARG(grads && params && slabs && partials && (!lamb || (m && v)));
    SLK_CHECK_ARG(!loss.v || (loss.n > 0 && loss.capacity > 0 && loss.ring && loss.counter));
    SlkTrustLayout L;
    SLK_CHECK_ARG(slk_trust_layout(nslab, n, nw, group, nseg, ngroup, L));
    TnormMulti a{};
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        float* part = partials[group[s]];
        SLK_CHECK_ARG(grads[s] && params[s] && slabs[s] && part && aligned16(part) && (!lamb || (m[s] && v[s])));
        const bool in_place = grads[s] == slabs[s];
        SLK_CHECK_ARG(!in_place || nslab[s] == 1);
        a.seg[s] = TnormSeg{in_place ? nullptr : grads[s], params[s], lamb ? m[s] : nullptr, lamb ? v[s] : nullptr,
                            slabs[s], part + 4 * (size_t)L.c.off[s], nslab[s], n[s], nw[s], L.c.nblk[s]};
        nblk += L.c.nblk[s];
    }
    a.nseg = nseg;
    a.h = h;
    a.exclude_bias = exclude_bias ? 1 : 0;
    a.loss = loss;
    if (loss.v) ++nblk;
    if (nblk == 0) return 0;
    if (lamb)
        reduce_tnorm_multi_kernel<true><<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    else
        reduce_tnorm_multi_kernel<false><<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

// the segments of pass 2 (s1, s2: buf, NULL or m, v); returns the launch's block count or -1
static int trust_segs(TrustSeg* seg, float* const* params, const float* const* grads, float* const* s1,
                      float* const* s2, const int* nslab, const int* n, const int* nw, const int* group, int nseg,
                      const float* const* partials, float* const* trust_out, int ngroup) {
    if (!params || !partials || !trust_out) return -1;
    SlkTrustLayout L;
    if (!slk_trust_layout(nslab, n, nw, group, nseg, ngroup, L)) return -1;
    int nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        const float* part = partials[group[s]];
        float* out = trust_out[group[s]];
        if (!params[s] || !part || !aligned16(part) || !out || (grads && !grads[s]) || (s1 && !s1[s]) ||
            (s2 && !s2[s]))
            return -1;
        seg[s] = TrustSeg{params[s], grads ? grads[s] : nullptr, s1 ? s1[s] : nullptr, s2 ? s2[s] : nullptr,
                          part + 4 * (size_t)L.c.off[s], out + 6 * L.slot[s], n[s], nw[s], (n[s] + 1023) / 1024,
                          L.c.nblk[s]};
        nblk += seg[s].nblk;
    }
    return nblk;
}

extern "C" int slk_reduce_tnorm_multi(float* const* grads, const float* const* params, const float* const* slabs,
                                      const int* nslab, const int* n, const int* nw, const int* group, int nseg,
                                      float* const* partials, int ngroup, const float* loss_values, int loss_n,
                                      float loss_scale, float* ring, int capacity, int* counter, void* stream) {
    static_assert(SGD_MAXSEG == SLK_CLIP_MAXSEG, "trust layout");
    return tnorm_launch(false, grads, params, nullptr, nullptr, slabs, nslab, n, nw, group, nseg, partials, ngroup,
                        AdamHyper{}, 0, LossLogArgs{loss_values, loss_n, loss_scale, ring, capacity, counter}, stream);
}

extern "C" int slk_lars_multi(float* const* params, const float* const* grads, float* const* bufs, const int* nslab,
                              const int* n, const int* nw, const int* group, int nseg, const float* const* partials,
                              float* const* trust_out, int ngroup, const float* lr_table, int lr_len,
                              const int* step, float momentum, float dampening, float weight_decay, int nesterov,
                              float trust_coef, float eps, int exclude_bias, void* stream) {
    SLK_CHECK_ARG(grads && lr_table && lr_len >= 1 && step && (bufs || momentum == 0.f));
    LarsMulti a{};
    const int nblk = trust_segs(a.seg, params, grads, momentum != 0.f ? bufs : nullptr, nullptr, nslab, n, nw, group,
                                nseg, partials, trust_out, ngroup);
    SLK_CHECK_ARG(nblk >= 0);
    a.nseg = nseg;
    a.h = SgdmHyper{lr_table, lr_len, step, momentum, dampening, weight_decay, nesterov ? 1 : 0};
    a.trust_coef = trust_coef;
    a.eps = eps;
    a.exclude_bias = exclude_bias ? 1 : 0;
    if (nblk == 0) return 0;
    lars_multi_kernel<<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

extern "C" int slk_lamb_moments_multi(float* const* grads, const float* const* params, float* const* m,
                                      float* const* v, const float* const* slabs, const int* nslab, const int* n,
                                      const int* nw, const int* group, int nseg, float* const* partials, int ngroup,
                                      const int* step, float beta1, float beta2, float eps, float weight_decay,
                                      int exclude_bias, const float* loss_values, int loss_n, float loss_scale,
                                      float* ring, int capacity, int* counter, void* stream) {
    SLK_CHECK_ARG(step);
    return tnorm_launch(true, grads, params, m, v, slabs, nslab, n, nw, group, nseg, partials, ngroup,
                        AdamHyper{0.f, nullptr, 0, weight_decay, 0, beta1, beta2, eps, step}, exclude_bias,
                        LossLogArgs{loss_values, loss_n, loss_scale, ring, capacity, counter}, stream);
}

extern "C" int slk_lamb_multi(float* const* params, float* const* m, float* const* v, const int* nslab,
                              const int* n, const int* nw, const int* group, int nseg, const float* const* partials,
                              float* const* trust_out, int ngroup, const float* lr_table, int lr_len,
                              const int* step, float beta1, float beta2, float eps, float weight_decay,
                              int exclude_bias, void* stream) {
    SLK_CHECK_ARG(m && v && lr_table && lr_len >= 1 && step);
    LambMulti a{};
    const int nblk = trust_segs(a.seg, params, nullptr, m, v, nslab, n, nw, group, nseg, partials, trust_out, ngroup);
    SLK_CHECK_ARG(nblk >= 0);
    a.nseg = nseg;
    a.h = AdamHyper{0.f, lr_table, lr_len, weight_decay, 0, beta1, beta2, eps, step};
    a.exclude_bias = exclude_bias ? 1 : 0;
    if (nblk == 0) return 0;
    lamb_multi_kernel<<<nblk, 1024, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}

extern "C" int slk_sgd(float* param, const float* grad, int n, float lr, void* stream) {
    SLK_CHECK_ARG(n >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(param && grad);
    sgd_kernel<<<grid_for(n), 256, 0, slk_stream(stream)>>>(param, grad, n, lr);
    return slk_launch_status();
}

extern "C" int slk_loss_sum(const float* values, int n, float scale, float* out, void* stream) {
    SLK_CHECK_ARG(n > 0);
    SLK_CHECK_ARG(values && out);
    loss_sum_kernel<<<1, 256, 0, slk_stream(stream)>>>(values, n, scale, out);
    return slk_launch_status();
}

extern "C" int slk_loss_log(const float* values, int n, float scale, float* ring, int capacity,
                            int* counter, void* stream) {
    SLK_CHECK_ARG(n > 0 && capacity > 0);
    SLK_CHECK_ARG(values && ring && counter);
    loss_log_kernel<<<1, 256, 0, slk_stream(stream)>>>(values, n, scale, ring, capacity, counter);
    return slk_launch_status();
}

extern "C" int slk_abi_version(void) { return SLK_ABI_VERSION; }

// sha256 of the library's sources (splitcnn/build.py source_hash), baked in at compile time so the
// loader can refuse a binary built from other sources; the tag is also searchable in the file.
#ifndef SLK_BUILD_ID
#define SLK_BUILD_ID "unknown"
#endif
extern "C" __attribute__((used, visibility("default"))) const char slk_build_id_tag[] = "SLK_BUILD_ID:" SLK_BUILD_ID;
extern "C" const char* slk_build_id(void) { return slk_build_id_tag + 13; }

extern "C" const char* slk_error_string(int err) {
    return hipGetErrorString(static_cast<hipError_t>(err));
}
