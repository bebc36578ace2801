// slk_adam.h — the per-element Adam arithmetic, shared by the fused reduce + Adam kernels (slk_wide_head.hip)
// and the LAMB passes (slk_optim.hip). Internal; not part of the ABI.
#pragma once

#include "slk_common.h"

// Hyper-parameters of one Adam launch. TABLE = false is torch.optim.Adam(lr) as above (lr by value);
// TABLE = true (slk_adamw_*) reads the rate from a device table at *step (slk_lr_at) and applies weight
// decay: decoupled (torch.optim.AdamW: p *= 1 - lr * wd before the update, the factor in double like torch's
// Python float) or coupled (torch.optim.Adam(weight_decay): g += wd * p before the moments).
struct AdamHyper {
    float lr;
    const float* lr_table;
    int lr_len;
    float wd;
    int decoupled;
    float b1, b2, eps;
    const int* step;
};

// The bias corrections of step t = *step + 1, in double like torch's Python floats, then rounded:
// step_size = lr / (1 - b1^t), bc2s = sqrt(1 - b2^t); for LAMB's m-hat also rbc1 = 1 / (1 - b1^t).
struct AdamBias {
    float step_size, bc2s, rbc1;
};
template <bool RBC1 = false>
__device__ __forceinline__ AdamBias adam_bias(float b1, float b2, const int* step, float lr) {
    const double tt = (double)(*step + 1);
    const double bc1 = 1.0 - pow((double)b1, tt);
    const float step_size = (float)((double)lr / bc1);
    const float bc2s = (float)sqrt(1.0 - pow((double)b2, tt));
    return AdamBias{step_size, bc2s, RBC1 ? (float)(1.0 / bc1) : 0.f};
}
// m = m + (1-b1)(g - m)  [lerp]; v = v*b2 + (1-b2) g*g  [mul_ + addcmul_]
__device__ __forceinline__ void adam_moments(float t, float& m, float& v, float b1, float b2) {
    m = m + (1.f - b1) * (t - m);
    v = v * b2 + t * t * (1.f - b2);
}
// sqrt(v) / sqrt(1 - b2^t) + eps
__device__ __forceinline__ float adam_denom(float v, float bc2s, float eps) { return sqrtf(v) / bc2s + eps; }

// p = p - step_size * m / denom  [addcdiv_]: ONE fused multiply-add, asked for by name. Left to contraction, the
// fourth segment slot of lamb_multi_kernel merged this line's tail with LAMB's p - fl(r u) into a shared v_sub_f32 and
// rounded the product on its own, so an excluded bias there missed slk_adamw_from_slabs' bits.
__device__ __forceinline__ float adam_step(float p, float m, float denom, float step_size) {
    return __builtin_fmaf(-step_size, m / denom, p);
}

// the Adam update of element i from its summed gradient t (shared by the reduction forms)
template <bool TABLE>
__device__ __forceinline__ void adam_apply(int i, float t, float* __restrict__ param, float* __restrict__ grad,
                                           float* __restrict__ m_, float* __restrict__ v_, const AdamHyper& h) {
    if (grad) grad[i] = t;
    const float b1 = h.b1, b2 = h.b2, eps = h.eps;
    const float lr = TABLE ? slk_lr_at(h.lr_table, h.lr_len, *h.step) : h.lr;
    float p = param[i];
    if (TABLE && h.wd != 0.f) {
        if (h.decoupled)
            p = p * (float)(1.0 - (double)lr * (double)h.wd);
        else
            t = t + h.wd * p;
    }
    const AdamBias bc = adam_bias(b1, b2, h.step, lr);
    float m = m_[i], v = v_[i];
    adam_moments(t, m, v, b1, b2);
    const float denom = adam_denom(v, bc.bc2s, eps);
    param[i] = adam_step(p, m, denom, bc.step_size);
    m_[i] = m;
    v_[i] = v;
}

// LAMB's update direction of one element from its moved moments and its parameter before the step:
// u = fl(fl(m / denom) * rbc1) + fl(wd * p), both products rounded on their own (pass 1 and pass 2 of
// slk_lamb_* evaluate this on the same stored bits and must agree bit for bit).
__device__ __forceinline__ float lamb_direction(float m, float v, float p, const AdamBias& bc, float eps, float wd) {
    float c = m / adam_denom(v, bc.bc2s, eps);
    slk_keep(c);
    float u = c * bc.rbc1;
    slk_keep(u);
    if (wd != 0.f) {
        float wp = wd * p;
        slk_keep(wp);
        u = u + wp;
    }
    return u;
}
