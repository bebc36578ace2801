// slk_eval.h — the per-sample evaluation stage shared by fc_head16_kernel<MODE & 8> (slk_server.hip) and
// eval_logits_kernel (slk_eval.hip): one function, so both give the same loss_i / pred bits from the same logits.
#pragma once

#include "slk_common.h"

// z = the sample's 10 logits. pred[i] = argmax z as numpy.argmax does it: the first maximum wins on exact ties and
// a NaN counts as the maximum (the first NaN wins). With labels: loss_i[i] = logsumexp(z) - z[y] in the expression
// order of fc_head16_kernel's cross-entropy stage (bitwise training's loss_i); a label outside [0, 10) gives NaN and
// sets *err_flag (may be null). labels == null (predict only): loss_i and err_flag are not touched.
__device__ __forceinline__ void slk_eval_row(const float (&z)[slk::NCLS], const int64_t* __restrict__ labels, size_t i,
                                             float* __restrict__ loss_i, int64_t* __restrict__ pred, int* err_flag) {
    using slk::NCLS;
    int best = 0;
    float bv = z[0];
#pragma unroll
    for (int jj = 1; jj < NCLS; ++jj) {
        const bool take = !(bv != bv) && (z[jj] > bv || z[jj] != z[jj]);
        bv = take ? z[jj] : bv;
        best = take ? jj : best;
    }
    pred[i] = (int64_t)best;
    if (labels) {
        float m = z[0];
#pragma unroll
        for (int jj = 1; jj < NCLS; ++jj) m = fmaxf(m, z[jj]);
        float se = 0.f;
#pragma unroll
        for (int jj = 0; jj < NCLS; ++jj) se += expf(z[jj] - m);
        const float lse = m + logf(se);
        const int64_t y = labels[i];
        const bool ok = (y >= 0 && y < NCLS);
        if (!ok && err_flag) atomicOr(err_flag, 1);
        float yz = 0.f;
#pragma unroll
        for (int jj = 0; jj < NCLS; ++jj) yz = (jj == y) ? z[jj] : yz;
        const float nanv = __builtin_nanf("");
        loss_i[i] = ok ? (lse - yz) : nanv;
    }
}
