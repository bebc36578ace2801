// slk_eval.hip — evaluation / prediction: per-sample loss + argmax from logits in memory, and the metric
// accumulator that sums them over a whole dataset on the device.
//
// The reference builds a test split and never uses it (src/client_part.py:52,73); a user's
//     model.eval(); for x, y in test_loader: out = model(x); loss += criterion(out, y); correct += (out.argmax(1) == y).sum()
// loop is what these kernels stand in for, with no host sync per batch: the counters live in device memory
// (layout in include/slk.h) and a stream's launches update them in order. The fc head's own evaluation mode
// (logits -> loss_i / pred inside the head's launch) is fc_head16_kernel<9> in slk_server.hip; both use
// slk_eval_row (slk_eval.h), so their bits agree.
#include "slk_eval.h"

using namespace slk;

// One thread per sample: 40 B read, 12 B written.
__global__ __launch_bounds__(256) void eval_logits_kernel(const float* __restrict__ logits,
                                                          const int64_t* __restrict__ labels, int B,
                                                          float* __restrict__ loss_i, int64_t* __restrict__ pred,
                                                          int* err_flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    float z[NCLS];
#pragma unroll
    for (int jj = 0; jj < NCLS; ++jj) z[jj] = logits[(size_t)i * NCLS + jj];
    slk_eval_row(z, labels, (size_t)i, loss_i, pred, err_flag);
}

// One workgroup per launch. Thread t takes samples t, t + 256, ...: its loss values summed in float64 in that
// order, the 64 lanes of a wave combined by a fixed butterfly, the 4 wave sums added in wave order by thread 0,
// which then read-modify-writes acc[0..3] (no global atomics: launches on a stream are ordered). The integer
// counts go through LDS integer adds (exact in any order) and leave as plain stores by threads 0-99.
constexpr int EVA_T = 256, EVA_NCONF = NCLS * NCLS;
__global__ __launch_bounds__(EVA_T) void eval_accumulate_kernel(const float* __restrict__ loss_i,
                                                                const int64_t* __restrict__ pred,
                                                                const int64_t* __restrict__ labels, int B,
                                                                int64_t* __restrict__ acc) {
    __shared__ unsigned int conf[EVA_NCONF];
    __shared__ unsigned int cnt[2];  // correct, bad labels
    __shared__ double wsum[EVA_T / 64];
    const int tid = threadIdx.x;
    if (tid < EVA_NCONF) conf[tid] = 0u;
    if (tid < 2) cnt[tid] = 0u;
    __syncthreads();
    double ls = 0.0;
    for (int64_t i = tid; i < B; i += EVA_T) {
        const int64_t y = labels[i], p = pred[i];
        if (y >= 0 && y < NCLS) {
            ls += (double)loss_i[i];
            if (p == y) atomicAdd(&cnt[0], 1u);
            if (p >= 0 && p < NCLS) atomicAdd(&conf[(int)y * NCLS + (int)p], 1u);
        } else {
            atomicAdd(&cnt[1], 1u);
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) ls += __shfl_xor(ls, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = ls;
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
#pragma unroll
        for (int w = 1; w < EVA_T / 64; ++w) t += wsum[w];
        acc[0] += (int64_t)B;
        acc[1] += (int64_t)cnt[0];
        acc[2] += (int64_t)cnt[1];
        double* lsum = reinterpret_cast<double*>(acc + 3);
        *lsum = *lsum + t;
    }
    if (tid < EVA_NCONF) acc[4 + tid] += (int64_t)conf[tid];
}

extern "C" int slk_eval_logits(const float* logits, const int64_t* labels, int B, float* loss_i, int64_t* pred,
                               int* err_flag, void* stream) {
    SLK_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(logits && pred && (!labels || loss_i));
    eval_logits_kernel<<<(B + 255) / 256, 256, 0, slk_stream(stream)>>>(logits, labels, B, loss_i, pred, err_flag);
    return slk_launch_status();
}

extern "C" int slk_eval_accumulate(const float* loss_i, const int64_t* pred, const int64_t* labels, int B,
                                   int64_t* acc, void* stream) {
    SLK_CHECK_ARG(B >= 0);
    if (B == 0) return 0;
    SLK_CHECK_ARG(loss_i && pred && labels && acc && ((uintptr_t)acc & 7) == 0);
    eval_accumulate_kernel<<<1, EVA_T, 0, slk_stream(stream)>>>(loss_i, pred, labels, B, acc);
    return slk_launch_status();
}
