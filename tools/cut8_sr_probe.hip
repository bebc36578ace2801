// cut8_sr_probe.hip — the bare v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32 of gfx950 for tools/cut8_sr_check.py: what the
// instruction returns for a given (y, r), and over how many random words it rounds up. Check only; not part of
// libslk. Built by `python tools/cut8_sr_check.py --build-probe` into build_abl/cut8_sr_probe.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
template <int FMT> __device__ __forceinline__ uint32_t cvt_sr(float y, uint32_t r) {
    const int w = FMT == 0 ? __builtin_amdgcn_cvt_sr_fp8_f32(y, r, 0, 0) : __builtin_amdgcn_cvt_sr_bf8_f32(y, r, 0, 0);
    return (uint32_t)w & 0xffu;
}

// code[i] = cvt(y[i], r[i])
template <int FMT> __global__ void pairs_kernel(const float* y, const uint32_t* r, int n, uint8_t* code) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) code[i] = (uint8_t)cvt_sr<FMT>(y[i], r[i]);
}

// Block b: count[b] = the number of j in [0, 2^bits) with cvt(y[b], j << shift) != lo[b]; 256 threads.
template <int FMT>
__global__ __launch_bounds__(256) void count_kernel(const float* y, const uint8_t* lo, int bits, int shift, uint32_t* count) {
    __shared__ uint32_t red[256];
    const float v = y[blockIdx.x];
    const uint32_t down = lo[blockIdx.x];
    uint32_t c = 0;
    for (uint32_t j = threadIdx.x; j < (1u << bits); j += 256) c += cvt_sr<FMT>(v, j << shift) != down ? 1u : 0u;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[blockIdx.x] = red[0];
}
}  // namespace

extern "C" int probe_pairs(const float* y, const uint32_t* r, int n, int fmt, uint8_t* code, void* stream) {
    if (n <= 0 || !y || !r || !code || (fmt != 0 && fmt != 1)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (fmt == 0) pairs_kernel<0><<<(n + 255) / 256, 256, 0, st>>>(y, r, n, code);
    else pairs_kernel<1><<<(n + 255) / 256, 256, 0, st>>>(y, r, n, code);
    return (int)hipGetLastError();
}

extern "C" int probe_count(const float* y, const uint8_t* lo, int n, int fmt, int bits, int shift, uint32_t* count, void* stream) {
    if (n <= 0 || !y || !lo || !count || (fmt != 0 && fmt != 1) || bits < 8 || bits > 24 || shift < 0 || bits + shift > 32) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (fmt == 0) count_kernel<0><<<n, 256, 0, st>>>(y, lo, bits, shift, count);
    else count_kernel<1><<<n, 256, 0, st>>>(y, lo, bits, shift, count);
    return (int)hipGetLastError();
}
