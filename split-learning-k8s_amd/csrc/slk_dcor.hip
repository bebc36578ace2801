// slk_dcor.hip — the distance correlation between a batch of raw inputs and its cut (include/slk.h, "Distance
// correlation"): dCor(x, z) of Székely et al. 2007 in its biased (V-statistic) form, from three launches and no
// n x n matrix in memory.
//
//   1. dcor_sqnorm_kernel: one block per sample, s_x[i] = |x_i|^2 and s_z[i] = |z_i|^2, summed in float64 and rounded
//      once to float32.
//   2. dcor_tile_kernel: one block of 256 threads (four waves, 2 x 2, a 64 x 64 quarter each) per 128 x 128 tile of
//      pairs with tj >= ti. It runs two K loops over the same 2 x 2 set of 32 x 32 accumulators: the Gram block of x
//      on v_mfma_f32_32x32x2_f32 (the image's float32 as stored), turned into the distances a_ij in registers, then
//      the Gram block of z on v_mfma_f32_32x32x16_bf16, turned into b_ij. Both operands are row-major with K
//      contiguous, so a K chunk is 128 bytes of every row (32 floats / 64 bf16) on both sides of the block and both
//      loops share the staging: a thread moves four 16-byte pieces per side from global memory into registers while
//      the MFMAs of the chunk before run out of LDS, then stores them into the other LDS buffer (rows padded to 144
//      bytes: the 16-byte fragment reads of 32 consecutive rows hit 64 distinct banks). One barrier per chunk. A lane
//      feeds the MFMAs of both sides with the same 16 bytes of its row, so K is visited in a permuted order that is
//      the same for A and B, and the accumulation chain restarts every 16 chunks (the chains are added up in
//      float32). A diagonal tile stages its rows once. Rows at or past n are read from row n - 1 and
//      masked in the epilogue by a select.
//      Epilogue, in registers and float64: the tile's sum of a b, a a and b b (doubled off the diagonal), its row
//      sums and — off the diagonal — its column sums, reduced by xor butterflies inside the wave and in a fixed order
//      across the waves through LDS. Every output slot has exactly one writer; there are no atomics.
//   3. dcor_finish_kernel: one block sums the row parts over the tiles per row, the five totals and the closed form
//      in float64, in one fixed order.
#include "slk_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int TILE = 128;               // pairs tile edge
constexpr int THREADS = 256;            // four waves: wave w owns rows 64 (w >> 1).., columns 64 (w & 1)..
constexpr int CHUNK_B = 128;            // bytes of one row in one K chunk: 32 floats or 64 bf16
constexpr int ROW_B = CHUNK_B + 16;     // padded LDS row
constexpr int SIDE_B = TILE * ROW_B;    // one side (the tile's rows or its columns) of one chunk
constexpr int STAGE_B = 2 * SIDE_B;
constexpr int PIECES = TILE * (CHUNK_B / 16) / THREADS;   // 16-byte pieces per thread and side: 4

// tau in units of 2^-24: see include/slk.h. K + 128 for the K of the K5 operands; tau itself is exact in float32.
constexpr int TAU_X_ULPS = 3072 + 128, TAU_Z_ULPS = 16384 + 128;
constexpr float TAU_X = TAU_X_ULPS * 0x1p-24f, TAU_Z = TAU_Z_ULPS * 0x1p-24f;

// ------------------------------------------------------------------------------------------------ workspace
// doubles first (8-byte aligned from a 16-byte aligned base), then the two float32 norm arrays.
struct Layout {
    int64_t T, Np, ntiles;
    int64_t off_rpa, off_rpb, off_tri, off_sx, off_sz, bytes;
};
inline Layout layout(int64_t n) {
    Layout L;
    L.T = (n + TILE - 1) / TILE;
    L.Np = L.T * TILE;
    L.ntiles = L.T * (L.T + 1) / 2;
    L.off_rpa = 0;
    L.off_rpb = L.off_rpa + 8 * L.T * L.Np;
    L.off_tri = L.off_rpb + 8 * L.T * L.Np;
    L.off_sx = L.off_tri + 8 * 3 * L.ntiles;
    L.off_sz = L.off_sx + 4 * L.Np;
    L.bytes = L.off_sz + 4 * L.Np;
    return L;
}

// ------------------------------------------------------------------------------------------------ reductions
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ 1. norms
__global__ __launch_bounds__(THREADS) void dcor_sqnorm_kernel(const float* __restrict__ x, int dx,
                                                              const uint16_t* __restrict__ z, int dz,
                                                              float* __restrict__ s_x, float* __restrict__ s_z) {
    __shared__ double red[2][4];
    const size_t row = blockIdx.x;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * (size_t)dx);
    const u32x4* zr = reinterpret_cast<const u32x4*>(z + row * (size_t)dz);
    double ax = 0.0, az = 0.0;
    for (int i = threadIdx.x; i < dx / 4; i += THREADS) {
        const f32x4 v = xr[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) ax += (double)v[k] * (double)v[k];
    }
    for (int i = threadIdx.x; i < dz / 8; i += THREADS) {
        const u32x4 v = zr[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double lo = (double)__uint_as_float(v[k] << 16), hi = (double)__uint_as_float(v[k] & 0xFFFF0000u);
            az += lo * lo;
            az += hi * hi;
        }
    }
    ax = wave_sum_f64(ax);
    az = wave_sum_f64(az);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = ax;
        red[1][threadIdx.x >> 6] = az;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double t = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
        (threadIdx.x ? s_z : s_x)[row] = (float)t;
    }
}

// ------------------------------------------------------------------------------------------------ 2. pair tiles
struct Pieces {
    u32x4 v[2 * PIECES];   // [side][piece]
};

// One K loop: tot = rows(I) . rows(J)^T over `nchunk` chunks of 128 bytes per row. pa / pb are this thread's four
// source rows per side (already offset to its 16-byte column), `lds` the two staging buffers. The MFMAs accumulate
// FLUSH chunks in a chain, then the chain is added to tot and restarts from 0: a float32 chain of all-positive
// products (a post-ReLU cut) loses accuracy with its length, and 16,384 in one chain measured 6 x 2^-24 on a
// squared distance.
constexpr int FLUSH = 16;
template <bool BF16>
__device__ __forceinline__ void gram_loop(f32x16 (&tot)[2][2], const char* (&pa)[PIECES],
                                          const char* (&pb)[PIECES], int nchunk, bool diag, unsigned char* lds,
                                          int st_off, int a_off, int b_off) {
    Pieces p;
    auto gload = [&](int c) {
#pragma unroll
        for (int q = 0; q < PIECES; ++q) p.v[q] = *reinterpret_cast<const u32x4*>(pa[q] + (size_t)c * CHUNK_B);
        if (!diag) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q)
                p.v[PIECES + q] = *reinterpret_cast<const u32x4*>(pb[q] + (size_t)c * CHUNK_B);
        }
    };
    auto lstore = [&](int buf) {
        unsigned char* d = lds + buf * STAGE_B + st_off;
#pragma unroll
        for (int q = 0; q < PIECES; ++q) *reinterpret_cast<u32x4*>(d + q * 32 * ROW_B) = p.v[q];
        if (!diag) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) *reinterpret_cast<u32x4*>(d + SIDE_B + q * 32 * ROW_B) = p.v[PIECES + q];
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = tot[bi][bj][r] = 0.f;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        if (more) gload(c + 1);
        const unsigned char* sa = lds + (c & 1) * STAGE_B + a_off;
        const unsigned char* sb = lds + (c & 1) * STAGE_B + b_off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u32x4 av[2], bv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                av[h] = *reinterpret_cast<const u32x4*>(sa + h * 32 * ROW_B + s * 32);
                bv[h] = *reinterpret_cast<const u32x4*>(sb + h * 32 * ROW_B + s * 32);
            }
            if (BF16) {
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj)
                        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, av[bi]), __builtin_bit_cast(bf16x8, bv[bj]), acc[bi][bj], 0, 0, 0);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                        for (int bj = 0; bj < 2; ++bj)
                            acc[bi][bj] = mfma32x32x2(__uint_as_float(av[bi][t]), __uint_as_float(bv[bj][t]), acc[bi][bj]);
            }
        }
        if ((c & (FLUSH - 1)) == FLUSH - 1 || !more) {
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                    tot[bi][bj] += acc[bi][bj];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;
                }
        }
        if (more) lstore((c + 1) & 1);
        __syncthreads();
    }
}

// Gram accumulators -> distances, in place: d2 = (s_i + s_j) - 2 g, 0 where d2 <= tau (s_i + s_j) (a compare: a NaN
// stays), sqrt; exactly 0 on the diagonal and for a row or column at or past n (selects, so what the clamped loads
// brought in never reaches a sum).
__device__ __forceinline__ void to_distance(f32x16 (&acc)[2][2], const float* si, const float* sj, float tau, int i0,
                                            int j0, int n) {
    const int lane = threadIdx.x & 63, c = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const int lj = bj * 32 + c;
            const float s_j = sj[lj];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int li = bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const float sum = si[li] + s_j;
                float d2 = sum - 2.f * acc[bi][bj][r];
                d2 = d2 <= tau * sum ? 0.f : d2;
                const float d = sqrtf(d2);
                const int i = i0 + li, j = j0 + lj;
                acc[bi][bj][r] = (i == j || i >= n || j >= n) ? 0.f : d;
            }
        }
}

__global__ __launch_bounds__(THREADS) void dcor_tile_kernel(const float* __restrict__ x, int dx,
                                                            const uint16_t* __restrict__ z, int dz, int n, int T,
                                                            const float* __restrict__ s_x,
                                                            const float* __restrict__ s_z, double* __restrict__ rpa,
                                                            double* __restrict__ rpb, double* __restrict__ tri) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE_B];
    __shared__ float ssm[4][TILE];   // s_x of the tile's rows, of its columns, then s_z of both
    // tile blockIdx.x of the upper triangle, rows first: (0,0) (0,1) .. (0,T-1) (1,1) ..
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) {
        rem -= T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    const int I0 = ti * TILE, J0 = tj * TILE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1;
    {
        const int r = (tid < TILE ? I0 : J0 - TILE) + tid;
        ssm[tid >> 7][tid & (TILE - 1)] = r < n ? s_x[r] : 0.f;
        ssm[2 + (tid >> 7)][tid & (TILE - 1)] = r < n ? s_z[r] : 0.f;
    }
    // staging: thread -> 16-byte column tid & 7 of rows (tid >> 3) + 32 q
    const int st_off = (tid >> 3) * ROW_B + (tid & 7) * 16;
    // fragments: lane -> row lane & 31 of its 32-row block, bytes 16 (lane >> 5) of every 32-byte step
    const int frag = (lane & 31) * ROW_B + (lane >> 5) * 16;
    const int a_off = wr * 64 * ROW_B + frag;
    const int b_off = (diag ? 0 : SIDE_B) + wc * 64 * ROW_B + frag;
    size_t ra[PIECES], rb[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        ra[q] = (size_t)min(I0 + (tid >> 3) + 32 * q, n - 1);
        rb[q] = (size_t)min(J0 + (tid >> 3) + 32 * q, n - 1);
    }
    f32x16 a[2][2], b[2][2];
    {
        const char* base = reinterpret_cast<const char*>(x) + (tid & 7) * 16;
        const char* pa[PIECES] = {base + ra[0] * dx * 4, base + ra[1] * dx * 4, base + ra[2] * dx * 4,
                                  base + ra[3] * dx * 4};
        const char* pb[PIECES] = {base + rb[0] * dx * 4, base + rb[1] * dx * 4, base + rb[2] * dx * 4,
                                  base + rb[3] * dx * 4};
        gram_loop<false>(a, pa, pb, dx / 32, diag, lds, st_off, a_off, b_off);
    }
    to_distance(a, ssm[0] + wr * 64, ssm[1] + wc * 64, TAU_X, I0 + wr * 64, J0 + wc * 64, n);
    {
        const char* base = reinterpret_cast<const char*>(z) + (tid & 7) * 16;
        const char* pa[PIECES] = {base + ra[0] * dz * 2, base + ra[1] * dz * 2, base + ra[2] * dz * 2,
                                  base + ra[3] * dz * 2};
        const char* pb[PIECES] = {base + rb[0] * dz * 2, base + rb[1] * dz * 2, base + rb[2] * dz * 2,
                                  base + rb[3] * dz * 2};
        gram_loop<true>(b, pa, pb, dz / 64, diag, lds, st_off, a_off, b_off);
    }
    to_distance(b, ssm[2] + wr * 64, ssm[3] + wc * 64, TAU_Z, I0 + wr * 64, J0 + wc * 64, n);

    // ---- epilogue. The staging buffers are free (the loop's last barrier is behind every wave): they now hold
    // rs[k][wc][row], cs[k][wr][col] (k = 0: a, 1: b) and t3[wave][3].
    double* rs = reinterpret_cast<double*>(lds);
    double* cs = rs + 2 * 2 * TILE;
    double* t3 = cs + 2 * 2 * TILE;
    const int c = lane & 31, hi = lane >> 5;
    double sab = 0.0, saa = 0.0, sbb = 0.0;
    double ca[2] = {0.0, 0.0}, cb[2] = {0.0, 0.0};
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double a0 = a[bi][0][r], a1 = a[bi][1][r], b0 = b[bi][0][r], b1 = b[bi][1][r];
            sab += a0 * b0;
            sab += a1 * b1;
            saa += a0 * a0;
            saa += a1 * a1;
            sbb += b0 * b0;
            sbb += b1 * b1;
            ca[0] += a0;
            ca[1] += a1;
            cb[0] += b0;
            cb[1] += b1;
            double pa = a0 + a1, pb = b0 + b1;   // this row over the lane's two columns, then over the 32 lanes
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) {
                pa += __shfl_xor(pa, o, 64);
                pb += __shfl_xor(pb, o, 64);
            }
            if (c == 0) {
                const int li = wr * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                rs[(0 * 2 + wc) * TILE + li] = pa;
                rs[(1 * 2 + wc) * TILE + li] = pb;
            }
        }
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        ca[bj] += __shfl_xor(ca[bj], 32, 64);
        cb[bj] += __shfl_xor(cb[bj], 32, 64);
        if (hi == 0) {
            cs[(0 * 2 + wr) * TILE + wc * 64 + bj * 32 + c] = ca[bj];
            cs[(1 * 2 + wr) * TILE + wc * 64 + bj * 32 + c] = cb[bj];
        }
    }
    sab = wave_sum_f64(sab);
    saa = wave_sum_f64(saa);
    sbb = wave_sum_f64(sbb);
    if (lane == 0) {
        t3[wave * 3 + 0] = sab;
        t3[wave * 3 + 1] = saa;
        t3[wave * 3 + 2] = sbb;
    }
    __syncthreads();
    const size_t Np = (size_t)T * TILE;
    if (tid < TILE) {
        rpa[(size_t)tj * Np + I0 + tid] = rs[0 * TILE + tid] + rs[1 * TILE + tid];
        rpb[(size_t)tj * Np + I0 + tid] = rs[2 * TILE + tid] + rs[3 * TILE + tid];
    } else if (!diag) {
        const int col = tid - TILE;
        rpa[(size_t)ti * Np + J0 + col] = cs[0 * TILE + col] + cs[1 * TILE + col];
        rpb[(size_t)ti * Np + J0 + col] = cs[2 * TILE + col] + cs[3 * TILE + col];
    }
    if (tid < 3) {
        const double t = (t3[tid] + t3[3 + tid]) + (t3[6 + tid] + t3[9 + tid]);
        tri[(size_t)blockIdx.x * 3 + tid] = diag ? t : 2.0 * t;
    }
}

// ------------------------------------------------------------------------------------------------ 3. finish
constexpr int NACC = 9;   // Ta, Tb, sum ra rb, sum ra^2, sum rb^2, sum (s_x + s_z), Sab, Saa, Sbb

__global__ __launch_bounds__(THREADS) void dcor_finish_kernel(const double* __restrict__ rpa,
                                                              const double* __restrict__ rpb,
                                                              const double* __restrict__ tri,
                                                              const float* __restrict__ s_x,
                                                              const float* __restrict__ s_z, int n, int T, int ntiles,
                                                              float* __restrict__ out4) {
    __shared__ double red[NACC][THREADS];
    const size_t Np = (size_t)T * TILE;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        double ra = 0.0, rb = 0.0;
        for (int t = 0; t < T; ++t) {
            ra += rpa[(size_t)t * Np + i];
            rb += rpb[(size_t)t * Np + i];
        }
        acc[0] += ra;
        acc[1] += rb;
        acc[2] += ra * rb;
        acc[3] += ra * ra;
        acc[4] += rb * rb;
        acc[5] += (double)s_x[i] + (double)s_z[i];
    }
    for (int k = threadIdx.x; k < ntiles; k += THREADS) {
        acc[6] += tri[(size_t)k * 3 + 0];
        acc[7] += tri[(size_t)k * 3 + 1];
        acc[8] += tri[(size_t)k * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double N = (double)n, N2 = N * N, N3 = N2 * N, N4 = N2 * N2;
        const double Ta = red[0][0], Tb = red[1][0];
        const double dcov2 = red[6][0] / N2 - 2.0 * red[2][0] / N3 + Ta * Tb / N4;
        const double dvx = red[7][0] / N2 - 2.0 * red[3][0] / N3 + Ta * Ta / N4;
        const double dvz = red[8][0] / N2 - 2.0 * red[4][0] / N3 + Tb * Tb / N4;
        const double prod = dvx * dvz;
        const double num = dcov2 < 0.0 ? 0.0 : dcov2;
        const double dcor = prod <= 0.0 ? 0.0 : sqrt(num / sqrt(prod));
        // 0 for finite inputs, NaN as soon as any element of x or z is NaN or +-inf (its row's square norm is then
        // NaN or inf): all four outputs, also the variance of the operand that was finite
        const double poison = 0.0 * red[5][0];
        out4[0] = (float)(dcor + poison);
        out4[1] = (float)(dcov2 + poison);
        out4[2] = (float)(dvx + poison);
        out4[3] = (float)(dvz + poison);
    }
}

__global__ void dcor_zero_kernel(float* __restrict__ out4) {
    if (threadIdx.x < 4) out4[threadIdx.x] = 0.f;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
}  // namespace

extern "C" int slk_dcor_tau(int which) { return which == 0 ? TAU_X_ULPS : which == 1 ? TAU_Z_ULPS : -1; }

extern "C" int64_t slk_dcor_workspace_bytes(int n) { return n < 0 ? -1 : layout(n).bytes; }

extern "C" int slk_dcor(const float* x, int dx, const void* z_bf16, int dz, int n, void* workspace, float* out4,
                        void* stream) {
    SLK_CHECK_ARG(n >= 0 && dx >= 0 && dz >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x && z_bf16 && workspace && out4);
    SLK_CHECK_ARG(aligned(x, 16) && aligned(z_bf16, 16) && aligned(workspace, 16) && aligned(out4, 16));
    hipStream_t st = slk_stream(stream);
    if (n == 1) {   // one sample has no pairs: nothing is read
        dcor_zero_kernel<<<1, 64, 0, st>>>(out4);
        return slk_launch_status();
    }
    SLK_CHECK_ARG(dx > 0 && dz > 0 && dx % 64 == 0 && dz % 64 == 0);
    const Layout L = layout(n);
    SLK_CHECK_ARG(L.ntiles <= 0x7FFFFFFF);
    char* ws = static_cast<char*>(workspace);
    double* rpa = reinterpret_cast<double*>(ws + L.off_rpa);
    double* rpb = reinterpret_cast<double*>(ws + L.off_rpb);
    double* tri = reinterpret_cast<double*>(ws + L.off_tri);
    float* s_x = reinterpret_cast<float*>(ws + L.off_sx);
    float* s_z = reinterpret_cast<float*>(ws + L.off_sz);
    const uint16_t* z = static_cast<const uint16_t*>(z_bf16);
    dcor_sqnorm_kernel<<<(unsigned)n, THREADS, 0, st>>>(x, dx, z, dz, s_x, s_z);
    dcor_tile_kernel<<<(unsigned)L.ntiles, THREADS, 0, st>>>(x, dx, z, dz, n, (int)L.T, s_x, s_z, rpa, rpb, tri);
    dcor_finish_kernel<<<1, THREADS, 0, st>>>(rpa, rpb, tri, s_x, s_z, n, (int)L.T, (int)L.ntiles, out4);
    return slk_launch_status();
}
