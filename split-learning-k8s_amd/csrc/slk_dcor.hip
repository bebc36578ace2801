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
constexpr int TILE_VEC = TILE * TILE / 4;                 // f32x4 of one stored tile

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

// slk_dcor_grad's workspace: the metric's layout first (rpa at offset 0), then what the gradient adds. A function of T
// alone, shared by the host and dcor_tile_kernel<true>.
struct GradOffsets {
    int64_t off_rpu, off_coef, off_f, off_ta, off_tb, off_u, bytes;
};
__host__ __device__ inline GradOffsets grad_offsets(int64_t T) {
    const int64_t Np = T * TILE, ntiles = T * (T + 1) / 2;
    GradOffsets G;
    G.off_rpu = 8 * T * Np * 2 + 8 * 3 * ntiles + 8 * Np;   // = layout(n).bytes, padded to 16
    G.off_rpu = (G.off_rpu + 15) & ~(int64_t)15;
    G.off_coef = G.off_rpu + 8 * T * Np;                      // ra/n [Np], rb/n [Np], Ta/n^2, Tb/n^2, C/Vz, f
    G.off_f = G.off_coef + 8 * (2 * Np + 4);                  // f as float32 (16 bytes kept)
    G.off_ta = G.off_f + 16;                                  // float32 a tiles [ntiles][128 x 128]
    G.off_tb = G.off_ta + 4 * ntiles * TILE * TILE;
    G.off_u = G.off_tb + 4 * ntiles * TILE * TILE;            // bf16 U [Np][Np]
    G.bytes = G.off_u + 2 * Np * Np;
    return G;
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

// STORE: the tile's a and b also go to the workspace as float32 (grad_offsets), 64 values per thread in the register
// order below ([blockIdx.x][bi][bj][r >> 2][tid] as f32x4): only dcor_weight_kernel reads them back, lane for lane.
// The two stores are found from rpa (the workspace's base) and T, so both instantiations take the same arguments.
template <bool STORE>
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
    if constexpr (STORE) {
        const GradOffsets G = grad_offsets(T);
        f32x4* qa = reinterpret_cast<f32x4*>(reinterpret_cast<char*>(rpa) + G.off_ta) + (size_t)blockIdx.x * TILE_VEC + tid;
        f32x4* qb = reinterpret_cast<f32x4*>(reinterpret_cast<char*>(rpa) + G.off_tb) + (size_t)blockIdx.x * TILE_VEC + tid;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = ((bi * 2 + bj) * 4 + q) * THREADS;
                    qa[e] = f32x4{a[bi][bj][4 * q], a[bi][bj][4 * q + 1], a[bi][bj][4 * q + 2], a[bi][bj][4 * q + 3]};
                    qb[e] = f32x4{b[bi][bj][4 * q], b[bi][bj][4 * q + 1], b[bi][bj][4 * q + 2], b[bi][bj][4 * q + 3]};
                }
    }

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

// ================================================================================================ gradient
// slk_dcor_grad (include/slk.h, "Distance correlation gradient"): out = dcut + alpha d dCor^2 / d z, from six launches.
//   1-3. the metric's three, the tile kernel as dcor_tile_kernel<true>: the same distances bit for bit, also stored.
//   4. dcor_coef_kernel: one block re-sums rpa / rpb / tri in dcor_finish_kernel's order and stores ra_i / n,
//      rb_i / n, Ta / n^2, Tb / n^2, C / Vz and the scalar factor f (float64; f also rounded once to float32).
//   5. dcor_weight_kernel: one block per stored tile with the tile kernel's thread mapping: u_ij in float64 from the
//      float32 distances, rounded once to bf16 into an LDS tile, from which the block writes the tile and — off the
//      diagonal — its transpose into the row-major U[Np][Np] with 16-byte stores, and the float64 row (and column)
//      sums of the ROUNDED values into rpu[tile column][row], one writer per slot like rpa.
//   6. dcor_product_kernel: acc = U Z on v_mfma_f32_32x32x16_bf16 and the epilogue in registers. A workgroup of four
//      waves (2 x 2) owns 128 rows x 256 features, a wave 64 x 128 as 2 x 4 accumulators of 32 x 32 (128 registers).
//      K runs over j in chunks of 64: the U chunk (128 rows x 128 bytes) stages exactly like a Gram chunk (rows padded
//      to 144 bytes, the same fragment reads); the Z chunk is staged as stored, 64 rows of 512 bytes padded to 576
//      (the four rows a 16-lane group of a transpose read touches then sit 64 bytes apart modulo 256), and its
//      fragments come from ds_read_b64_tr_b16: a lane of a 16-lane group points at 4 features of row k0 + (l >> 2)
//      and receives feature n0 + l of rows k0 .. k0 + 3. No transposed copy of the cut exists. Both operands are
//      double-buffered through registers and two LDS stages, one barrier per chunk. The accumulation is one float32
//      chain over all of K, j ascending.
constexpr int PK = 64;                          // j per chunk
constexpr int PF = 256;                         // features per workgroup
constexpr int ZROW_B = PF * 2 + 64;             // padded LDS row of the Z chunk
constexpr int PA_B = TILE * ROW_B;              // the U chunk
constexpr int PSTAGE_B = PA_B + PK * ZROW_B;    // one stage: 18,432 + 36,864 bytes
constexpr int ZPIECES = PK * (PF * 2 / 16) / THREADS;   // 16-byte pieces of Z per thread: 8
constexpr int UT_ROW = TILE + 2;                // LDS row of the bf16 weight tile: 65 words, column walks hit 32 banks

// round-to-nearest-even of a float64 to bf16 in ONE rounding: the float32 on the way is nudged off a bf16 tie that
// only the first rounding made.
__device__ __forceinline__ uint16_t bf16_from_f64(double u) {
    const float f = (float)u;
    if (f != f) return 0x7FC0;
    uint32_t w = __float_as_uint(f);
    if ((w & 0xFFFFu) == 0x8000u && (double)f != u) w += fabs((double)f) < fabs(u) ? 1u : 0xFFFFFFFFu;
    return (uint16_t)((w + 0x7FFFu + ((w >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ uint16_t bf16_from_f32(float f) {
    const uint32_t w = __float_as_uint(f);
    return f != f ? (uint16_t)0x7FC0 : (uint16_t)((w + 0x7FFFu + ((w >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// ------------------------------------------------------------------------------------------------ 4. coefficients
__global__ __launch_bounds__(THREADS) void dcor_coef_kernel(const double* __restrict__ rpa,
                                                            const double* __restrict__ rpb,
                                                            const double* __restrict__ tri,
                                                            const float* __restrict__ s_x,
                                                            const float* __restrict__ s_z, int n, int T, int ntiles,
                                                            const float* __restrict__ alpha, int squared,
                                                            double* __restrict__ coef, float* __restrict__ fout) {
    __shared__ double red[NACC][THREADS];
    const size_t Np = (size_t)T * TILE;
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < (int)Np; i += THREADS) {   // dcor_finish_kernel's sums; rows at or past n hold 0
        double ra = 0.0, rb = 0.0;
        if (i < n) {
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
        coef[i] = ra / (double)n;
        coef[Np + i] = rb / (double)n;
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
        const bool clamped = prod <= 0.0 || dcov2 <= 0.0;   // where the closed form clamps: no gradient (NaN: neither)
        const double root = sqrt(prod);
        double f = (double)alpha[0] * 2.0 / (N2 * root);
        if (!squared) f /= 2.0 * sqrt(dcov2 / root);
        f = (clamped ? 0.0 : f) + 0.0 * red[5][0];          // the metric's poison term: NaN for a non-finite input
        coef[2 * Np + 0] = Ta / N2;
        coef[2 * Np + 1] = Tb / N2;
        coef[2 * Np + 2] = clamped ? 0.0 : dcov2 / dvz;
        coef[2 * Np + 3] = f;
        fout[0] = (float)f;
    }
}

// ------------------------------------------------------------------------------------------------ 5. weights
__global__ __launch_bounds__(THREADS) void dcor_weight_kernel(const float* __restrict__ sa,
                                                              const float* __restrict__ sb,
                                                              const double* __restrict__ coef, int T,
                                                              uint16_t* __restrict__ U, double* __restrict__ rpu) {
    __shared__ uint16_t ut[TILE * UT_ROW];
    __shared__ double cr[4][TILE];   // ra / n of the tile's rows, of its columns, then rb / n of both
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) {
        rem -= T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    const int I0 = ti * TILE, J0 = tj * TILE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1;
    const size_t Np = (size_t)T * TILE;
    {
        const int r = (tid < TILE ? I0 : J0 - TILE) + tid;
        cr[tid >> 7][tid & (TILE - 1)] = coef[r];
        cr[2 + (tid >> 7)][tid & (TILE - 1)] = coef[Np + r];
    }
    const double tan2 = coef[2 * Np], tbn2 = coef[2 * Np + 1], cvz = coef[2 * Np + 2];
    __syncthreads();
    const f32x4* qa = reinterpret_cast<const f32x4*>(sa) + (size_t)blockIdx.x * TILE_VEC + tid;
    const f32x4* qb = reinterpret_cast<const f32x4*>(sb) + (size_t)blockIdx.x * TILE_VEC + tid;
    const int c = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const int lj = wc * 64 + bj * 32 + c;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 av = qa[((bi * 2 + bj) * 4 + q) * THREADS], bv = qb[((bi * 2 + bj) * 4 + q) * THREADS];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int li = wr * 64 + bi * 32 + k + 8 * q + 4 * hi;   // r = 4 q + k
                    const double a = av[k], b = bv[k];
                    const double abar = ((a - cr[0][li]) - cr[1][lj]) + tan2;
                    const double bbar = ((b - cr[2][li]) - cr[3][lj]) + tbn2;
                    const double u = (abar - cvz * bbar) / b;
                    ut[li * UT_ROW + lj] = b > 0.0 ? bf16_from_f64(u) : (uint16_t)0;
                }
            }
        }
    __syncthreads();
    for (int e = tid; e < TILE * (TILE / 8); e += THREADS) {
        const int row = e >> 4, pc = e & 15;
        uint32_t w[4], wt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = (uint32_t)ut[row * UT_ROW + pc * 8 + 2 * k] | (uint32_t)ut[row * UT_ROW + pc * 8 + 2 * k + 1] << 16;
            wt[k] = (uint32_t)ut[(pc * 8 + 2 * k) * UT_ROW + row] | (uint32_t)ut[(pc * 8 + 2 * k + 1) * UT_ROW + row] << 16;
        }
        *reinterpret_cast<u32x4*>(U + (size_t)(I0 + row) * Np + J0 + pc * 8) = u32x4{w[0], w[1], w[2], w[3]};
        if (!diag) *reinterpret_cast<u32x4*>(U + (size_t)(J0 + row) * Np + I0 + pc * 8) = u32x4{wt[0], wt[1], wt[2], wt[3]};
    }
    // the sums of the rounded weights: row tid over the tile's columns ascending, column tid - 128 over its rows
    if (tid < TILE) {
        double s = 0.0;
        for (int k = 0; k < TILE; ++k) s += (double)bf16_to_f32(ut[tid * UT_ROW + k]);
        rpu[(size_t)tj * Np + I0 + tid] = s;
    } else if (!diag) {
        double s = 0.0;
        for (int k = 0; k < TILE; ++k) s += (double)bf16_to_f32(ut[k * UT_ROW + tid - TILE]);
        rpu[(size_t)ti * Np + J0 + tid - TILE] = s;
    }
}

// ------------------------------------------------------------------------------------------------ 6. product
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(THREADS) void dcor_product_kernel(const uint16_t* __restrict__ U,
                                                               const uint16_t* __restrict__ z, int dz, int n, int T,
                                                               const double* __restrict__ rpu,
                                                               const float* __restrict__ fp,
                                                               const uint16_t* dcut, uint16_t* out) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * PSTAGE_B];
    __shared__ float rus[TILE];
    typedef __attribute__((address_space(3))) bf16x4* lp4;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1;
    const int I0 = blockIdx.x * TILE, F0 = blockIdx.y * PF;
    const size_t Np = (size_t)T * TILE;
    const float f = fp[0];
    const int nchunk = f == 0.f ? 0 : 2 * T;   // f == 0: out = dcut, U is not read

    // staging. U: thread -> 16-byte column tid & 7 of rows (tid >> 3) + 32 q. Z: 16-byte column tid & 31 (8 features)
    // of chunk rows (tid >> 5) + 8 q; columns at or past dz stage zeros, rows at or past n read row n - 1.
    const char* pu = reinterpret_cast<const char*>(U + (size_t)(I0 + (tid >> 3)) * Np) + (tid & 7) * 16;
    const bool zcol = F0 + (tid & 31) * 8 < dz;
    const char* pz = reinterpret_cast<const char*>(z + F0 + (zcol ? (tid & 31) * 8 : 0));
    const int ust = (tid >> 3) * ROW_B + (tid & 7) * 16;
    const int zst = PA_B + (tid >> 5) * ZROW_B + (tid & 31) * 16;
    u32x4 ru[PIECES], rz[ZPIECES];
    auto gload = [&](int c) {
#pragma unroll
        for (int q = 0; q < PIECES; ++q)
            ru[q] = *reinterpret_cast<const u32x4*>(pu + (size_t)q * 32 * Np * 2 + (size_t)c * CHUNK_B);
#pragma unroll
        for (int q = 0; q < ZPIECES; ++q) {
            const size_t j = (size_t)min(c * PK + (tid >> 5) + 8 * q, n - 1);
            rz[q] = zcol ? *reinterpret_cast<const u32x4*>(pz + j * dz * 2) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto lstore = [&](int buf) {
        unsigned char* d = lds + buf * PSTAGE_B;
#pragma unroll
        for (int q = 0; q < PIECES; ++q) *reinterpret_cast<u32x4*>(d + ust + q * 32 * ROW_B) = ru[q];
#pragma unroll
        for (int q = 0; q < ZPIECES; ++q) *reinterpret_cast<u32x4*>(d + zst + q * 8 * ZROW_B) = rz[q];
    };
    // fragments. U as in gram_loop. Z by transpose reads: lane l of a 16-lane group g points at features 4 (l & 3) ..
    // of chunk row k0 + (l >> 2) and receives feature 16 (g & 1) + l of rows k0 .. k0 + 3, k0 = 8 (g >> 1) (+ 4).
    const int a_off = (wr * 64 + (lane & 31)) * ROW_B + (lane >> 5) * 16;
    const int b_off = PA_B + (8 * (lane >> 5) + ((lane & 15) >> 2)) * ZROW_B +
                      (wc * 128 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    f32x16 acc[2][4];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;
    if (nchunk > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        if (more) gload(c + 1);
        const unsigned char* sa = lds + (c & 1) * PSTAGE_B + a_off;
        const unsigned char* sb = lds + (c & 1) * PSTAGE_B + b_off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bf16x8 av[2], bv[4];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
                av[bi] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(sa + bi * 32 * ROW_B + s * 32));
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                const unsigned char* pb = sb + s * 16 * ZROW_B + bj * 64;
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp4)pb);
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp4)(pb + 4 * ZROW_B));
                bv[bj] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 4; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[bi], bv[bj], acc[bi][bj], 0, 0, 0);
        }
        if (more) lstore((c + 1) & 1);
        __syncthreads();
    }
    // ---- epilogue: ru_i = the row's parts over the tile columns ascending (float64, rounded once to float32), then
    // out = bf16(fmaf(f, fmaf(ru_i, z, -acc), dcut)); dcut's own bits where f == 0.
    if (tid < TILE) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += rpu[(size_t)t * Np + I0 + tid];
        rus[tid] = (float)s;
    }
    __syncthreads();
    const int c = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int li = wr * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const int i = I0 + li;
            const float rui = rus[li];
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) {
                const int k = F0 + wc * 128 + bj * 32 + c;
                if (i < n && k < dz) {
                    const size_t e = (size_t)i * dz + k;
                    const uint16_t d = dcut[e];
                    const float t = __builtin_fmaf(rui, bf16_to_f32(z[e]), -acc[bi][bj][r]);
                    out[e] = f == 0.f ? d : bf16_from_f32(__builtin_fmaf(f, t, bf16_to_f32(d)));
                }
            }
        }
}

__global__ void dcor_copy_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int count) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) dst[i] = src[i];
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
    dcor_tile_kernel<false><<<(unsigned)L.ntiles, THREADS, 0, st>>>(x, dx, z, dz, n, (int)L.T, s_x, s_z, rpa, rpb, tri);
    dcor_finish_kernel<<<1, THREADS, 0, st>>>(rpa, rpb, tri, s_x, s_z, n, (int)L.T, (int)L.ntiles, out4);
    return slk_launch_status();
}

extern "C" int64_t slk_dcor_grad_workspace_bytes(int n) {
    return n < 0 ? -1 : grad_offsets((n + TILE - 1) / TILE).bytes;
}

extern "C" int slk_dcor_grad(const float* x, int dx, const void* z_bf16, int dz, int n, const void* dcut_bf16,
                             const float* alpha, int squared, void* workspace, void* out_bf16, float* out4,
                             void* stream) {
    SLK_CHECK_ARG(n >= 0 && dx >= 0 && dz >= 0 && (squared == 0 || squared == 1));
    if (n == 0) return 0;
    SLK_CHECK_ARG(x && z_bf16 && dcut_bf16 && alpha && workspace && out_bf16 && out4);
    SLK_CHECK_ARG(aligned(x, 16) && aligned(z_bf16, 16) && aligned(dcut_bf16, 16) && aligned(alpha, 4) &&
                  aligned(workspace, 16) && aligned(out_bf16, 16) && aligned(out4, 16));
    hipStream_t st = slk_stream(stream);
    const uint16_t* z = static_cast<const uint16_t*>(z_bf16);
    const uint16_t* dcut = static_cast<const uint16_t*>(dcut_bf16);
    uint16_t* out = static_cast<uint16_t*>(out_bf16);
    if (n == 1) {   // one sample has no pairs: the gradient term is 0
        if (out != dcut && dz > 0) dcor_copy_kernel<<<(dz + 255) / 256, 256, 0, st>>>(dcut, out, dz);
        dcor_zero_kernel<<<1, 64, 0, st>>>(out4);
        return slk_launch_status();
    }
    SLK_CHECK_ARG(dx > 0 && dz > 0 && dx % 64 == 0 && dz % 64 == 0);
    const Layout L = layout(n);
    SLK_CHECK_ARG(L.T <= 0xFFFF);   // the product's grid; also keeps every tile count inside an int
    const GradOffsets G = grad_offsets(L.T);
    char* ws = static_cast<char*>(workspace);
    double* rpa = reinterpret_cast<double*>(ws + L.off_rpa);
    double* rpb = reinterpret_cast<double*>(ws + L.off_rpb);
    double* tri = reinterpret_cast<double*>(ws + L.off_tri);
    float* s_x = reinterpret_cast<float*>(ws + L.off_sx);
    float* s_z = reinterpret_cast<float*>(ws + L.off_sz);
    double* rpu = reinterpret_cast<double*>(ws + G.off_rpu);
    double* coef = reinterpret_cast<double*>(ws + G.off_coef);
    float* fslot = reinterpret_cast<float*>(ws + G.off_f);
    const float* ta = reinterpret_cast<const float*>(ws + G.off_ta);
    const float* tb = reinterpret_cast<const float*>(ws + G.off_tb);
    uint16_t* U = reinterpret_cast<uint16_t*>(ws + G.off_u);
    dcor_sqnorm_kernel<<<(unsigned)n, THREADS, 0, st>>>(x, dx, z, dz, s_x, s_z);
    dcor_tile_kernel<true><<<(unsigned)L.ntiles, THREADS, 0, st>>>(x, dx, z, dz, n, (int)L.T, s_x, s_z, rpa, rpb, tri);
    dcor_finish_kernel<<<1, THREADS, 0, st>>>(rpa, rpb, tri, s_x, s_z, n, (int)L.T, (int)L.ntiles, out4);
    dcor_coef_kernel<<<1, THREADS, 0, st>>>(rpa, rpb, tri, s_x, s_z, n, (int)L.T, (int)L.ntiles, alpha, squared, coef,
                                            fslot);
    dcor_weight_kernel<<<(unsigned)L.ntiles, THREADS, 0, st>>>(ta, tb, coef, (int)L.T, U, rpu);
    dcor_product_kernel<<<dim3((unsigned)L.T, (unsigned)((dz + PF - 1) / PF)), THREADS, 0, st>>>(
        U, z, dz, n, (int)L.T, rpu, fslot, dcut, out);
    return slk_launch_status();
}
