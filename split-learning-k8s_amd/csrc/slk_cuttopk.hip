// slk_cuttopk.hip — top-k sparsified records of the K5 cut and its gradient (include/slk.h, "Top-k cut records").
//
// One workgroup of 256 threads owns one sample of 16,384 bf16 elements = 2,048 16-byte pieces of 8 elements. Wave w
// owns the 512 contiguous pieces [512 w, 512 w + 512); in round j = 0..7 lane l holds piece 512 w + 64 j + l, so every
// load and store instruction of a wave covers 1 KiB contiguous, and the sample stays in 32 registers to the end. Piece
// p is also byte p of the record's bit map (8 elements = 8 bits), which is why the bit map is built from bytes.
//
// Selection: an exact two-level radix select on the 15-bit key mag = bits & 0x7fff. Pass 1 counts mag >> 7 in 256
// bins, pass 2 counts mag & 127 in 128 bins over the elements of the crossing bin; each wave has its own histogram
// in LDS (integer ds_add: the sum does not depend on the order) and zeros are not counted at all (their number is
// 16,384 minus the rest). A block-wide suffix sum from the top bin finds the crossing bin and what is still needed;
// the result is the threshold T and r = k - #{mag > T}, the number of elements equal to T that are kept. Bin 255 of
// pass 1 is exactly the non-finite elements: a nonzero count poisons the sample.
//
// Ties and compaction: each thread keeps a 64-bit mask of its elements above T and one of those equal to T (byte j =
// round j). The index-order rank of a piece's first element among the marked elements is a wave prefix sum per round
// (two rounds packed into one word), the rounds' totals accumulated in round order, and the waves' totals through
// LDS. An equal element is kept where its rank among the equal ones is below r; a kept element's slot in the record
// is (#above before it) + min(#equal before it, r). Values are compacted into an LDS stage and the bit map bytes into
// another; both leave as 16-byte stores. Every output byte has one writer; no global atomics, no scratch.
#include "slk_common.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SAMPLE = 16384;
constexpr int ROUNDS = 8;                    // pieces per thread
constexpr int PIECES = SAMPLE / 8;           // 2,048 pieces = bit map bytes
constexpr int HEADER = 16;
constexpr int VALUES_OFF = HEADER + PIECES;  // 2,064
constexpr int K_MAX = 8192;
constexpr uint32_t FMT_WORD = 0x20u;
constexpr uint32_t NAN2 = 0x7fc07fc0u;

inline bool k_ok(int k) { return k >= 8 && k <= K_MAX && (k & 7) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline size_t record_bytes(int k) { return (size_t)VALUES_OFF + 2u * (size_t)k; }

struct Sample {
    u32x4 v[ROUNDS];   // round j: piece piece_of(j), element 2i in the low half of word i
};

__device__ __forceinline__ int piece_of(int j) {
    return (int)(threadIdx.x >> 6) * (PIECES / WAVES) + j * 64 + (int)(threadIdx.x & 63u);
}

__device__ __forceinline__ void load_sample(const uint16_t* x, Sample& s) {
    const u32x4* p = reinterpret_cast<const u32x4*>(x);
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) s.v[j] = p[piece_of(j)];
}

__device__ __forceinline__ void store_sample(uint16_t* out, const Sample& s) {
    u32x4* p = reinterpret_cast<u32x4*>(out);
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) p[piece_of(j)] = s.v[j];
}

__device__ __forceinline__ void nan_sample(Sample& s) {
    const u32x4 nan = {NAN2, NAN2, NAN2, NAN2};
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) s.v[j] = nan;
}

// bits of element e (0..7) of a piece
__device__ __forceinline__ uint32_t elem(const u32x4& v, int e) { return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu; }

// Inclusive prefix sum over the 64 lanes of a wave, in lane order.
__device__ __forceinline__ uint32_t wave_iscan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
        v += lane >= o ? u : 0u;
    }
    return v;
}

// Exclusive prefix sum of one value per thread over the block in thread order, and the block's total. One barrier;
// red holds WAVES words that nobody else uses.
__device__ __forceinline__ uint32_t block_escan(uint32_t v, uint32_t* red, uint32_t& total) {
    const uint32_t inc = wave_iscan(v);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) red[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
        const uint32_t t = red[w];
        base += w < wave ? t : 0u;
        total += t;
    }
    return base + inc - v;
}

struct SelectLds {
    uint32_t hist[WAVES][256];
    uint32_t red[2][WAVES];
    int bin;          // pass 1's crossing bin, -1 where the k-th element is a zero
    uint32_t need;    // how many elements of that bin are kept
    uint32_t poison;  // the sample holds a non-finite element
    uint32_t T, r;
};

struct Threshold {
    uint32_t T, r;
    bool poison;
};

// The threshold of the sample in registers: the k-th largest key T and r = k - #{mag > T} >= 1. Block-wide.
__device__ __forceinline__ Threshold select(const Sample& s, uint32_t k, SelectLds& L) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    uint32_t* flat = &L.hist[0][0];
#pragma unroll
    for (int i = 0; i < WAVES; ++i) flat[i * THREADS + tid] = 0u;
    if (tid == 0) L.bin = -1;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t mag = elem(s.v[j], e) & 0x7fffu;
            if (mag != 0u) atomicAdd(&L.hist[wave][mag >> 7], 1u);
        }
    }
    __syncthreads();
    // bin tid over the four waves; S = #{elements in bins >= tid}
    const uint32_t c = L.hist[0][tid] + L.hist[1][tid] + L.hist[2][tid] + L.hist[3][tid];
    uint32_t nonzero;
    const uint32_t excl = block_escan(c, L.red[0], nonzero);
    const uint32_t S = nonzero - excl, Snext = S - c;
    if (S >= k && Snext < k) {
        L.bin = (int)tid;
        L.need = k - Snext;
    }
    if (tid == 255u) L.poison = c != 0u;   // mag >> 7 == 255: mag >= 0x7f80
    // every thread has read its bin (block_escan's barrier): clear for pass 2
#pragma unroll
    for (int i = 0; i < WAVES; ++i) flat[i * THREADS + tid] = 0u;
    __syncthreads();
    Threshold t;
    t.poison = L.poison != 0u;
    const int bin = L.bin;
    if (t.poison || bin < 0) {   // uniform; fewer than k nonzeros: every nonzero is kept and the first r zeros
        t.T = 0u;
        t.r = k - nonzero;
        return t;
    }
    const uint32_t need = L.need;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t mag = elem(s.v[j], e) & 0x7fffu;
            if (mag != 0u && (int)(mag >> 7) == bin) atomicAdd(&L.hist[wave][mag & 127u], 1u);
        }
    }
    __syncthreads();
    const uint32_t c2 = tid < 128u ? L.hist[0][tid] + L.hist[1][tid] + L.hist[2][tid] + L.hist[3][tid] : 0u;
    uint32_t inbin;
    const uint32_t excl2 = block_escan(c2, L.red[1], inbin);
    const uint32_t S2 = inbin - excl2, S2next = S2 - c2;
    if (tid < 128u && S2 >= need && S2next < need) {
        L.T = ((uint32_t)bin << 7) | tid;
        L.r = need - S2next;
    }
    __syncthreads();
    t.T = L.T;
    t.r = L.r;
    return t;
}

// The thread's elements above T (gt) and equal to T (eq): bit 8 j + e is element e of round j's piece.
__device__ __forceinline__ void masks(const Sample& s, uint32_t T, uint64_t& gt, uint64_t& eq) {
    gt = eq = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        uint32_t g = 0, q = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t mag = elem(s.v[j], e) & 0x7fffu;
            g |= (uint32_t)(mag > T) << e;
            q |= (uint32_t)(mag == T) << e;
        }
        gt |= (uint64_t)g << (8 * j);
        eq |= (uint64_t)q << (8 * j);
    }
}

__device__ __forceinline__ uint32_t byte_of(uint64_t m, int j) { return (uint32_t)(m >> (8 * j)) & 0xffu; }

// rank[j] = how many elements marked in m (by any thread) come before the first element of this thread's round-j
// piece in index order; total = how many are marked in the block. One barrier; wsum holds WAVES words of its own.
__device__ __forceinline__ void piece_ranks(uint64_t m, uint32_t* wsum, uint32_t (&rank)[ROUNDS], uint32_t& total) {
    uint32_t cnt[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) cnt[j] = (uint32_t)__popc(byte_of(m, j));
    uint32_t base = 0;   // the wave's marked elements in the rounds before: a wave's rounds are 512 elements apart
#pragma unroll
    for (int q = 0; q < ROUNDS / 2; ++q) {   // two rounds per scan: a round's wave total is at most 512
        const uint32_t inc = wave_iscan(cnt[2 * q] | (cnt[2 * q + 1] << 16));
        const uint32_t tot = (uint32_t)__shfl((int)inc, 63, 64);
        rank[2 * q] = base + (inc & 0xffffu) - cnt[2 * q];
        base += tot & 0xffffu;
        rank[2 * q + 1] = base + (inc >> 16) - cnt[2 * q + 1];
        base += tot >> 16;
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wsum[wave] = base;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
        const uint32_t t = wsum[w];
        before += w < wave ? t : 0u;
        total += t;
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) rank[j] += before;
}

// The kept elements: everything above T and the first r, in index order, of those equal to it.
__device__ __forceinline__ uint64_t kept_mask(uint64_t gt, uint64_t eq, const uint32_t (&eq_rank)[ROUNDS], uint32_t r) {
    uint64_t kept = gt;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t q = byte_of(eq, j);
        uint32_t keep = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t before = eq_rank[j] + (uint32_t)__popc(q & ((1u << e) - 1u));
            keep |= (((q >> e) & 1u) & (uint32_t)(before < r)) << e;
        }
        kept |= (uint64_t)keep << (8 * j);
    }
    return kept;
}

// kept ? x : +0, in registers.
__device__ __forceinline__ void sparsify(Sample& s, uint64_t kept) {
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t b = byte_of(kept, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t lo = (b >> (2 * i)) & 1u ? 0x0000ffffu : 0u, hi = (b >> (2 * i + 1)) & 1u ? 0xffff0000u : 0u;
            s.v[j][i] &= lo | hi;
        }
    }
}

struct RankLds {
    uint32_t gt[WAVES], eq[WAVES];
};

__global__ __launch_bounds__(THREADS) void cuttopk_encode_kernel(const uint16_t* __restrict__ x, uint32_t k,
                                                                 uint8_t* __restrict__ rec) {
    __shared__ SelectLds L;
    __shared__ RankLds W;
    __shared__ __attribute__((aligned(16))) uint16_t stage[K_MAX];   // the kept values by slot
    __shared__ __attribute__((aligned(16))) uint8_t bitmap[PIECES];
    uint8_t* r = rec + (size_t)blockIdx.x * (VALUES_OFF + 2u * (size_t)k);
    Sample s;
    load_sample(x + (size_t)blockIdx.x * SAMPLE, s);
    const Threshold t = select(s, k, L);
    if (threadIdx.x == 0) {
        const u32x4 head = {k, FMT_WORD, t.poison ? 1u : 0u, 0u};
        *reinterpret_cast<u32x4*>(r) = head;
    }
    u32x4* bm_out = reinterpret_cast<u32x4*>(r + HEADER);
    u32x4* val_out = reinterpret_cast<u32x4*>(r + VALUES_OFF);
    const uint32_t nval = k / 8u;   // 16-byte pieces of values
    if (t.poison) {                 // uniform
        const u32x4 zero = {0u, 0u, 0u, 0u};
        if (threadIdx.x < PIECES / 16) bm_out[threadIdx.x] = zero;
        for (uint32_t i = threadIdx.x; i < nval; i += THREADS) val_out[i] = zero;
        return;
    }
    uint64_t gt, eq;
    masks(s, t.T, gt, eq);
    uint32_t gt_rank[ROUNDS], eq_rank[ROUNDS], ngt, neq;
    piece_ranks(gt, W.gt, gt_rank, ngt);
    piece_ranks(eq, W.eq, eq_rank, neq);
    const uint64_t kept = kept_mask(gt, eq, eq_rank, t.r);
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t g = byte_of(gt, j), q = byte_of(eq, j), b = byte_of(kept, j);
        bitmap[piece_of(j)] = (uint8_t)b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if ((b >> e) & 1u) {
                const uint32_t below = (1u << e) - 1u;
                const uint32_t slot = gt_rank[j] + (uint32_t)__popc(g & below) +
                                      min(eq_rank[j] + (uint32_t)__popc(q & below), t.r);
                stage[slot & (K_MAX - 1)] = (uint16_t)elem(s.v[j], e);   // slot < k: exactly k elements are kept
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < PIECES / 16) bm_out[threadIdx.x] = reinterpret_cast<const u32x4*>(bitmap)[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < nval; i += THREADS) val_out[i] = reinterpret_cast<const u32x4*>(stage)[i];
}

// decode(encode(x)) without the record; x and out are not __restrict__: they may be the same buffer (a thread reads
// all of its pieces before its first store, and no other thread touches them).
__global__ __launch_bounds__(THREADS) void cuttopk_roundtrip_kernel(const uint16_t* x, uint32_t k, uint16_t* out) {
    __shared__ SelectLds L;
    __shared__ RankLds W;
    Sample s;
    load_sample(x + (size_t)blockIdx.x * SAMPLE, s);
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
    const Threshold t = select(s, k, L);
    if (t.poison) {   // uniform
        nan_sample(s);
        store_sample(o, s);
        return;
    }
    uint64_t gt, eq;
    masks(s, t.T, gt, eq);
    uint32_t eq_rank[ROUNDS], neq;
    piece_ranks(eq, W.eq, eq_rank, neq);
    sparsify(s, kept_mask(gt, eq, eq_rank, t.r));
    store_sample(o, s);
}

__global__ __launch_bounds__(THREADS) void cuttopk_decode_kernel(const uint8_t* __restrict__ rec, uint32_t k,
                                                                 uint16_t* __restrict__ out, int* __restrict__ err_flag) {
    __shared__ RankLds W;
    __shared__ __attribute__((aligned(16))) uint16_t stage[K_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t bitmap[PIECES];
    const uint8_t* r = rec + (size_t)blockIdx.x * (VALUES_OFF + 2u * (size_t)k);
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
    const u32x4 head = *reinterpret_cast<const u32x4*>(r);
    const bool bad_head = head[0] != k || head[1] != FMT_WORD || head[2] > 1u || head[3] != 0u;
    Sample s;
    if (bad_head || head[2] == 1u) {   // uniform: malformed, or poisoned (the payload is not looked at)
        if (bad_head && threadIdx.x == 0) err_flag[0] = 1;
        nan_sample(s);
        store_sample(o, s);
        return;
    }
    if (threadIdx.x < PIECES / 16)
        reinterpret_cast<u32x4*>(bitmap)[threadIdx.x] = reinterpret_cast<const u32x4*>(r + HEADER)[threadIdx.x];
    const uint32_t nval = k / 8u;
    for (uint32_t i = threadIdx.x; i < nval; i += THREADS)
        reinterpret_cast<u32x4*>(stage)[i] = reinterpret_cast<const u32x4*>(r + VALUES_OFF)[i];
    __syncthreads();
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) m |= (uint64_t)bitmap[piece_of(j)] << (8 * j);
    uint32_t rank[ROUNDS], total;
    piece_ranks(m, W.gt, rank, total);
    if (total != k) {   // uniform, and before anything is written or gathered
        if (threadIdx.x == 0) err_flag[0] = 1;
        nan_sample(s);
        store_sample(o, s);
        return;
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t b = byte_of(m, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t w = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int e = 2 * i + h;
                if ((b >> e) & 1u) {
                    const uint32_t slot = rank[j] + (uint32_t)__popc(b & ((1u << e) - 1u));   // < total == k
                    w |= (uint32_t)stage[slot & (K_MAX - 1)] << (16 * h);
                }
            }
            s.v[j][i] = w;
        }
    }
    store_sample(o, s);
}

// ---- The masked backward ("Top-k cut records: the masked backward"): the cut gradient travels at the positions the
// forward kept. The selection is given — the forward's bit map, u8 [n, 2048] — so there is no select: a thread's
// share of the map is one byte per round (piece p is map byte p), the ranks are piece_ranks over those bytes, and
// the block-wide popcount that falls out of them is the poison check (a map that does not hold k bits).
constexpr uint32_t MASKED_FMT_WORD = 0x21u;
inline size_t masked_record_bytes(int k) { return (size_t)HEADER + 2u * (size_t)k; }

// The thread's eight map bytes, byte j = round j: a wave's load covers 64 contiguous bytes.
__device__ __forceinline__ uint64_t load_map(const uint8_t* map) {
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) m |= (uint64_t)map[piece_of(j)] << (8 * j);
    return m;
}

// How many bits the block's masks hold. One barrier; red holds WAVES words of its own.
__device__ __forceinline__ uint32_t block_popcount(uint64_t m, uint32_t* red) {
    uint32_t c = (uint32_t)__popcll(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// slk_cuttopk_roundtrip that also leaves its selection: the kept bytes go through a 2 KiB LDS byte map and leave as
// 128 16-byte stores. A kernel of its own, so that cuttopk_roundtrip_kernel's code stays what it is.
__global__ __launch_bounds__(THREADS) void cuttopk_roundtrip_map_kernel(const uint16_t* x, uint32_t k, uint16_t* out,
                                                                        uint8_t* __restrict__ map) {
    __shared__ SelectLds L;
    __shared__ RankLds W;
    __shared__ __attribute__((aligned(16))) uint8_t bitmap[PIECES];
    Sample s;
    load_sample(x + (size_t)blockIdx.x * SAMPLE, s);
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
    u32x4* bm_out = reinterpret_cast<u32x4*>(map + (size_t)blockIdx.x * PIECES);
    const Threshold t = select(s, k, L);
    if (t.poison) {   // uniform
        const u32x4 zero = {0u, 0u, 0u, 0u};
        if (threadIdx.x < PIECES / 16) bm_out[threadIdx.x] = zero;
        nan_sample(s);
        store_sample(o, s);
        return;
    }
    uint64_t gt, eq;
    masks(s, t.T, gt, eq);
    uint32_t eq_rank[ROUNDS], neq;
    piece_ranks(eq, W.eq, eq_rank, neq);
    const uint64_t kept = kept_mask(gt, eq, eq_rank, t.r);
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) bitmap[piece_of(j)] = (uint8_t)byte_of(kept, j);
    sparsify(s, kept);
    store_sample(o, s);
    __syncthreads();
    if (threadIdx.x < PIECES / 16) bm_out[threadIdx.x] = reinterpret_cast<const u32x4*>(bitmap)[threadIdx.x];
}

// out = bit set ? g : +0; g and out are not __restrict__: they may be the same buffer (as in the roundtrip). No value
// leaves its lane: the map byte of a piece is the byte mask of that piece's eight elements.
__global__ __launch_bounds__(THREADS) void cuttopk_mask_kernel(const uint16_t* g, const uint8_t* __restrict__ map,
                                                               uint32_t k, uint16_t* out) {
    __shared__ uint32_t red[WAVES];
    Sample s;
    load_sample(g + (size_t)blockIdx.x * SAMPLE, s);
    const uint64_t m = load_map(map + (size_t)blockIdx.x * PIECES);
    if (block_popcount(m, red) != k)   // uniform, and before anything is written
        nan_sample(s);
    else
        sparsify(s, m);
    store_sample(out + (size_t)blockIdx.x * SAMPLE, s);
}

// The k values under the map's bits, compacted in index order through the LDS stage into a masked record.
__global__ __launch_bounds__(THREADS) void cuttopk_gather_kernel(const uint16_t* __restrict__ g,
                                                                 const uint8_t* __restrict__ map, uint32_t k,
                                                                 uint8_t* __restrict__ rec) {
    __shared__ RankLds W;
    __shared__ __attribute__((aligned(16))) uint16_t stage[K_MAX];
    uint8_t* r = rec + (size_t)blockIdx.x * (HEADER + 2u * (size_t)k);
    Sample s;
    load_sample(g + (size_t)blockIdx.x * SAMPLE, s);
    const uint64_t m = load_map(map + (size_t)blockIdx.x * PIECES);
    uint32_t rank[ROUNDS], total;
    piece_ranks(m, W.gt, rank, total);
    const bool poison = total != k;   // uniform, and before anything is written
    if (threadIdx.x == 0) {
        const u32x4 head = {k, MASKED_FMT_WORD, poison ? 1u : 0u, 0u};
        *reinterpret_cast<u32x4*>(r) = head;
    }
    u32x4* val_out = reinterpret_cast<u32x4*>(r + HEADER);
    const uint32_t nval = k / 8u;
    if (poison) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (uint32_t i = threadIdx.x; i < nval; i += THREADS) val_out[i] = zero;
        return;
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t b = byte_of(m, j);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if ((b >> e) & 1u) {
                const uint32_t slot = rank[j] + (uint32_t)__popc(b & ((1u << e) - 1u));   // < total == k
                stage[slot & (K_MAX - 1)] = (uint16_t)elem(s.v[j], e);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nval; i += THREADS) val_out[i] = reinterpret_cast<const u32x4*>(stage)[i];
}

// A masked record back to a dense row: the values staged in LDS, then every set bit fetches its own by rank.
__global__ __launch_bounds__(THREADS) void cuttopk_scatter_kernel(const uint8_t* __restrict__ rec,
                                                                  const uint8_t* __restrict__ map, uint32_t k,
                                                                  uint16_t* __restrict__ out, int* __restrict__ err_flag) {
    __shared__ RankLds W;
    __shared__ __attribute__((aligned(16))) uint16_t stage[K_MAX];
    const uint8_t* r = rec + (size_t)blockIdx.x * (HEADER + 2u * (size_t)k);
    uint16_t* o = out + (size_t)blockIdx.x * SAMPLE;
    const u32x4 head = *reinterpret_cast<const u32x4*>(r);
    const bool bad_head = head[0] != k || head[1] != MASKED_FMT_WORD || head[2] > 1u || head[3] != 0u;
    Sample s;
    if (bad_head || head[2] == 1u) {   // uniform: malformed, or poisoned (neither payload nor map is looked at)
        if (bad_head && threadIdx.x == 0) err_flag[0] = 1;
        nan_sample(s);
        store_sample(o, s);
        return;
    }
    const uint32_t nval = k / 8u;
    for (uint32_t i = threadIdx.x; i < nval; i += THREADS)
        reinterpret_cast<u32x4*>(stage)[i] = reinterpret_cast<const u32x4*>(r + HEADER)[i];
    const uint64_t m = load_map(map + (size_t)blockIdx.x * PIECES);
    uint32_t rank[ROUNDS], total;
    piece_ranks(m, W.gt, rank, total);   // its barrier also publishes the stage
    if (total != k) {                    // uniform, and before anything is written or gathered
        if (threadIdx.x == 0) err_flag[0] = 1;
        nan_sample(s);
        store_sample(o, s);
        return;
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const uint32_t b = byte_of(m, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t w = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int e = 2 * i + h;
                if ((b >> e) & 1u) {
                    const uint32_t slot = rank[j] + (uint32_t)__popc(b & ((1u << e) - 1u));   // < total == k
                    w |= (uint32_t)stage[slot & (K_MAX - 1)] << (16 * h);
                }
            }
            s.v[j][i] = w;
        }
    }
    store_sample(o, s);
}
}  // namespace

extern "C" int64_t slk_cuttopk_record_bytes(int k) { return k_ok(k) ? (int64_t)record_bytes(k) : -1; }
extern "C" int64_t slk_cuttopk_masked_record_bytes(int k) { return k_ok(k) ? (int64_t)masked_record_bytes(k) : -1; }

// Refusals in this order: negative counts, then n == 0 (nothing looked at), then the pointers, then k against the rule.
extern "C" int slk_cuttopk_encode(const void* x_bf16, int n, int k, void* rec, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && rec && aligned16(x_bf16) && aligned16(rec));
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_encode_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(static_cast<const uint16_t*>(x_bf16), (uint32_t)k,
                                                                        static_cast<uint8_t*>(rec));
    return slk_launch_status();
}

extern "C" int slk_cuttopk_decode(const void* rec, int n, int k, void* out_bf16, int* err_flag, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(rec && out_bf16 && err_flag && aligned16(rec) && aligned16(out_bf16));
    SLK_CHECK_ARG((reinterpret_cast<uintptr_t>(err_flag) & 3u) == 0);
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_decode_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(static_cast<const uint8_t*>(rec), (uint32_t)k,
                                                                        static_cast<uint16_t*>(out_bf16), err_flag);
    return slk_launch_status();
}

extern "C" int slk_cuttopk_roundtrip(const void* x_bf16, int n, int k, void* out_bf16, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && aligned16(x_bf16) && aligned16(out_bf16));
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_roundtrip_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(static_cast<const uint16_t*>(x_bf16),
                                                                           (uint32_t)k, static_cast<uint16_t*>(out_bf16));
    return slk_launch_status();
}

// The masked backward's entries: the family's refusals in the family's order; every pointer is required.
extern "C" int slk_cuttopk_roundtrip_map(const void* x_bf16, int n, int k, void* out_bf16, void* map, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(x_bf16 && out_bf16 && map && aligned16(x_bf16) && aligned16(out_bf16) && aligned16(map));
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_roundtrip_map_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(
        static_cast<const uint16_t*>(x_bf16), (uint32_t)k, static_cast<uint16_t*>(out_bf16), static_cast<uint8_t*>(map));
    return slk_launch_status();
}

extern "C" int slk_cuttopk_mask(const void* g_bf16, const void* map, int n, int k, void* out_bf16, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(g_bf16 && map && out_bf16 && aligned16(g_bf16) && aligned16(map) && aligned16(out_bf16));
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_mask_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(
        static_cast<const uint16_t*>(g_bf16), static_cast<const uint8_t*>(map), (uint32_t)k, static_cast<uint16_t*>(out_bf16));
    return slk_launch_status();
}

extern "C" int slk_cuttopk_gather(const void* g_bf16, const void* map, int n, int k, void* rec, void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(g_bf16 && map && rec && aligned16(g_bf16) && aligned16(map) && aligned16(rec));
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_gather_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(
        static_cast<const uint16_t*>(g_bf16), static_cast<const uint8_t*>(map), (uint32_t)k, static_cast<uint8_t*>(rec));
    return slk_launch_status();
}

extern "C" int slk_cuttopk_scatter(const void* rec, const void* map, int n, int k, void* out_bf16, int* err_flag,
                                   void* stream) {
    SLK_CHECK_ARG(n >= 0 && k >= 0);
    if (n == 0) return 0;
    SLK_CHECK_ARG(rec && map && out_bf16 && err_flag && aligned16(rec) && aligned16(map) && aligned16(out_bf16));
    SLK_CHECK_ARG((reinterpret_cast<uintptr_t>(err_flag) & 3u) == 0);
    if (!k_ok(k)) return (int)hipErrorInvalidConfiguration;
    cuttopk_scatter_kernel<<<(unsigned)n, THREADS, 0, slk_stream(stream)>>>(
        static_cast<const uint8_t*>(rec), static_cast<const uint8_t*>(map), (uint32_t)k, static_cast<uint16_t*>(out_bf16),
        err_flag);
    return slk_launch_status();
}
