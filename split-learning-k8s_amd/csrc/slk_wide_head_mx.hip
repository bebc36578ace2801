// slk_wide_head_mx.hip — the K5 server head run straight from MX cut records (include/slk.h, "The head on MX cut
// records"): what slk_cutmx_decode -> slk_wide_head -> slk_cutmx_encode compute, bit for bit, in the head's two
// launches, with no bf16 cut and no bf16 cut gradient in memory.
//
// The arithmetic is slk_wide_head.hip's, through the helpers of slk_wide_head.h: a chunk of 8 codes is decoded to the
// 8 bf16 the decoder would have written (cutmx's rule: exact, so the float32 the MFMA and the fma chains see are the
// same), and everything after that point is the same expression in the same order. What differs is how the bytes move.
//
// Pass 1, wide_head16_mx_kernel (16 samples per workgroup, 8 waves, wave w owning chunks [256 w, 256 w + 256)):
// an MX block of 32 stored elements is exactly the four 8-element chunks that the four kg lanes of a sample feed into
// one block of MFMAs, so lane (s16, kg) needs its chunk's 4 (e2m1) or 8 (e4m3) code bytes and shares the block's scale
// byte with the three other kg lanes. The codes come by each lane's own narrow load (the shipped form) or through
// a wave-private LDS tile filled by 16-byte loads (-DSLK_HEAD_MX_STAGED=1, measured no faster): see wide_head16_mx_kernel. The scale bytes of the 8 blocks a lane keeps in flight are 8 consecutive bytes
// of the record: one 8-byte load per round of 8 blocks. Every lane validates its own row's header (one 16-byte load,
// the same address in 32 lanes) and wave 0 leaves the verdict in `work` for pass 2.
// Epilogue: thread = chunk as in wide_head16_kernel; the 4 chunks of a block sit in 4 adjacent lanes, so the block's
// amax is two DPP quad_perm steps, every lane of the quad derives the same exponent and encodes its own 8 codes (one 4-
// or 8-byte store, 256 or 512 contiguous bytes a wave), and the scale bytes of four quads leave as one dword gathered
// by DPP row shifts. One thread writes the header. Every output byte has one writer; no atomics but the label flag's.
//
// Pass 2, wide_head_mx_back_kernel: wide_head_back_kernel<false> with the chunk's codes, its block's scale byte and
// the sample's verdict in the prefetch ring instead of 16 bytes of bf16.
#include "slk_common.h"
#include "slk_cutmx.h"
#include "slk_wide_head.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {
#ifndef SLK_HEAD_MX_STAGED
#define SLK_HEAD_MX_STAGED 0   // direct loads ship: the LDS tile is within 0.7 % either way (profiles/head_mx_ab*.txt)
#endif
constexpr int MX_PF = 8;   // blocks in flight per lane in pass 1 = the scale bytes of one 8-byte load
static_assert((WH_CPW / 4) % MX_PF == 0 && NCH % WH_T == 0, "head16 tiling");
static_assert(cutmx::BLOCK == 32 && cutmx::PAYLOAD_OFF % 16 == 0 && (cutmx::HEADER + WH_CPW / 4) % 8 == 0, "record layout");

// The codes of one 8-element chunk: 4 bytes (e2m1: element 2i in bits 0..3 of byte i) or 8 bytes (e4m3).
template <int FMT> struct Chunk;
template <> struct Chunk<0> { typedef uint32_t T; };
template <> struct Chunk<1> { typedef uint2 T; };

constexpr int rec_bytes(int fmt) { return fmt == 0 ? cutmx::record_bytes<0>() : fmt == 1 ? cutmx::record_bytes<1>() : CUTF * 2; }

__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi, int e) {
    return (uint32_t)cut8::scaled_bf16(__float_as_uint(lo), e) | ((uint32_t)cut8::scaled_bf16(__float_as_uint(hi), e) << 16);
}

// codes -> the 8 bf16 slk_cutmx_decode writes for them under block exponent e (the conversions of slk_cutmx.hip)
__device__ __forceinline__ uint4 decode_codes(uint32_t c, int e) {
    const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, 1.0f, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, 1.0f, 1);
    const f32x2 g = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, 1.0f, 2), h = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, 1.0f, 3);
    return make_uint4(bf16_pair(a[0], a[1], e), bf16_pair(b[0], b[1], e), bf16_pair(g[0], g[1], e), bf16_pair(h[0], h[1], e));
}
__device__ __forceinline__ uint4 decode_codes(uint2 c, int e) {
    const int x = (int)c.x, y = (int)c.y;
    return make_uint4(bf16_pair(__builtin_amdgcn_cvt_f32_fp8(x, 0), __builtin_amdgcn_cvt_f32_fp8(x, 1), e),
                      bf16_pair(__builtin_amdgcn_cvt_f32_fp8(x, 2), __builtin_amdgcn_cvt_f32_fp8(x, 3), e),
                      bf16_pair(__builtin_amdgcn_cvt_f32_fp8(y, 0), __builtin_amdgcn_cvt_f32_fp8(y, 1), e),
                      bf16_pair(__builtin_amdgcn_cvt_f32_fp8(y, 2), __builtin_amdgcn_cvt_f32_fp8(y, 3), e));
}

// The decoded chunk under scale byte sb: NaNs for a poisoned block (0xFF), a scale byte below 27 or a bad header.
template <typename C> __device__ __forceinline__ uint4 decode_chunk(C c, uint32_t sb, bool bad_head) {
    const uint4 v = decode_codes(c, (int)sb - cutmx::BIAS);
    const uint32_t n2 = cutmx::BF16_NAN | ((uint32_t)cutmx::BF16_NAN << 16);
    const bool nan = bad_head || sb < (uint32_t)(cutmx::E_MIN + cutmx::BIAS) || sb == cutmx::SCALE_NAN;
    return nan ? make_uint4(n2, n2, n2, n2) : v;
}

__device__ __forceinline__ bool bad_header(const uint4 head, int fmt) {
    return head.x != (uint32_t)cutmx::BLOCK || head.y != cutmx::FMT_WORD + (uint32_t)fmt || (head.z | head.w) != 0u;
}

// max (bits & 0x7fff) over the chunk's 8 bf16
__device__ __forceinline__ uint32_t chunk_amax(const uint4 v) {
    const uint32_t w[4] = {v.x & 0x7fff7fffu, v.y & 0x7fff7fffu, v.z & 0x7fff7fffu, v.w & 0x7fff7fffu};
    uint32_t a = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) a = max(a, max(w[k] & 0xffffu, w[k] >> 16));
    return a;
}

template <int CTRL> __device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}

// x * 2^-e of the two bf16 of a word (slk_cutmx.hip's scaled_pair: exact float32 products)
__device__ __forceinline__ void scaled_pair(uint32_t w, float s, float& lo, float& hi) {
    lo = __uint_as_float(w << 16) * s;
    hi = __uint_as_float(w & 0xffff0000u) * s;
}

// the 8 bf16 of a chunk -> their codes under block exponent e (slk_cutmx.hip's encode_block, a quarter of it)
template <int FMT> __device__ __forceinline__ typename Chunk<FMT>::T encode_chunk(const uint4 v, int e) {
    const float s = __uint_as_float((uint32_t)(127 - e) << 23);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (FMT == 0) {
        uint32_t c = 0;
        float lo, hi;
        scaled_pair(w[0], s, lo, hi);
        c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, lo, hi, 1.0f, 0);
        scaled_pair(w[1], s, lo, hi);
        c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, lo, hi, 1.0f, 1);
        scaled_pair(w[2], s, lo, hi);
        c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, lo, hi, 1.0f, 2);
        scaled_pair(w[3], s, lo, hi);
        c = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(c, lo, hi, 1.0f, 3);
        return c;
    } else {
        uint32_t c[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float f0, f1, f2, f3;
            scaled_pair(w[2 * i], s, f0, f1);
            scaled_pair(w[2 * i + 1], s, f2, f3);
            const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
            c[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, lo, true);
        }
        return make_uint2(c[0], c[1]);
    }
}

// Orders a wave's LDS stores before its later LDS loads (and the reverse) where the two belong to different lanes: the
// ring of the staged pass 1 is wave-private, so no barrier is needed, only that neither the compiler nor the wave's
// own issue order swaps them. Emits no instruction beyond the waits the loads need anyway.
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// FIN: the records' format; FOUT: the cut gradient's (-1: dense bf16 rows); STAGED: how pass 1 fetches the codes.
// false: lane (s16, kg) loads its chunk's 4 / 8 bytes itself. true: the wave fetches a slice of 8 blocks x 16 rows
// with 16-byte loads, lane = (row, 16-byte piece), so one load instruction covers 64 contiguous bytes in each of 16
// rows (2 instructions a slice for e2m1, 4 for e4m3, against 8 narrow ones); the next slice waits in registers while
// the current one sits in a wave-private LDS tile [16 rows][128 | 256 B + 16 B pad] from which lane (s16, kg) reads
// its chunk back (ds_read_b32 / b64; the pad spreads 16 rows x 4 chunks over 64 banks).
template <int FIN, int FOUT, bool STAGED>
__global__ __launch_bounds__(WH_T) void wide_head16_mx_kernel(
    const uint8_t* __restrict__ rec, const float* __restrict__ wf8, const float* __restrict__ bf,
    const int64_t* __restrict__ labels, const int* __restrict__ step_ptr, uint32_t seed, uint32_t thresh,
    float keep_scale, float grad_scale, float* __restrict__ logits, float* __restrict__ loss_i,
    float* __restrict__ dlogits, uint8_t* __restrict__ dout, uint8_t* __restrict__ kbits, uint8_t* __restrict__ verdict,
    int* __restrict__ label_err, int* __restrict__ rec_err, int b0, int B) {
    typedef typename Chunk<FIN>::T CIn;
    constexpr int RIN = rec_bytes(FIN), ROUT = rec_bytes(FOUT);
    __shared__ __attribute__((aligned(16))) uint8_t kbl[WH_S * WH_KBS];
    __shared__ __attribute__((aligned(16))) f32x4 red[WH_W * 64];
    __shared__ float zl[WH_S][NC];
    __shared__ float dls[WH_S][NC];
    constexpr int NI = MX_PF * 4 * (int)sizeof(CIn) / 64;   // 16-byte pieces per lane and slice (staged): 2 | 4
    constexpr int TROW = 64 * NI + 16;                      // tile row stride in bytes
    __shared__ __attribute__((aligned(16))) uint8_t tile[STAGED ? WH_W * WH_S * TROW : 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s0 = blockIdx.x * WH_S, ns = min(WH_S, B - s0);
    const uint32_t step = (uint32_t)*step_ptr;
    {
        const int s16 = lane & 15, kg = lane >> 4, sl = min(s16, ns - 1);  // rows past the batch: never stored
        const uint8_t* rrow = rec + (size_t)(s0 + sl) * RIN;
        const bool bad_head = bad_header(*reinterpret_cast<const uint4*>(rrow), FIN);
        if (tid < ns) {  // wave 0, kg 0: the sample's verdict for pass 2
            verdict[s0 + tid] = bad_head ? 1 : 0;
            if (bad_head) rec_err[0] = 1;
        }
        const CIn* prow = reinterpret_cast<const CIn*>(rrow + cutmx::PAYLOAD_OFF);
        const uint2* srow = reinterpret_cast<const uint2*>(rrow + cutmx::HEADER + wave * (WH_CPW / 4));
        const float4* wrow = reinterpret_cast<const float4*>(wf8 + (size_t)min(s16, NC - 1) * CUTF);
        const int cb = wave * WH_CPW + kg;
        const int bs = b0 + s0 + sl;
        // staged: this wave's share of the row's payload in 16-byte pieces, slice k = pieces [4 NI k, 4 NI (k + 1))
        const uint4* grow = reinterpret_cast<const uint4*>(prow + wave * WH_CPW) + kg;
        uint8_t* trow = tile + (STAGED ? (wave * WH_S + s16) * TROW : 0);
        CIn cv[STAGED ? 1 : MX_PF];
        uint4 g0 = {}, g1 = {}, g2 = {}, g3 = {};   // the next slice's pieces (g2, g3: e4m3 only)
        auto fetch = [&](int k) {
            g0 = grow[4 * NI * k];
            g1 = grow[4 * NI * k + 4];
            if constexpr (NI == 4) {
                g2 = grow[4 * NI * k + 8];
                g3 = grow[4 * NI * k + 12];
            }
        };
        float4 wv[MX_PF][2];
        uint2 sc = srow[0];
        if constexpr (STAGED) fetch(0);
#pragma unroll
        for (int p = 0; p < MX_PF; ++p) {
            if constexpr (!STAGED) cv[p] = prow[cb + 4 * p];
            wv[p][0] = wrow[2 * (cb + 4 * p)];
            wv[p][1] = wrow[2 * (cb + 4 * p) + 1];
        }
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            slk_keep(acc[q]);
        }
        bool bad_scale = false;
#pragma unroll 1
        for (int blk = 0; blk < WH_CPW / 4; blk += MX_PF) {
            const uint2 scur = sc;   // the scale bytes of blocks blk .. blk + 7
            if (blk + MX_PF < WH_CPW / 4) sc = srow[blk / MX_PF + 1];
            if constexpr (STAGED) {
                wave_lds_order();   // the last slice's reads are done
                uint4* tp = reinterpret_cast<uint4*>(trow) + kg;
                tp[0] = g0;
                tp[4] = g1;
                if constexpr (NI == 4) {
                    tp[8] = g2;
                    tp[12] = g3;
                }
                if (blk + MX_PF < WH_CPW / 4) fetch(blk / MX_PF + 1);
                wave_lds_order();   // every lane's pieces are in the tile
            }
#pragma unroll
            for (int p = 0; p < MX_PF; ++p) {
                const int ch = cb + 4 * (blk + p);
                CIn c;
                if constexpr (STAGED) c = *reinterpret_cast<const CIn*>(trow + (4 * p + kg) * sizeof(CIn));
                else c = cv[p];
                const float wf[8] = {wv[p][0].x, wv[p][0].y, wv[p][0].z, wv[p][0].w,
                                     wv[p][1].x, wv[p][1].y, wv[p][1].z, wv[p][1].w};
                if (blk + MX_PF < WH_CPW / 4) {
                    if constexpr (!STAGED) cv[p] = prow[ch + 4 * MX_PF];
                    wv[p][0] = wrow[2 * (ch + 4 * MX_PF)];
                    wv[p][1] = wrow[2 * (ch + 4 * MX_PF) + 1];
                }
                const uint32_t sb = ((p < 4 ? scur.x : scur.y) >> (8 * (p & 3))) & 0xffu;
                bad_scale |= sb < (uint32_t)(cutmx::E_MIN + cutmx::BIAS);
                const uint4 v = decode_chunk(c, sb, bad_head);
                float d[8];
                const uint32_t kb = dropped(v, bs, ch, step, seed, thresh, keep_scale, d);
                kbl[s16 * WH_KBS + ch] = (uint8_t)kb;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[i], wf[i], acc[i & 3], 0, 0, 0);
            }
        }
        if (bad_scale) rec_err[0] = 1;
        // D[4 (lane >> 4) + r][lane & 15] = (sample, class) partial over this wave's chunks
        red[wave * 64 + lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
    __syncthreads();
    if (tid < 256) {
        const int l = tid & 63, r = tid >> 6, n = l & 15, s = 4 * (l >> 4) + r;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WH_W; ++w) v += red[w * 64 + l][r];
        if (n < NC) zl[s][n] = v + bf[n];
    }
    __syncthreads();
    if (tid < WH_S) {  // cross-entropy of sample tid (wide_head16_kernel's lines)
        const int s = tid;
        if (s < ns) {
            const int b = s0 + s;
            float z[NC], m = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                z[j] = zl[s][j];
                m = fmaxf(m, z[j]);
            }
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < NC; ++j) se += expf(z[j] - m);
            const float lse = m + logf(se);
            const int64_t y = labels[b];
            const bool ok = y >= 0 && y < NC;
            if (!ok) atomicOr(label_err, 1);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const float g = ok ? (expf(z[j] - lse) - (j == y ? 1.f : 0.f)) * grad_scale : __builtin_nanf("");
                logits[(size_t)b * NC + j] = z[j];
                dlogits[(size_t)b * NC + j] = g;
                dls[s][j] = g;
            }
            loss_i[b] = ok ? lse - z[(int)y] : __builtin_nanf("");
        }
    }
    __syncthreads();
    // the dropout bits for pass 2 (kbits [B][2048])
#pragma unroll
    for (int i = tid; i < WH_S * NCH / 16; i += WH_T) {
        const int s = i / (NCH / 16), q = i - s * (NCH / 16);
        if (s < ns)
            reinterpret_cast<uint4*>(kbits + (size_t)(s0 + s) * NCH)[q] =
                *reinterpret_cast<const uint4*>(kbl + s * WH_KBS + 16 * q);
    }
    // cut gradient: thread = chunk (4 per thread), Wf's 80 floats of it in registers; the loops are uniform over the
    // workgroup (NCH % WH_T == 0), so all 64 lanes are active at every DPP step
#pragma unroll 1
    for (int ch = tid; ch < NCH; ch += WH_T) {
        float w[NC][8];
        load_w(wf8, ch, w);
#pragma unroll 1
        for (int s = 0; s < ns; ++s) {
            asm volatile("" ::: "memory");  // keeps the 16 x 10 dls reads from being hoisted out of the chunk loop
            float dlr[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) dlr[j] = dls[s][j];
            const uint4 o = dcut_chunk(w, dlr, kbl[s * WH_KBS + ch], keep_scale);
            uint8_t* orow = dout + (size_t)(s0 + s) * ROUT;
            if constexpr (FOUT < 0) {
                reinterpret_cast<uint4*>(orow)[ch] = o;
            } else {
                typedef typename Chunk<FOUT>::T COut;
                uint32_t a = chunk_amax(o);
                a = max(a, dpp<0xB1>(a));   // quad_perm 1,0,3,2
                a = max(a, dpp<0x4E>(a));   // quad_perm 2,3,0,1: the block's amax in its four lanes
                const bool poison = a >= 0x7f80u;
                const int e = poison ? 0 : cutmx::block_exp<FOUT>(a);
                const uint32_t sb = poison ? cutmx::SCALE_NAN : (uint32_t)(e + cutmx::BIAS);
                // the scale bytes of the four quads of 16 lanes as one word in the first of them (row_shl 4, 8, 12)
                const uint32_t sw = sb | (dpp<0x104>(sb) << 8) | (dpp<0x108>(sb) << 16) | (dpp<0x10C>(sb) << 24);
                if ((lane & 15) == 0) *reinterpret_cast<uint32_t*>(orow + cutmx::HEADER + (ch >> 2)) = sw;
                COut c = encode_chunk<FOUT>(o, e);
                if (poison) c = COut{};
                reinterpret_cast<COut*>(orow + cutmx::PAYLOAD_OFF)[ch] = c;
                if (ch == 0) *reinterpret_cast<uint4*>(orow) = make_uint4((uint32_t)cutmx::BLOCK, cutmx::FMT_WORD + (uint32_t)FOUT, 0u, 0u);
            }
        }
    }
}

// One sample's share of a chunk thread in pass 2: the codes, the block's scale byte, the sample's verdict.
template <int FMT> struct RawChunk {
    typename Chunk<FMT>::T c;
    uint32_t sb, bad;
};
template <int FMT>
__device__ __forceinline__ RawChunk<FMT> raw_chunk(const uint8_t* __restrict__ rec, const uint8_t* __restrict__ verdict, int b,
                                                   int fc, int B) {
    RawChunk<FMT> r{};
    if (b < B) {
        const uint8_t* rrow = rec + (size_t)b * rec_bytes(FMT);
        r.c = reinterpret_cast<const typename Chunk<FMT>::T*>(rrow + cutmx::PAYLOAD_OFF)[fc];
        r.sb = rrow[cutmx::HEADER + (fc >> 2)];
        r.bad = verdict[b];
    }
    return r;
}

template <int FIN>
__global__ __launch_bounds__(256) void wide_head_mx_back_kernel(const uint8_t* __restrict__ rec,
                                                                const float* __restrict__ dlogits, float keep_scale,
                                                                float* __restrict__ slabs, const uint8_t* __restrict__ kbits,
                                                                const uint8_t* __restrict__ verdict, int B) {
    const int slice = blockIdx.x % HSLICE, grp = blockIdx.x / HSLICE;
    const int fc = slice * 256 + threadIdx.x;
    float acc[NC][8];
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    float accb = 0.f;
    const int b1 = min(B, (grp + 1) * HSG);
    RawChunk<FIN> ring[HPF];
#pragma unroll
    for (int i = 0; i < HPF; ++i) ring[i] = raw_chunk<FIN>(rec, verdict, grp * HSG + i, fc, b1);
#pragma unroll 1
    for (int b = grp * HSG; b < b1; ++b) {
        const RawChunk<FIN> r = ring[0];
#pragma unroll
        for (int i = 0; i + 1 < HPF; ++i) ring[i] = ring[i + 1];
        ring[HPF - 1] = raw_chunk<FIN>(rec, verdict, b + HPF, fc, b1);
        const uint32_t kb = kbits[(size_t)b * NCH + fc];   // the forward's bits (pass 1)
        float d[8];
        unpack8(decode_chunk(r.c, r.sb, r.bad != 0u), d);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (kb >> k) & 1 ? d[k] * keep_scale : 0.f;
        const float* dl = dlogits + (size_t)b * NC;
        float dlr[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) dlr[j] = dl[j];
#pragma unroll
        for (int j = 0; j < NC; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = __builtin_fmaf(dlr[j], d[k], acc[j][k]);
        if (slice == 0 && threadIdx.x < NC) accb += dl[threadIdx.x];
    }
    float* slab = slabs + (size_t)grp * (NC * CUTF + NC);
    const int plane = fc >> 6, pix = fc & 63;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) slab[(size_t)j * CUTF + (plane * 8 + k) * 64 + pix] = acc[j][k];
    if (slice == 0 && threadIdx.x < NC) slab[NC * CUTF + threadIdx.x] = accb;
}

struct HeadMxArgs {
    const uint8_t* rec;
    const float *wf8, *bf;
    const int64_t* labels;
    const int* step;
    uint32_t seed, thresh;
    float keep_scale, grad_scale;
    float *logits, *loss_i, *dlogits;
    uint8_t* dout;
    float* slabs;
    uint8_t* work;
    int *label_err, *rec_err;
    int b0, B;
    hipStream_t st;
};

template <int FIN, int FOUT> void launch(const HeadMxArgs& a) {
    constexpr bool STAGED = SLK_HEAD_MX_STAGED != 0;
    uint8_t* verdict = a.work + (size_t)a.B * NCH;   // behind the dropout bits
    hipLaunchKernelGGL((wide_head16_mx_kernel<FIN, FOUT, STAGED>), dim3((a.B + WH_S - 1) / WH_S), dim3(WH_T), 0, a.st, a.rec, a.wf8, a.bf,
                       a.labels, a.step, a.seed, a.thresh, a.keep_scale, a.grad_scale, a.logits, a.loss_i, a.dlogits, a.dout,
                       a.work, verdict, a.label_err, a.rec_err, a.b0, a.B);
    hipLaunchKernelGGL(wide_head_mx_back_kernel<FIN>, dim3(HSLICE * slk_wide_head_nslab(a.B)), dim3(256), 0, a.st, a.rec,
                       a.dlogits, a.keep_scale, a.slabs, (const uint8_t*)a.work, (const uint8_t*)verdict, a.B);
}
template <int FIN> void launch_in(const HeadMxArgs& a, int fmt_out) {
    if (fmt_out == 0) launch<FIN, 0>(a);
    else if (fmt_out == 1) launch<FIN, 1>(a);
    else launch<FIN, -1>(a);
}

inline bool aligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
}  // namespace

// the dropout bits (B x 2048 B, slk_wide_head_work) and one verdict byte per sample behind them
extern "C" int slk_wide_head_mx_work(int B) { return B > 0 ? B * (NCH / 4) + (B + 3) / 4 : 0; }

extern "C" int slk_wide_head_mx(const void* rec_in, int fmt_in, const float* wf8, const float* bf, const int64_t* labels,
                                const int* step, uint32_t seed, uint32_t keep_threshold, float keep_scale, float grad_scale,
                                float* logits, float* loss_i, float* dlogits, void* dcut_out, int fmt_out, float* slabs,
                                float* work, int* label_err, int* rec_err, int b0, int B, void* stream) {
    SLK_CHECK_ARG(B >= 0 && b0 >= 0 && (fmt_in == 0 || fmt_in == 1) && fmt_out >= -1 && fmt_out <= 1);
    if (B == 0) return 0;
    SLK_CHECK_ARG(rec_in && wf8 && bf && labels && step && logits && loss_i && dlogits && dcut_out && slabs && work &&
                  label_err && rec_err);
    SLK_CHECK_ARG(aligned(rec_in, 16) && aligned(dcut_out, 16) && aligned(work, 16) && aligned(label_err, 4) &&
                  aligned(rec_err, 4));
    const HeadMxArgs a{static_cast<const uint8_t*>(rec_in), wf8, bf, labels, step, seed, keep_threshold, keep_scale,
                       grad_scale, logits, loss_i, dlogits, static_cast<uint8_t*>(dcut_out), slabs,
                       reinterpret_cast<uint8_t*>(work), label_err, rec_err, b0, B, slk_stream(stream)};
    if (fmt_in == 0) launch_in<0>(a, fmt_out);
    else launch_in<1>(a, fmt_out);
    return slk_launch_status();
}
