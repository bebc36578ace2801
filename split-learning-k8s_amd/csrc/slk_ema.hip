// slk_ema.hip — exponential moving average of the parameters (include/slk.h, slk_ema_multi).
//
// One launch moves up to 8 segments (e, p, n): e <- e + (1 - d)(p - e), or e <- p before `start`. The launch is
// latency, not bandwidth (1.3 MB for K2, 6.4 MB for K5 per step), so it is sized like the optimizer launches it
// follows: a flat list of work items, 256 per block, every item owned by exactly one thread — an item is one
// 16-byte vector of a segment's aligned body or one scalar of its head / tail. Nothing is shared between threads:
// no atomics, no LDS, and the result of an element does not depend on the grid or on what else is in the launch.
#include "slk_common.h"

struct EmaSeg {
    float* e;
    const float* p;
    int n;     // elements
    int head;  // scalars in front of the vector body (n when the two pointers' 16-byte phases differ)
    int nvec;  // 16-byte vectors of the body: elements [head, head + 4 * nvec)
    int nblk;  // blocks of 256 items: nvec vectors, then the head and the tail scalars
};
struct EmaMulti {
    EmaSeg seg[SLK_EMA_MAXSEG];
    int nseg;
    const float* decay;
    const int* step;
    int start, warmup;
};

// fl(1 - d) of this step and whether it is a copy (include/slk.h, "the rule"); uniform over the launch.
__device__ __forceinline__ float ema_weight(const EmaMulti& a, bool& copy) {
    const int k = *a.step;
    copy = k < a.start;
    float d = *a.decay;
    if (a.warmup) {
        const float nf = (float)((unsigned)(copy ? 0 : k - a.start) + 1u);  // n = t + 1 <= 2^31, nearest even
        const float w = (1.f + nf) / (10.f + nf);
        d = w < d ? w : d;
    }
    return 1.f - d;
}

__device__ __forceinline__ float ema_one(float e, float p, float omd, bool copy) {
    const float diff = p - e;
    return copy ? p : __builtin_fmaf(omd, diff, e);
}

__device__ __forceinline__ void ema_block(const EmaSeg& g, int blk, float omd, bool copy) {
    const int64_t item = (int64_t)blk * 256 + threadIdx.x;
    if (item < g.nvec) {
        const size_t o = (size_t)g.head + 4 * (size_t)item;
        const f32x4 p = *reinterpret_cast<const f32x4*>(g.p + o);
        f32x4 e = *reinterpret_cast<const f32x4*>(g.e + o);
        e.x = ema_one(e.x, p.x, omd, copy);
        e.y = ema_one(e.y, p.y, omd, copy);
        e.z = ema_one(e.z, p.z, omd, copy);
        e.w = ema_one(e.w, p.w, omd, copy);
        *reinterpret_cast<f32x4*>(g.e + o) = e;
        return;
    }
    const int64_t j = item - g.nvec;              // scalar j of this segment: the head, then the tail
    const int64_t body = 4 * (int64_t)g.nvec;
    if (j < (int64_t)g.n - body) {
        const size_t o = (size_t)(j < g.head ? j : j + body);
        g.e[o] = ema_one(g.e[o], g.p[o], omd, copy);
    }
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const EmaMulti a) {
    bool copy;
    const float omd = ema_weight(a, copy);
    int blk = blockIdx.x;
#pragma unroll
    for (int s = 0; s < SLK_EMA_MAXSEG; ++s) {
        if (s < a.nseg) {
            if (blk < a.seg[s].nblk) {
                ema_block(a.seg[s], blk, omd, copy);
                return;
            }
            blk -= a.seg[s].nblk;
        }
    }
}

extern "C" int slk_ema_multi(float* const* e, const float* const* p, const int* n, int nseg, const float* decay,
                             const int* step, int start, int warmup, void* stream) {
    SLK_CHECK_ARG(e && p && n && decay && step);
    SLK_CHECK_ARG(nseg >= 1 && nseg <= SLK_EMA_MAXSEG && start >= 0);
    EmaMulti a{};
    int64_t nblk = 0;
    for (int s = 0; s < nseg; ++s) {
        SLK_CHECK_ARG(n[s] >= 0 && ((e[s] && p[s]) || n[s] == 0));  // an empty segment may have no address
        const uintptr_t ea = reinterpret_cast<uintptr_t>(e[s]), pa = reinterpret_cast<uintptr_t>(p[s]);
        const uintptr_t bytes = 4 * (uintptr_t)n[s];
        SLK_CHECK_ARG(((ea | pa) & 3u) == 0 && (ea != pa || !ea));
        SLK_CHECK_ARG(ea + bytes <= pa || pa + bytes <= ea);  // the two blocks do not overlap
        int head = n[s];
        if ((ea & 15u) == (pa & 15u)) {
            head = (int)(((16u - (ea & 15u)) & 15u) / 4u);
            if (head > n[s]) head = n[s];
        }
        const int nvec = (n[s] - head) / 4;
        const int64_t items = (int64_t)nvec + (n[s] - 4 * (int64_t)nvec);
        a.seg[s] = EmaSeg{e[s], p[s], n[s], head, nvec, (int)((items + 255) / 256)};
        nblk += a.seg[s].nblk;
    }
    SLK_CHECK_ARG(nblk <= 0x7fffffff);
    a.nseg = nseg;
    a.decay = decay;
    a.step = step;
    a.start = start;
    a.warmup = warmup ? 1 : 0;
    if (nblk == 0) return 0;
    ema_multi_kernel<<<(unsigned)nblk, 256, 0, slk_stream(stream)>>>(a);
    return slk_launch_status();
}
