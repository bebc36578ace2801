// Host-side check of the layer-wise launches' layout and argument validation (slk_trust_layout in
// csrc/slk_common.h and the refusals of the four entry points), as a stand-alone program for a sanitizer run:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -I include -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer tools/trust_layout_check.cpp split-learning-k8s_amd/csrc/slk_optim.hip \
//         -o /tmp/trust_layout_check && /tmp/trust_layout_check
//
// Every call here is refused before a launch (or only computes the layout), so it needs no GPU.
#include <cstdio>
#include <cstdlib>

#include "../split-learning-k8s_amd/csrc/slk_common.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

int main() {
    SlkTrustLayout L;
    // the fused K2 step: the server's two pairs (group 0), the client's one (group 1), at B = 4096's slab counts
    {
        const int nslab[3] = {256, 64, 256}, n[3] = {18496, 92170, 320}, nw[3] = {18432, 92160, 288}, g[3] = {0, 0, 1};
        CHECK(slk_trust_layout(nslab, n, nw, g, 3, 2, L));
        CHECK(L.c.nblk[0] == 289 && L.c.nblk[1] == 361 && L.c.nblk[2] == 5);
        CHECK(L.c.off[0] == 0 && L.c.off[1] == 289 && L.c.off[2] == 0);
        CHECK(L.slot[0] == 0 && L.slot[1] == 1 && L.slot[2] == 0);
    }
    // four segments of one group; nw at both ends
    {
        const int nslab[4] = {1, 17, 65, 1}, n[4] = {1300, 1300, 1300, 0}, nw[4] = {0, 1300, 1024, 0}, g[4] = {0, 0, 0, 0};
        CHECK(slk_trust_layout(nslab, n, nw, g, 4, 1, L));
        CHECK(L.c.nblk[0] == 2 && L.c.nblk[1] == 6 && L.c.nblk[2] == 21 && L.c.nblk[3] == 0);
        CHECK(L.c.off[3] == 29 && L.slot[3] == 3);
    }
    // refusals of the layout
    {
        const int nslab[2] = {1, 1}, n[2] = {100, 100}, g[2] = {0, 1};
        const int over[2] = {101, 0}, neg[2] = {0, -1}, ok[2] = {100, 0}, gap[2] = {0, 2}, zslab[2] = {1, 0};
        CHECK(!slk_trust_layout(nslab, n, over, g, 2, 2, L));
        CHECK(!slk_trust_layout(nslab, n, neg, g, 2, 2, L));
        CHECK(!slk_trust_layout(nslab, n, nullptr, g, 2, 2, L));
        CHECK(!slk_trust_layout(nslab, n, ok, gap, 2, 2, L));
        CHECK(!slk_trust_layout(zslab, n, ok, g, 2, 2, L));
        CHECK(!slk_trust_layout(nslab, n, ok, g, 2, 1, L));
        CHECK(!slk_trust_layout(nslab, n, ok, g, 0, 1, L));
        CHECK(!slk_trust_layout(nslab, n, ok, g, 5, 2, L));
        CHECK(slk_trust_layout(nslab, n, ok, g, 2, 2, L));
    }
    // refusals of the entry points (host pointers: nothing is dereferenced before the checks pass, nothing launched)
    {
        alignas(16) static float buf[64];
        float* p[5] = {buf, buf, buf, buf, buf};
        const float* cp[5] = {buf, buf, buf, buf, buf};
        const int nslab[5] = {1, 1, 1, 1, 1}, n[5] = {8, 8, 8, 8, 8}, g[5] = {0, 0, 0, 0, 0};
        const int over[5] = {9, 0, 0, 0, 0}, neg[5] = {-1, 0, 0, 0, 0}, ok[5] = {4, 4, 4, 4, 4};
        const int step = 0;
        const float lr = 0.1f;
        const int inv = (int)hipErrorInvalidValue;
        for (const int* nw : {over, neg}) {
            CHECK(slk_reduce_tnorm_multi(p, cp, cp, nslab, n, nw, g, 1, p, 1, nullptr, 0, 0.f, nullptr, 0, nullptr, nullptr) == inv);
            CHECK(slk_lars_multi(p, cp, p, nslab, n, nw, g, 1, cp, p, 1, &lr, 1, &step, 0.9f, 0.f, 0.f, 0, 1e-3f, 1e-8f, 1, nullptr) == inv);
            CHECK(slk_lamb_moments_multi(p, cp, p, p, cp, nslab, n, nw, g, 1, p, 1, &step, 0.9f, 0.999f, 1e-6f, 0.01f, 1, nullptr, 0,
                                         0.f, nullptr, 0, nullptr, nullptr) == inv);
            CHECK(slk_lamb_multi(p, p, p, nslab, n, nw, g, 1, cp, p, 1, &lr, 1, &step, 0.9f, 0.999f, 1e-6f, 0.01f, 1, nullptr) == inv);
        }
        CHECK(slk_reduce_tnorm_multi(p, cp, cp, nslab, n, ok, g, 5, p, 1, nullptr, 0, 0.f, nullptr, 0, nullptr, nullptr) == inv);
        CHECK(slk_lamb_multi(p, p, p, nslab, n, ok, g, 5, cp, p, 1, &lr, 1, &step, 0.9f, 0.999f, 1e-6f, 0.01f, 1, nullptr) == inv);
        CHECK(slk_reduce_tnorm_multi(nullptr, cp, cp, nslab, n, ok, g, 1, p, 1, nullptr, 0, 0.f, nullptr, 0, nullptr, nullptr) == inv);
        CHECK(slk_lars_multi(p, cp, nullptr, nslab, n, ok, g, 1, cp, p, 1, &lr, 1, &step, 0.9f, 0.f, 0.f, 0, 1e-3f, 1e-8f, 1, nullptr) == inv);
        CHECK(slk_lars_multi(p, cp, p, nslab, n, ok, g, 1, cp, nullptr, 1, &lr, 1, &step, 0.9f, 0.f, 0.f, 0, 1e-3f, 1e-8f, 1, nullptr) == inv);
        CHECK(slk_lamb_moments_multi(p, cp, p, nullptr, cp, nslab, n, ok, g, 1, p, 1, &step, 0.9f, 0.999f, 1e-6f, 0.01f, 1, nullptr, 0,
                                     0.f, nullptr, 0, nullptr, nullptr) == inv);
        float* misaligned[1] = {buf + 1};
        CHECK(slk_reduce_tnorm_multi(p, cp, cp, nslab, n, ok, g, 1, misaligned, 1, nullptr, 0, 0.f, nullptr, 0, nullptr, nullptr) == inv);
    }
    std::puts("trust_layout_check: ok");
    return 0;
}
