"""Test infrastructure: the work partitions of the persistent conv kernels restated in Python, from the launch code
alone (csrc/slk_x3.hip, csrc/slk_wide.hip). tests/test_unit_partition_cpu.py executes every claim that the docstring
of tests/test_steady_exact_gpu.py makes about a batch; that file uses the same functions for its host-side guards.

K2 x3 kernels: a workgroup (or K share) walks the CONTIGUOUS range [u0, u1) of n units,
    per = ceil(n / G), u0 = min(i per, n), u1 = min(u0 + per, n)          (workgroup / share i of G)
  forward x3 / x3s / x3i / x3p   n = 3 B units (thirds of a sample), G = min(3 B, 256)
  forward x3sa (in-kernel amax)  n = 3 B, G = min(B, 256), per = 3 ceil(B / G): whole samples
  dgrad, dgrad_c1w, dgrad_pack   n = 3 B pairs (sample, part), G = min(3 B, 256)
  wgrad x3 (f32 act)             n = 3 B, G = min(3 B, 128) K shares (x 2 co halves that walk the same range)
  wgrad x3s (images, 2:4 sparse) n = 3 B, G = min(6 B, 256) K shares
Direct forward / dgrad (csrc/slk_server.hip) and Winograd dgrad (csrc/slk_wino.hip): whole samples b = i, i + G, ...
with G = min(B, 256); Winograd forward: super-units (two bands = thirds of a sample) su = i, i + 256, ...
K5 weight gradients (wide_wgrad_kernel<WgCfg<CI, CO, HW, TR>>): 256 workgroups = NBLK blocks x KSPLIT shares; share ks
walks the tile slots t = ks, ks + KSPLIT, ... while valid(t); slot t is image n = (j / RB) 8 + (t & 7), row block
rb = j % RB with j = t >> 3, RB = HW / TR; valid(t) = n < B.
"""
from collections import Counter, namedtuple


def ceil_div(a, b):
    return -(-a // b)


def contiguous_ranges(n, G, per=None):
    """[(u0, u1)] of workgroups 0..G-1."""
    per = ceil_div(n, G) if per is None else per
    out = []
    for i in range(G):
        u0 = min(i * per, n)
        out.append((u0, min(u0 + per, n)))
    return per, out


def x3_fwd(B):
    return contiguous_ranges(3 * B, min(3 * B, 256))


def x3_fwd_amax(B):
    G = min(B, 256)
    return contiguous_ranges(3 * B, G, per=3 * ceil_div(B, G))


def x3_dgrad(B):
    return contiguous_ranges(3 * B, min(3 * B, 256))


def x3_wgrad_f32(B):
    return contiguous_ranges(3 * B, min(3 * B, 128))


def x3_wgrad_images(B):
    return contiguous_ranges(3 * B, min(6 * B, 256))


def strided(n, G):
    """[(0, count)] per workgroup of a strided walk u = i, i + G, ... < n (lengths only: for length_counts).
    The direct forward / dgrad and the Winograd dgrad walk whole samples this way with G = min(B, 256)."""
    G = min(n, G)
    return [(0, len(range(i, n, G))) for i in range(G)]


def wino_fwd(B):
    """The Winograd forward: super-units su = i, i + 256, ... of the ceil(3 B / 2) pairs of bands (band 2 su + pr)."""
    return strided((3 * B + 1) // 2, 256)


def length_counts(ranges):
    """{range length: number of workgroups}."""
    return dict(Counter(u1 - u0 for u0, u1 in ranges))


def sample_span(ranges):
    """The largest number of samples (unit // 3) that one range touches."""
    return max(((u1 - 1) // 3 - u0 // 3 + 1) for u0, u1 in ranges if u1 > u0)


def lag_pairs(ranges, lags=(2, 3)):
    """Every (u, u - d) with both units inside one range: the unit whose operands last sat in a two-slot (d = 2) or
    three-slot (d = 3) buffer that unit u now reads, and for d = 2 also the one a three-slot ring held before."""
    a, b = [], []
    for u0, u1 in ranges:
        for u in range(u0, u1):
            for d in lags:
                if u - d >= u0:
                    a.append(u)
                    b.append(u - d)
    return a, b


def x3i_refills(ranges):
    """The act16 forward's three-slot ring: at position k (unit u = u0 + k) it reads slot k % 3 and requests unit
    min(u + 2, u1 - 1) into slot (k + 2) % 3; units u0 and u0 + 1 are requested before the loop. A request is a real
    refill when the slot was read before (k >= 1) and the unit is not the clamped one (u + 2 < u1; the clamped
    request is never read). Returns per workgroup the list of refilled slots, in order: the unit of refill i is read
    at position i + 3, two positions after its request."""
    return [[(k + 2) % 3 for k in range(1, u1 - u0) if u0 + k + 2 < u1] for u0, u1 in ranges]


# ----------------------------------------------------------------------------- K5 weight gradients
WgCfg = namedtuple("WgCfg", "CI CO HW TR")
WG2 = WgCfg(64, 128, 32, 4)       # conv2: RB 8, NBLK 1, KSPLIT 256
WG3 = WgCfg(128, 256, 16, 8)      # conv3: RB 2, NBLK 4, KSPLIT 64


def wg_rb(c):
    return c.HW // c.TR


def wg_ksplit(c):
    return 256 // ((c.CO // 128) * (c.CI // 64))


def tile_of(c, t):
    j = t >> 3
    return (j // wg_rb(c)) * 8 + (t & 7), j % wg_rb(c)


def valid(c, t, B):
    return tile_of(c, t)[0] < B


def share_slots(c, ks, B, rounds):
    """valid() of the first `rounds` slots of share ks, walked or not."""
    return [valid(c, ks + k * wg_ksplit(c), B) for k in range(rounds)]


def share_tiles(c, ks, B):
    """The tiles share ks walks: the kernel's loop `for (t = ks; valid(t); t += KSPLIT)`."""
    out, t = [], ks
    while valid(c, t, B):
        out.append(t)
        t += wg_ksplit(c)
    return out
