"""The cut-noise rule (include/slk.h, "Cut noise") restated in numpy, independently of splitcnn/privacy.py and of the
kernel: the uint32 hash on uint64 arrays, the float32 reduction in the kernel's documented order with every product and
sum cast to float32, bf16 round-to-nearest-even by bits. Rows are uint16 arrays of bf16 bits, [n, 16384].

THE NORM'S BOUND (norm_bound). A bf16 value has an 8-bit significand, so fl(x * x) is exact in float32 (16 bits)
unless it underflows: for elements that are 0 or at least 2^-60 in magnitude, and a sum below 2^127, the only errors of
s2 are those of the additions. Every term is non-negative and reaches the total through at most 63 rounded additions
inside its thread (the first of the 64 adds to 0 and is exact), 6 in the wave's butterfly and 2 across the waves: 71
roundings, each (1 + d), |d| <= u = 2^-24. Non-negative terms cannot cancel, so s2^ = s2 (1 + th) with
|th| <= (1 + u)^71 - 1 < 71.01 u. The square root is correctly rounded: norm^ = sqrt(s2^) (1 + d'), |d'| <= u, and
|sqrt(1 + th) - 1| <= |th| / 2 + th^2 / 2. Together |norm^ - norm| <= (35.51 + 1 + 1e-3) u norm < 37 u norm."""
import math

import numpy as np

SAMPLE = 16384
THREADS = 256
TABLE = 1024
M32 = 0xFFFFFFFF
U = 2.0 ** -24
NORM_RTOL = 37 * U
CLIP = 8.0


def norm_bound(norm64):
    """The bound above on |norm^ - norm| for float64 norms of rows inside its preconditions."""
    return NORM_RTOL * np.asarray(norm64, dtype=np.float64)


def norm_bound_applies(bits):
    """Rows whose elements are all 0 or finite with magnitude >= 2^-60, and whose exact s2 is below 2^127."""
    x = to_f32(bits).astype(np.float64)
    ok = np.isfinite(x).all(axis=1) & ((x == 0) | (np.abs(x) >= 2.0 ** -60)).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        return ok & ((np.where(np.isfinite(x), x, 0.0) ** 2).sum(axis=1) < 2.0 ** 127)


# ------------------------------------------------------------------------------------------------ bits
def to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(f):
    """float32 -> bf16 bits, round to nearest even; a NaN becomes 0x7FC0."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7FC0), r)


def is_nan_bits(bits):
    b = np.asarray(bits, dtype=np.uint16)
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def same_bits(got, want):
    """Bit for bit, NaNs compared by NaN-ness only."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = is_nan_bits(got), is_nan_bits(want)
    return got.shape == want.shape and bool(np.array_equal(gn, wn) and np.array_equal(got[~wn], want[~wn]))


def same_f32(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(gn, wn) and
                                            np.array_equal(got[~wn].view(np.uint32), want[~wn].view(np.uint32)))


# ------------------------------------------------------------------------------------------------ draws
def hash32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def clz32(x):
    """Leading zeros of uint32 values held in uint64 arrays; 32 for 0."""
    n = np.full(x.shape, 32, dtype=np.int64)
    v = x.copy()
    for _ in range(32):
        live = v != 0
        n = n - live
        v = v >> np.uint64(1)
    return n


def words(rows, t, seed):
    """(r, r2) of every element of the global rows `rows` at counter t: uint64 arrays [len(rows), 16384]."""
    g = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    i = np.arange(SAMPLE, dtype=np.uint64).reshape(1, -1)
    m = np.uint64(M32)
    key = np.uint64((((t & M32) * 0x85EBCA77) + ((seed & M32) * 0xC2B2AE3D) + 3 * 0x27D4EB2F) & M32)
    base = hash32(((g * np.uint64(0x9E3779B1)) + key) & m)
    r = hash32((base + i * np.uint64(0x9E3779B1)) & m)
    r2 = hash32((r + np.uint64(0x9E3779B9)) & m)
    return r, r2


def draws(rows, t, seed, variant=None):
    r, r2 = words(rows, t, seed)
    neg = (r >> np.uint64(31)).astype(bool)
    k = ((r if variant == "k_low" else (r >> np.uint64(21))) & np.uint64(1023)).astype(np.int64)
    G = clz32(r if variant == "G_from_r" else r2)
    return neg, k, G


def noise(rows, t, seed, table, tail, scale, variant=None):
    """float32 [len(rows), 16384]: n = +-fl(scale * fl(fl(tail * G) + table[k]))."""
    neg, k, G = draws(rows, t, seed, variant)
    table = np.asarray(table, dtype=np.float32)
    a = (np.float32(tail) * G.astype(np.float32)).astype(np.float32)
    a = (a + table[k]).astype(np.float32)
    n = (np.float32(scale) * a).astype(np.float32)
    return np.where(neg, -n, n).astype(np.float32), a


# ------------------------------------------------------------------------------------------------ clip
def sumsq(x):
    """s2 of float32 rows [n, 16384] in the kernel's order."""
    n = x.shape[0]
    v = x.reshape(n, 4, THREADS, 16).transpose(0, 2, 1, 3).reshape(n, THREADS, 64)   # [row, thread, j * 16 + e]
    acc = np.zeros((n, THREADS), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for e in range(64):
            p = (v[:, :, e] * v[:, :, e]).astype(np.float32)
            acc = (acc + p).astype(np.float32)
        acc = acc.reshape(n, 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, :, lane ^ o]).astype(np.float32)
        w = acc[:, :, 0]
        return ((w[:, 0] + w[:, 1]).astype(np.float32) + (w[:, 2] + w[:, 3]).astype(np.float32)).astype(np.float32)


def clip_stats(x, max_norm):
    """(norm, coef) float32 [n] each."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        norm = np.sqrt(sumsq(x)).astype(np.float32)
        q = (np.float32(max_norm) / (norm + np.float32(1e-6)).astype(np.float32)).astype(np.float32)
        coef = np.where(q > np.float32(1.0), np.float32(1.0), q).astype(np.float32)
    return norm, coef


def apply(bits, table=None, tail=0.0, scale=None, clip=None, seed=0, t=0, row0=0, variant=None):
    """(y bits [n, 16384], stats float32 [n, 2] or None). scale=None: no noise; clip=None: no clip."""
    x = to_f32(bits)
    n = x.shape[0]
    stats = None
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        nz = None
        if scale is not None:
            nz, a = noise(np.arange(row0, row0 + n), t, seed, table, tail, scale, variant)
        if variant == "noise_before_clip" and nz is not None:
            x = (x + nz).astype(np.float32)
        c = x
        if clip is not None:
            norm, coef = clip_stats(x, clip)
            stats = np.stack([norm, coef], axis=1)
            c = (coef[:, None] * x).astype(np.float32)
        if nz is not None and variant != "noise_before_clip":
            if variant == "fma":   # one rounding of c + scale * a: the contracted form
                s = np.where(draws(np.arange(row0, row0 + n), t, seed)[0], -1.0, 1.0)
                c = (c.astype(np.float64) + s * np.float64(np.float32(scale)) * a.astype(np.float64)).astype(np.float32)
            else:
                c = (c + nz).astype(np.float32)
    return to_bf16(c), stats


def scale_rows(bits, stats):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return to_bf16((np.asarray(stats, dtype=np.float32)[:, 1:2] * to_f32(bits)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ laws
def laplace_table():
    return np.array([-math.log1p(-(k + 0.5) / 2048.0) for k in range(TABLE)], dtype=np.float64), math.log(2.0)


def law_moments(table, tail):
    """(E x^2, E x^4, E |x|) of the unit-scale law in float64: the magnitude tail * G + table[k], G geometric
    (P(G = g) = 2^-(g+1) for g < 32, P(G = 32) = 2^-32), k uniform, by enumeration; the sign is symmetric."""
    table = np.asarray(table, dtype=np.float64)
    pg = np.array([2.0 ** -(g + 1) for g in range(32)] + [2.0 ** -32])
    mag = tail * np.arange(33)[:, None] + table[None, :]
    w = pg[:, None] / TABLE
    return float((w * mag ** 2).sum()), float((w * mag ** 4).sum()), float((w * mag).sum())


# ------------------------------------------------------------------------------------------------ the test set
LAWS = ("laplace", "gaussian", "hand")
SCALES = {"laplace": 0.3, "gaussian": 0.75, "hand": 0.37}   # no powers of two: fl(scale * a) rounds
KEYS = [(0, 0, 0), (5, 1, 0), (0xDEADBEEF, 0x80000003, 7), (1, 12345, 1000)]   # (seed, step, row0)


def hand_table():
    """A hand-made table with a nonzero tail: nothing like a quantile function."""
    k = np.arange(TABLE, dtype=np.float64)
    return (0.05 + ((k * 37) % 1024) / 1024.0).astype(np.float32), 0.25


def _scaled_to(row64, target):
    return to_bf16((row64 * (target / np.sqrt((row64 ** 2).sum()))).astype(np.float32))


def samples():
    """[(name, bf16 bits [16384])]: the rows every device test runs."""
    rng = np.random.default_rng(20240607)
    relu = [np.maximum(rng.standard_normal(SAMPLE), 0.0) * s for s in (1.0, 0.05, 3.0)]
    out = [("all_zero", np.zeros(SAMPLE, dtype=np.uint16))]
    out += [(f"relu_{i}", to_bf16(r.astype(np.float32))) for i, r in enumerate(relu)]
    out.append(("under_clip", _scaled_to(relu[0], CLIP * (1 - 1e-3))))
    out.append(("over_clip", _scaled_to(relu[0], CLIP * (1 + 1e-3))))
    signed = to_bf16((rng.standard_normal(SAMPLE) * 0.1).astype(np.float32))
    signed[::7] = 0x8000
    out.append(("signed_neg_zero", signed))
    top = to_bf16(relu[1].astype(np.float32))
    top[[3, 4000, 16383]] = 0x7F7F
    top[5] = 0xFF7F
    out.append(("bf16_max", top))
    nan = to_bf16(relu[0].astype(np.float32))
    nan[1234] = 0x7FC0
    out.append(("has_nan", nan))
    inf = to_bf16(relu[0].astype(np.float32))
    inf[4321] = 0x7F80
    out.append(("has_inf", inf))
    out.append(("tiny", _scaled_to(relu[2], 1e-3)))
    return out


def sample_bits():
    return np.stack([b for _, b in samples()])
