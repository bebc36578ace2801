"""Layer-wise trust ratios (slk_reduce_tnorm_multi -> slk_lars_multi, slk_lamb_moments_multi -> slk_lamb_multi): a
float64 closed form of both recipes, a numpy float32 emulation of the partials and per-tensor totals in the order
include/slk.h documents, and the derived error bounds. Test infrastructure only (tests/test_layerwise_ref_cpu.py pins
it on the CPU; tests/test_layerwise_gpu.py and tests/test_layerwise_trainer_gpu.py use it on the GPU).

A tensor is the weight part [0, nw) or the bias part [nw, n) of one [W | b] segment.

The order. Pass 1: the thread that owns column i holds x2 = fl(x * x) and p2 = fl(p * p) in the weight pair or the bias
pair of [x2_W, p2_W, x2_b, p2_b] and zeros in the other pair; every other thread holds four zeros; each component is
summed over the block as clip_ref.block_sum (the owners are clip_ref.block_partials'). Pass 2: per component, thread j
adds the SEGMENT's partials j, j + 1024, ... and the block sums them: clip_ref.group_total over the segment's own
partials. w_norm = fl(sqrt(sum p2)), x_norm = fl(sqrt(sum x2)), then in float32
    LARS  ratio = fl(fl(trust_coef * wn) / fl(fl(gn + fl(wd * wn)) + eps))   where wn > 0 and gn > 0, else 1
    LAMB  ratio = fl(wn / un)                                                where wn > 0 and un > 0, else 1.

The bounds (derived, not measured). A norm: clip_ref.norm_bound at the tensor's partial count, the number of pass-1
blocks of its segment (zeros from blocks outside the tensor add nothing), relative. The ratio: write every float32 norm
as norm (1 + d), |d| <= its bound. LARS's numerator trust_coef * wn rounds once; the denominator is a sum of three
non-negative terms gn, fl(wd * wn) and eps, so its relative error is at most the largest term error, max(b_g, b_w + u),
plus one rounding per addition (2 u); the quotient rounds once:
    |ratio~ - ratio| / ratio <= (1 + b_w)(1 + u) (1 + u) / ((1 - max(b_g, b_w + u))(1 - u)^2) - 1
which is b_w + b_g + 5 u to first order (five float32 operations: two products, two additions, one division) and is
what lars_ratio_bound returns, evaluated exactly. LAMB's ratio is one division: (1 + b_w)(1 + u) / (1 - b_u) - 1.

LAMB's u is itself float32 arithmetic on the moments, so sum u^2 carries the elementwise error of u. With the standard
model fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-24, and g, m0, v0, p the float32 inputs (fused multiply-adds only
remove roundings):
    m1 = m0 + (1 - b1)(g - m0):   E_m <= u |m1| + 3.01 u (1 - b1) |g - m0|     (difference, factor, product; then the sum)
    v1 = v0 b2 + g g (1 - b2):    non-negative terms, four roundings deep: relative 4.1 u
    denom = sqrt(v1) / bc2s + eps: relative 4.1 u / 2 + u (sqrt) + u (bc2s rounded to float32) + u (division) + u (sum)
                                   <= 6.1 u
    c = m1 / denom:               E_c <= E_m / denom + 7.2 u |c|
    u = fl(c rbc1) + fl(wd p):    E_u <= rbc1 E_c + 2.01 u |c rbc1| + u |wd p| + u |u|
(lamb_u_error). Then |sum u~^2 - sum u^2| <= sum (2 |u| E_u + E_u^2) on top of the summation error of the float32
squares, which is clip_ref's gamma_k of the computed sum.
"""
from __future__ import annotations

import math

import numpy as np

import clip_ref as C

F32 = np.float32
U = C.U
N = C.N
NW_CASES = (1100, 1024, 1300, 1299)   # straddles a block in all three forms; on a boundary of all; no bias; 1 element


# ------------------------------------------------------------------------------------------ float32 emulation
def _block_sums(sq, nslab):
    """Per pass-1 block the clip_ref.block_sum of the owners' values `sq` (f32 [n]), the other threads 0."""
    sq = np.asarray(sq, dtype=F32)
    cols, nb = C.cols_per_block(nslab), C.nblk(sq.size, nslab)
    q = np.zeros((nb, 1024), dtype=F32)
    for b in range(nb):
        part = sq[b * cols:(b + 1) * cols]
        q[b, :part.size] = part
    return C.block_sum(q)


def partials(x, p, nslab, nw):
    """Pass 1's [nblk, 4] partials [x2_W, p2_W, x2_b, p2_b] of one segment (x: gradient or update direction)."""
    x, p = np.asarray(x, dtype=F32), np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        x2, p2 = (x * x).astype(F32), (p * p).astype(F32)
    w = np.arange(x.size) < nw
    zero = F32(0)
    comps = (np.where(w, x2, zero), np.where(w, p2, zero), np.where(w, zero, x2), np.where(w, zero, p2))
    with np.errstate(all="ignore"):
        return np.stack([_block_sums(c, nslab) for c in comps], axis=1)


def totals(parts):
    """Pass 2's four totals of one segment from its [nblk, 4] partials."""
    parts = np.asarray(parts, dtype=F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return [C.group_total(parts[:, k]) for k in range(4)]


def _sqrt32(t):
    with np.errstate(all="ignore"):
        return np.sqrt(F32(t)).astype(F32)


def lars_ratio32(sum_g2, sum_p2, trust_coef, wd, eps):
    """(w_norm, g_norm, ratio) in float32 as slk_lars_multi forms them."""
    wn, gn = _sqrt32(sum_p2), _sqrt32(sum_g2)
    with np.errstate(all="ignore"):
        num, dw = F32(F32(trust_coef) * wn), F32(F32(wd) * wn)
        r = F32(num / F32(F32(gn + dw) + F32(eps)))
    return wn, gn, (r if (wn > 0 and gn > 0) else F32(1))


def lamb_ratio32(sum_u2, sum_p2):
    wn, un = _sqrt32(sum_p2), _sqrt32(sum_u2)
    with np.errstate(all="ignore"):
        r = F32(wn / un)
    return wn, un, (r if (wn > 0 and un > 0) else F32(1))


# ------------------------------------------------------------------------------------------ float64 closed forms
def norm64(a):
    return math.sqrt(float((np.asarray(a, dtype=np.float64) ** 2).sum()))


def lars_ratio64(wn, gn, trust_coef, wd, eps):
    """The paper's local rate (timm Lars, trust_clip=False); 1 where a norm is zero or NaN (the compare fails)."""
    if wn > 0 and gn > 0:
        return float(trust_coef) * wn / (gn + float(wd) * wn + float(eps))
    return 1.0


def lamb_ratio64(wn, un):
    return wn / un if (wn > 0 and un > 0) else 1.0


def tensors(n, nw):
    """The (slice, is_bias) of the non-empty tensors of one segment."""
    return [(s, b) for s, b in ((slice(0, nw), False), (slice(nw, n), True)) if s.stop > s.start]


def lars_step64(p, g, buf, step, lr, nw, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0,
                trust_coef=1e-3, eps=1e-8, exclude_bias=True, ratios=None, variant=None):
    """One LARS step of one segment in float64 from (p, g, buf) before it. Returns (p, buf, [(w_norm, g_norm, ratio)
    of the weight, of the bias]). `ratios` = (weight's, bias's) replaces the computed ratios (the device's).
    `variant` builds a WRONG recipe: "decayed_norm" takes the ratio from |g + wd w|, "bias_in_weight" takes the
    weight's norms over the whole segment, "ratio_after_momentum" scales the momentum's output instead of its input."""
    p, g, buf = (np.array(a, dtype=np.float64) for a in (p, g, buf))
    newp, newb, rows = p.copy(), buf.copy(), []
    for k, (s, is_bias) in enumerate(tensors(p.size, nw)):
        excl = is_bias and exclude_bias
        wd = 0.0 if excl else float(weight_decay)
        sn = slice(0, p.size) if (variant == "bias_in_weight" and not is_bias) else s
        wn = norm64(p[sn])
        gn = norm64(g[sn] + wd * p[sn]) if variant == "decayed_norm" else norm64(g[sn])
        r = lars_ratio64(wn, gn, trust_coef, wd, eps)
        if excl:
            r = 1.0
        elif ratios is not None:
            r = float(ratios[1 if is_bias else 0])
        rows.append((wn, gn, r))
        d = g[s] + wd * p[s]
        if variant != "ratio_after_momentum":
            d = r * d
        if momentum != 0:
            b = d.copy() if step == 0 else momentum * buf[s] + (1.0 - dampening) * d
            newb[s] = b
            d = d + momentum * b if nesterov else b
        if variant == "ratio_after_momentum":
            d = r * d
        newp[s] = p[s] - lr * d
    return newp, newb, rows


def lamb_direction64(g, m, v, p, step, b1, b2, eps, wd):
    """(u, m1, v1) in float64: u = m-hat / (sqrt(v-hat) + eps) + wd p after the moments have moved."""
    g, m, v, p = (np.asarray(a, dtype=np.float64) for a in (g, m, v, p))
    t = step + 1
    m1 = m + (1.0 - b1) * (g - m)
    v1 = v * b2 + g * g * (1.0 - b2)
    denom = np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
    return (m1 / denom) / (1.0 - b1 ** t) + wd * p, m1, v1


def lamb_step64(p, g, m, v, step, lr, nw, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, exclude_bias=True,
                ratios=None):
    """One LAMB step of one segment in float64. Returns (p, m, v, [(w_norm, u_norm, ratio) per tensor])."""
    p = np.array(p, dtype=np.float64)
    newp, rows = p.copy(), []
    u0, m1, v1 = lamb_direction64(g, m, v, p, step, beta1, beta2, eps, 0.0)
    for s, is_bias in tensors(p.size, nw):
        excl = is_bias and exclude_bias
        u = u0[s] + (0.0 if excl else float(weight_decay)) * p[s]
        wn, un = norm64(p[s]), norm64(u)
        r = lamb_ratio64(wn, un)
        if excl:
            r = 1.0
        elif ratios is not None:
            r = float(ratios[1 if is_bias else 0])
        rows.append((wn, un, r))
        newp[s] = p[s] - lr * r * u
    return newp, m1, v1, rows


# ------------------------------------------------------------------------------------------ bounds
def norm_bound(npart, ref_terms=0):
    """Relative bound of a tensor's float32 norm: clip_ref.norm_bound at its segment's partial count."""
    return C.norm_bound(npart, ref_terms)


def lars_ratio_bound(npart, ref_terms=0):
    """Relative bound of LARS's float32 ratio against float64 (module docstring)."""
    b = norm_bound(npart, ref_terms)   # both norms of a tensor have the same partial count
    return (1 + b) * (1 + U) * (1 + U) / ((1 - (b + U)) * (1 - U) ** 2) - 1


def lamb_ratio_bound(npart, u_bound, ref_terms=0):
    """Relative bound of LAMB's float32 ratio: w_norm by norm_bound, u_norm by `u_bound` (lamb_unorm_bound)."""
    return (1 + norm_bound(npart, ref_terms)) * (1 + U) / (1 - u_bound) - 1


def lamb_u_error(g, m, v, p, step, b1, b2, eps, wd):
    """(u in float64, the elementwise absolute bound E_u of the float32 u) from the float32 inputs (docstring)."""
    g, m, v, p = (np.asarray(a, dtype=np.float64) for a in (g, m, v, p))
    t = step + 1
    u, m1, v1 = lamb_direction64(g, m, v, p, step, b1, b2, eps, wd)
    rbc1 = 1.0 / (1.0 - b1 ** t)
    denom = np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
    e_m = U * np.abs(m1) + 3.01 * U * (1.0 - b1) * np.abs(g - m)
    c = m1 / denom
    e_c = e_m / denom + 7.2 * U * np.abs(c)
    e_u = rbc1 * e_c + 2.01 * U * np.abs(c * rbc1) + U * np.abs(wd * p) + U * np.abs(u)
    return u, e_u


def sumsq_bound(u, e_u, chain):
    """Absolute bound of a float32 sum of squares of u~ (|u~ - u| <= e_u) against sum u^2, `chain` roundings deep."""
    u, e_u = np.abs(np.asarray(u, dtype=np.float64)), np.asarray(e_u, dtype=np.float64)
    s = float(((u + e_u) ** 2).sum())
    return C.gamma(chain) * s + float((2 * u * e_u + e_u * e_u).sum())


def lamb_unorm_bound(npart, u, e_u, ref_terms=0):
    """Relative bound of LAMB's float32 u_norm over one tensor: the summation bound of clip_ref plus u's own error
    (sqrt halves a relative error of the sum and rounds once)."""
    s = float((np.asarray(u, dtype=np.float64) ** 2).sum())
    if s == 0.0:
        return 0.0
    rel = sumsq_bound(u, e_u, C.chain_length(npart)) / s
    return (1.0 + rel / 2.0) * (1.0 + U) - 1.0 + ref_terms * 2.0 ** -53


# ------------------------------------------------------------------------------------------ the op tests' inputs
_PARAMS = {}


def params_case(i):
    """Segment i's parameters before the first step (f32 [N], read-only), seeded per segment: N(0, 1000^2), the size of
    the op tests' gradients (R.reduce_case sums, ~800 per element), so that weight_decay * w is visible next to g
    (with small weights a ratio taken from the decayed gradient's norm would pass every bound)."""
    if i not in _PARAMS:
        _PARAMS[i] = (np.random.default_rng(9100 + i).standard_normal(N) * 1e3).astype(F32)
        _PARAMS[i].setflags(write=False)
    return _PARAMS[i]


def state_case(i):
    """A non-zero momentum buffer / first moment for segment i (f32 [N], read-only)."""
    key = ("s", i)
    if key not in _PARAMS:
        _PARAMS[key] = (np.random.default_rng(9200 + i).standard_normal(N) * 0.05).astype(F32)
        _PARAMS[key].setflags(write=False)
    return _PARAMS[key]
