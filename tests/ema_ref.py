"""The exponential moving average of the parameters (slk_ema_multi, optim.EMA): a float64 closed form of the rule, numpy
float32 evaluations of it in the order include/slk.h documents, and the derived single-update error bound. Test
infrastructure only (tests/test_ema_cpu.py pins it on the CPU; tests/test_ema_gpu.py and tests/test_ema_trainer_gpu.py
use it on the GPU).

The rule. k = the stage's step counter before its tick, t = k - start:
    t <  0:  e' = p                                      (a copy of the bits)
    t >= 0:  n = t + 1;  d = warmup ? min(decay, (1 + n) / (10 + n)) : decay;  e' = e + (1 - d)(p - e)
with `decay` the float32 value the device holds. The closed form (step64) evaluates this in float64 from the float32
inputs: its own error is a few 2^-53 relative, five orders below the bound.

The float32 order (include/slk.h): nf = fl(n) (nearest even), w = fl(fl(1 + nf) / fl(10 + nf)), d = min(decay, w),
omd = fl(1 - d), diff = fl(p - e), e' = fma(omd, diff, e) (one rounding), or unfused fl(e + fl(omd * diff)).

The bound (derived, not measured), with the standard model fl(a op b) = (a op b)(1 + x), |x| <= u = 2^-24:
    A, the absolute error of omd against 1 - d:
      without warm-up d is the float32 decay itself and fl(1 - d) rounds once a value in (0, 1]:   A <= u / 2.
      with warm-up and n + 10 <= 2^24, nf, 1 + nf and 10 + nf are exact integers and the quotient w < 1 rounds once,
      |w - (1 + n) / (10 + n)| <= u / 2; min() is 1-Lipschitz, so |d - d*| <= u / 2, and fl(1 - d) adds u / 2:
      A <= u. A_SMALL = 1.5 u is used, half a unit of margin over this count.
      with n + 10 > 2^24, nf, the numerator and the denominator each carry a relative u, the quotient one more:
      |w - w*| <= (3 u + O(u^2)) w* + u / 2 < 4 u; with fl(1 - d):  A_LARGE = 4.5 u.
    diff = (p - e)(1 + x1); the product omd * diff is rounded (unfused, x2) or not (fused); so against (1 - d*)(p - e)
      T = |p - e| (A + (1 - d* + A)((1 + u)^2 - 1))
    and the sum rounds once, relative u of the computed sum, itself within T of the exact e'*:
      bound = T + u (|e'*| + T) + 3 * 2^-149     (the last term: gradual underflow of the three operations)
    To first order, with |e'*| <= max(|p|, |e|) and |p - e| <= |p| + |e|: (1.5 u + 2 u)(|p| + |e|) + u max(|p|, |e|)
    <= 4.5 u (|p| + |e|). Fused multiply-adds only remove roundings. bound() evaluates the exact
    expression above, not the first-order one.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U = 2.0 ** -24
A_SMALL = 1.5 * U     # n + 10 <= 2^24 (and no warm-up)
A_LARGE = 4.5 * U     # n + 10 >  2^24 under warm-up
TINY = 3 * 2.0 ** -149
DECAYS = (0.0, 0.9, 0.9999, float(np.nextafter(F32(1), F32(0))))   # the last: the largest float32 below 1
VARIANTS = (None, "n_is_t", "swapped", "start_off_by_one")          # None: the rule; the others deliberately wrong


def rate64(k: int, start: int, decay, warmup: bool, variant=None):
    """(copy, d) of step k in exact / float64 arithmetic; decay is taken as the float32 value the device holds."""
    d = float(F32(decay))
    first = start + 1 if variant == "start_off_by_one" else start
    t = int(k) - first
    if t < 0:
        return True, d
    n = t if variant == "n_is_t" else t + 1
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return False, d


def step64(e, p, k: int, start: int, decay, warmup: bool, variant=None):
    """The closed form: e' in float64 from the float32 blocks e and p (a copy of p, as float64, while k < start)."""
    e64, p64 = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    copy, d = rate64(k, start, decay, warmup, variant)
    if copy:
        return p64.copy()
    if variant == "swapped":
        return e64 + d * (p64 - e64)
    return e64 + (1.0 - d) * (p64 - e64)


def step32(e, p, k: int, start: int, decay, warmup: bool, fused: bool = False):
    """The rule in float32 in the documented order. fused: product and sum as one operation (the product of two
    float32 is exact in float64; the float64 sum is then rounded to float32)."""
    e, p = np.asarray(e, dtype=F32), np.asarray(p, dtype=F32)
    t = int(k) - int(start)
    if t < 0:
        return p.copy()
    d = F32(decay)
    if warmup:
        nf = F32(t + 1)
        w = F32(F32(1) + nf) / F32(F32(10) + nf)
        d = w if w < d else d
    omd = F32(F32(1) - d)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (p - e).astype(F32)
        if fused:
            return (np.float64(omd) * diff.astype(np.float64) + e.astype(np.float64)).astype(F32)
        return (e + (omd * diff).astype(F32)).astype(F32)


def bound(e, p, k: int, start: int, decay, warmup: bool):
    """Elementwise bound on |float32 result - step64| for one update from the float32 blocks e and p (0 for a copy)."""
    e64, p64 = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    copy, d = rate64(k, start, decay, warmup)
    if copy:
        return np.zeros_like(e64)
    n = int(k) - int(start) + 1
    A = A_LARGE if (warmup and n + 10 > 2 ** 24) else A_SMALL
    T = np.abs(p64 - e64) * (A + (1.0 - d + A) * ((1.0 + U) ** 2 - 1.0))
    exact = e64 + (1.0 - d) * (p64 - e64)
    return T + U * (np.abs(exact) + T) + TINY


def within(got, e, p, k, start, decay, warmup):
    """Whether every finite element of `got` (float32) lies within bound() of the closed form; non-finite elements of
    the closed form must be non-finite alike (NaN for NaN, the same infinity)."""
    got = np.asarray(got, dtype=np.float64)
    want = step64(e, p, k, start, decay, warmup)
    fin = np.isfinite(want)
    ok = np.abs(got[fin] - want[fin]) <= bound(e, p, k, start, decay, warmup)[fin]
    same = np.array_equal(got[~fin], want[~fin], equal_nan=True)
    return bool(ok.all()) and same
