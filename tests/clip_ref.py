"""Global-norm gradient clipping (slk_reduce_sqnorm_multi -> slk_sgdm_clip_multi / slk_adamw_clip_multi): numpy
float32 emulations of the two summation orders include/slk.h documents, a float64 reference and the derived error
bound. Test infrastructure only (tests/test_clip_ref_cpu.py pins it on the CPU; tests/test_clip_gpu.py and
tests/test_clip_trainer_gpu.py use it on the GPU).

The orders. Pass 1, one block of 1024 threads: the thread that owns a column holds q = fl(g * g), every other thread 0
(thread = column in the 1024-column form, threads 0..255 in the 256-column form, threads 0..63 in the 64-column
form); inside each of the 16 waves the 64 values are added as a balanced tree over neighbouring lanes; the 16 wave
sums are added in ascending wave order. Pass 2: thread j adds its group's partials j, j + 1024, ... ascending from 0,
then the same block sum. norm = fl(sqrt(total)); coef = fl(max_norm / fl(norm + 1e-6f)), 1 where that exceeds 1.

The bound (derived, not measured). Every term of sum g^2 is rounded once when squared and then passes through a
chain of float32 additions: 6 (tree) + 15 (waves) in pass 1, ceil(npart / 1024) (the thread's own partials, the
first one added to 0) + 6 + 15 in pass 2. With k = 1 + 21 + ceil(npart / 1024) + 21 roundings on the longest path
and only non-negative terms, the computed sum S~ satisfies |S~ - S| <= gamma_k S, gamma_k = k u / (1 - k u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any summation order, k the deepest
path). sqrt halves a relative error (sqrt(1 + d) <= 1 + d / 2) and rounds once more:
    |norm~ - norm| <= ((1 + gamma_k / 2)(1 + u) - 1) norm.
For the op tests (n = 1300 columns: 2 + 6 and 21 partials in the two groups) k = 44 and the bound is
1.37e-6 relative; a float64 reference adds its own n 2^-53, which norm_bound takes as `ref_terms`.
"""
from __future__ import annotations

import math

import numpy as np

import head_ref64 as R

F32 = np.float32
U = 2.0 ** -24
N = 1300                       # columns of every op-test segment: a partial last block in all three forms
SLAB_COUNTS = (1, 17, 65)      # one segment per reduction form (1024, 256 and 64 columns per block)
GROUPS = ((0, 1), (2,))        # the op tests' two groups: segments {0, 1} and {2}
PAD = 64


# ---------------------------------------------------------------------------------------------- the two orders
def wave_sum(v):
    """[..., 64] -> [...]: the butterfly of csrc/slk_common.h wave_sum = a balanced tree over neighbouring lanes."""
    v = np.asarray(v, dtype=F32)
    assert v.shape[-1] == 64
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    return v[..., 0]


def block_sum(v):
    """[..., 1024] -> [...]: wave_sum per wave, then the 16 wave sums in ascending wave order."""
    w = wave_sum(np.asarray(v, dtype=F32).reshape(v.shape[:-1] + (16, 64)))
    t = w[..., 0]
    for k in range(1, 16):
        t = (t + w[..., k]).astype(F32)
    return t


def cols_per_block(nslab):
    return {1: 1024, 4: 256, 16: 64}[R.reduce_form(nslab)]


def nblk(n, nslab):
    return -(-n // cols_per_block(nslab))


def block_partials(grad, nslab):
    """Pass 1's partials of one segment whose reduced gradient is `grad` (f32 [n]) summed from nslab slabs."""
    g = np.asarray(grad, dtype=F32)
    cols = cols_per_block(nslab)
    nb = nblk(g.size, nslab)
    q = np.zeros((nb, 1024), dtype=F32)
    sq = (g * g).astype(F32)
    for b in range(nb):
        part = sq[b * cols:(b + 1) * cols]
        q[b, :part.size] = part        # threads 0 .. cols-1 own the block's columns, the rest hold 0
    return block_sum(q)


def group_total(partials):
    """Pass 2's total of one group's partials (all its segments' partials, concatenated in segment order)."""
    p = np.asarray(partials, dtype=F32).reshape(-1)
    s = np.zeros(1024, dtype=F32)
    for j0 in range(0, p.size, 1024):
        chunk = p[j0:j0 + 1024]
        s[:chunk.size] = (s[:chunk.size] + chunk).astype(F32)
    return block_sum(s)


def norm_coef(total, max_norm):
    """(norm, coef) in float32 from a group's total, as the kernels form them (a NaN norm keeps a NaN coef)."""
    with np.errstate(all="ignore"):
        norm = np.sqrt(F32(total)).astype(F32)
        coef = F32(F32(max_norm) / F32(norm + F32(1e-6)))
    return norm, (F32(1.0) if coef > 1 else coef)


def emulate(grads, nslabs, max_norm):
    """One group: (partials concatenated, norm, coef) from its segments' gradients and slab counts."""
    parts = np.concatenate([block_partials(g, k) for g, k in zip(grads, nslabs)])
    norm, coef = norm_coef(group_total(parts), max_norm)
    return parts, norm, coef


# ---------------------------------------------------------------------------------------------- reference, bound
def norm64(grads):
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads))


def coef64(norm, max_norm):
    """torch's clip coefficient in float64 from a given norm: min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def chain_length(npart):
    """k of the module docstring for a group of npart partials."""
    return 1 + 21 + -(-int(npart) // 1024) + 21


def gamma(k):
    return k * U / (1.0 - k * U)


def norm_bound(npart, ref_terms=0):
    """Relative bound of the float32 norm against the exact one (+ ref_terms 2^-53 for a float64 reference)."""
    return (1.0 + gamma(chain_length(npart)) / 2.0) * (1.0 + U) - 1.0 + ref_terms * 2.0 ** -53


def plain_ascending_sumsq(grads):
    """sum g^2 added in ascending order in float32: NOT what the kernels do."""
    q = np.concatenate([(np.asarray(g, dtype=F32) ** 2).astype(F32) for g in grads])
    return np.cumsum(q, dtype=F32)[-1]


def ulps(a, b):
    """Distance of two finite float32 values in units in the last place."""
    ia, ib = (int(np.asarray(x, dtype=F32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


# ---------------------------------------------------------------------------------------------- the op tests' inputs
_CASES = {}


def case(i):
    """Segment i of the op tests: (slabs [SLAB_COUNTS[i], N] as R.reduce_case, its emulated reduced gradient)."""
    if i not in _CASES:
        s = R.reduce_case(SLAB_COUNTS[i], N, 7000 + SLAB_COUNTS[i])
        _CASES[i] = (s, R.reduce_emulated(s))
        for a in _CASES[i]:
            a.setflags(write=False)
    return _CASES[i]


def group_case(g, max_norm=np.inf):
    """Group g of GROUPS: (partials, norm, coef) emulated from its segments."""
    ids = GROUPS[g]
    return emulate([case(i)[1] for i in ids], [SLAB_COUNTS[i] for i in ids], max_norm)
