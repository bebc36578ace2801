"""TEST INFRASTRUCTURE: the soft-target cross-entropy (label smoothing + mixed labels) in float64, its float32
error bounds, and a float32 numpy emulation of the expression include/slk.h documents.

Reference (closed form, float64, max-subtracted like head_ref64.xent64), C = 10:
    t_j   = (1 - eps) ((j == a) (1 - wb) + (j == b) wb) + eps / C
    loss  = sum_{t_j != 0} t_j (lse - z_j),        dlogits_j = (softmax(z)_j - t_j) grad_scale
torch's probability-target path agrees with it to ~4e-16; torch's class-index path with label_smoothing only to
~4e-8, so that path is NOT the reference.

Bounds. The kernels compute, in float32 (slk.h, "soft targets"):
    wa = fl(1 - wb); keep = fl(1 - eps); flat = fl(eps / 10)
    u_j = (j == a ? wa : 0) + (j == b ? wb : 0);   t_j = fmaf(keep, u_j, flat)
    S = fmaf(t_j, z_j, S) over ascending j with t_j != 0;   loss = fl(lse - S);   g_j = fl(fl(p_j - t_j) gs)
head_ref64.loss_bound / grad_bound already cover lse = fl(m + log se), the final subtraction from lse of a value
below max|z|, p_j = exp(z_j - lse) and the two roundings of (p_j - t_j) gs. What is new is the error of t_j and of S.
Each float32 rounding contributes at most 2^-24 of the magnitude it rounds (first order; second-order terms are
2^-24 of these). Roundings that can be inexact, per class j:
    fl(1 - wb)            1 on class a                   when 0 < wb < 1                  (value <= 1)
    wa + wb               1 on class a == b              when 0 < wb < 1                  (value <= 1)
    fl(1 - eps)           1 on classes with u_j != 0     when 0 < eps < 1                 (keep u_j <= 1)
    fmaf(keep, u_j, flat) 1 on classes with u_j != 0     when eps > 0                     (t_j <= 1; with u_j = 0 the
                                                                                           fmaf returns flat exactly,
                                                                                           with eps = 0 it returns u_j)
    fl(eps / 10)          1 on every class               when eps > 0                     (value <= 0.1)
so |dt_j| <= 2^-24 nt_j with nt_j = (the count of the first four) + 0.1 (the fifth)         -> t_terms().
    S: one fmaf per class with t_j != 0, each rounding a partial sum of magnitude <= A = sum_j t_j |z_j| <= max|z|;
       none is inexact when eps = 0 and wb in {0, 1} (t is exactly one-hot, S = 1 * z_a)    -> nS roundings.
Hence
    soft_loss_bound = loss_bound + 2^-24 (nS A + sum_j nt_j |z_j|)        (dt_j reaches the loss through t_j z_j)
    soft_grad_bound = grad_bound + grad_scale 2^-24 nt_j                  (the magnitude rounded is t_j <= 1)
    soft_gradsum_bound = gradsum_bound + grad_scale 2^-24 sum_j nt_j      (the float32 t_j sum to 1 only that well)
At eps = 0, wb = 0 every count is 0 and the bounds ARE head_ref64's.
"""
import numpy as np

import head_ref64 as R

C = 10
EPS24 = 2.0 ** -24


def unpack_np(y):
    y = np.asarray(y, dtype=np.int64)
    wb = (y >> 32).astype(np.int32).view(np.float32) if y.ndim else np.int32(y >> 32).view(np.float32)
    return y & 0xFF, (y >> 8) & 0xFF, wb


def pack_np(a, b, wb):
    bits = np.asarray(wb, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.asarray(a, dtype=np.int64) | (np.asarray(b, dtype=np.int64) << 8) | (bits << 32)


def targets64(y, eps):
    """t [B,10] float64 of packed targets y."""
    a, b, wb = unpack_np(y)
    wb = wb.astype(np.float64)
    B = a.shape[0]
    u = np.zeros((B, C))
    u[np.arange(B), a] += 1.0 - wb
    u[np.arange(B), b] += wb
    return (1.0 - eps) * u + eps / C


def soft_xent64(z, y, eps, grad_scale=1.0):
    """(loss_i [B], dlogits [B,10], softmax p [B,10], t [B,10]) in float64 from the closed form. -inf logits are
    allowed on classes whose t_j is exactly 0."""
    z = np.asarray(z, dtype=np.float64)
    t = targets64(y, eps)
    m = z.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        logp = z - lse
    p = np.exp(logp)
    loss = np.zeros(z.shape[0])
    for j in range(C):                       # ascending, zero-weight classes skipped (0 * -inf would be NaN)
        nz = t[:, j] != 0
        loss[nz] += t[nz, j] * -logp[nz, j]
    return loss, (p - t) * grad_scale, p, t


def t_terms(y, eps):
    """nt [B,10]: the float32 roundings behind each t_j, weighted by the magnitude they round (module docstring)."""
    a, b, wb = unpack_np(y)
    B = a.shape[0]
    frac = (wb > 0) & (wb < 1)
    u_nz = np.zeros((B, C), dtype=bool)
    u_nz[np.arange(B), a] |= wb < 1
    u_nz[np.arange(B), b] |= wb > 0
    nt = np.zeros((B, C))
    nt[np.arange(B), a] += frac * 1.0 + (frac & (a == b)) * 1.0
    nt += u_nz * (1.0 if 0 < eps < 1 else 0.0)
    nt += u_nz * (1.0 if eps > 0 else 0.0)
    nt += 0.1 if eps > 0 else 0.0
    return nt


def _absz(z):
    a = np.abs(np.asarray(z, dtype=np.float64))
    return np.where(np.isfinite(a), a, 0.0)


def soft_loss_bound(z, y, eps, loss64):
    a, b, wb = unpack_np(y)
    t = targets64(y, eps)
    az = _absz(z)
    exact = (eps == 0) & ((wb == 0) | (wb == 1))
    nS = np.where(exact, 0, (t != 0).sum(axis=1))
    A = (t * az).sum(axis=1)
    return R.loss_bound(z, loss64) + EPS24 * (nS * A + (t_terms(y, eps) * az).sum(axis=1))


def soft_grad_bound(z, y, eps, p64, grad_scale=1.0):
    return R.grad_bound(z, p64, grad_scale) + grad_scale * EPS24 * t_terms(y, eps)


def soft_gradsum_bound(z, y, eps, grad_scale=1.0):
    return R.gradsum_bound(z, grad_scale) + grad_scale * EPS24 * t_terms(y, eps).sum(axis=1)


# ---------------------------------------------------------------------------- float32 emulation of the kernels
F = np.float32


def _fma32(a, b, c):
    """fmaf for float32 inputs: the product of two float32 is exact in float64; one float64 addition, then the
    rounding to float32 (a double rounding is possible but moves the result by at most one more half ulp, far
    inside what this emulation is used for: staying within the bounds, not matching bits)."""
    return F(np.float64(a) * np.float64(b) + np.float64(c))


VARIANTS = (None, "spread_c_minus_1", "wb_to_a", "smooth_lse_only")


def emulate32(z, y, eps, grad_scale=1.0, variant=None):
    """(loss [B], dlogits [B,10]) float32 by the documented expression, row by row. `variant` names a wrong
    implementation: smoothing spread over C - 1 classes (the off-target ones get eps / 9, the targets none), wb
    given to class a, or the smoothing's flat part left out of the target (so it reaches the loss through lse
    only)."""
    z = np.asarray(z, dtype=np.float32)
    a_, b_, wb_ = unpack_np(y)
    B = z.shape[0]
    loss, dl = np.zeros(B, dtype=F), np.zeros((B, C), dtype=F)
    eps, gs = F(eps), F(grad_scale)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r in range(B):
            zr, a, b, wb = z[r], int(a_[r]), int(b_[r]), F(wb_[r])
            m = zr.max()
            se = F(0)
            for j in range(C):
                se = F(se + np.exp(F(zr[j] - m)))
            lse = F(m + np.log(se))
            wa, keep, flat = F(F(1) - wb), F(F(1) - eps), F(eps / F(10))
            if variant == "wb_to_a":
                wa, wb = wb, wa
            t = np.zeros(C, dtype=F)
            for j in range(C):
                u = F((wa if j == a else F(0)) + (wb if j == b else F(0)))
                if variant == "spread_c_minus_1":
                    t[j] = _fma32(keep, u, F(0)) if u != 0 else F(eps / F(9))
                elif variant == "smooth_lse_only":
                    t[j] = _fma32(keep, u, F(0))
                else:
                    t[j] = _fma32(keep, u, flat)
            S = F(0)
            for j in range(C):
                if t[j] != 0:
                    S = _fma32(t[j], zr[j], S)
            loss[r] = F(lse - S)
            for j in range(C):
                dl[r, j] = F(F(np.exp(F(zr[j] - lse)) - t[j]) * gs)
    return loss, dl


def mixed_cases(y_plain, wb, same=False, shift=3):
    """Packed targets from the plain labels of head_ref64.xent_batch: class a = the case's label, class b = a (same)
    or (a + shift) % 10, weight wb."""
    a = np.asarray(y_plain, dtype=np.int64)
    b = a if same else (a + shift) % C
    return pack_np(a, b, np.full(a.shape, wb, dtype=np.float32))
