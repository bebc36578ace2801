"""Test infrastructure: the n-class K5 head (include/slk.h, "The n-class head") restated in float64 numpy, and the
bounds tests/test_wide_headn_gpu.py holds the float32 kernels to. Everything here is in torch's flatten order
(feature = c * 64 + pix); `c8` / `flat` convert to and from the cut's C8 order.

Bounds (nothing here was tuned on a GPU's output). Operands are the same bf16 values on both sides, so only the
float32 arithmetic differs from float64:
  logits   z_j = fl(ks * S_j) + bf_j with S_j a float32 sum of n = 16384 exact products in some order: the order-free
           worst case is |S - S64| <= (n - 1) u sum|terms| (u = 2^-24), the product by ks and the bias addition add one
           rounding each, so  |z - z64| <= (n + 2) u (ks sum|m c wq| + |bf|) =: E_j  (the issue's bound).
  loss, dlogits  are held against the float64 cross-entropy of the kernel's OWN float32 logits, so the logits' error
           does not enter, with tests/head_ref64.py's loss_bound / grad_bound and nc in place of 10:
             |loss - loss64| <= 2^-23 (max|z| + ln nc) + (nc - 10)+ u + (2e-6 |loss64| + 1e-6)
             |dl - dl64|     <= gs (p64 (2^-22 (max|z| + ln nc) + (nc - 10)+ u) + 2e-7)
           The first term is the two float32 roundings of m + logf(se) and lse - z_y (each at most u of a value below
           max|z| + ln nc; twice that in the exponent of p = expf(z - lse)). The bar in brackets is the project's, set
           for a 10-term sum; the float32 sum of nc positive terms expf(z_j - m) in ascending j has relative error
           <= (nc - 1) u, so log(se) moves by (nc - 10) u more than the 10-class bar already covers. At nc = 10 both
           are head_ref64's bounds to the letter.
"""
import numpy as np
import torch

CUT_F, U = 16384, 2.0 ** -24


def c8(flat):
    """[..., 16384] torch order -> C8 order: index (plane * 64 + pix) * 8 + k holds feature (plane * 8 + k) * 64 + pix."""
    return np.ascontiguousarray(flat.reshape(*flat.shape[:-1], 32, 8, 64).swapaxes(-1, -2)).reshape(flat.shape)


def flat(c):
    return np.ascontiguousarray(c.reshape(*c.shape[:-1], 32, 64, 8).swapaxes(-1, -2)).reshape(c.shape)


def bf16(x):
    """Round float32-representable values to bf16 (nearest even), returned as float64."""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def logits(cut, wq, bf, keep, ks):
    """(z as the rule rounds it when S is exact: fl(fl(ks S) + bf), S in float64, sum|terms|)."""
    d = cut * keep
    S, A = d @ wq.T, np.abs(d) @ np.abs(wq).T
    z = (np.float32(ks) * S.astype(np.float32)).astype(np.float32) + bf.astype(np.float32)
    return z, S, A


def logits_bound(A, bf, ks):
    return (CUT_F + 2) * U * (ks * A + np.abs(bf)[None, :])


def xent(z, y, gs):
    """float64 (loss_i, dlogits, lse) of float64 logits z."""
    m = z.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]
    p = np.exp(z - lse[:, None])
    onehot = np.eye(z.shape[1])[y]
    return lse - z[np.arange(len(y)), y], (p - onehot) * gs, lse


def xent_bounds(z32, y, gs):
    """(loss64, dl64, loss bound, dlogits bound) of float32 logits z32 (the kernel's own), per the derivation above."""
    nc = z32.shape[1]
    z = z32.astype(np.float64)
    loss, dl, lse = xent(z, y, gs)
    span = np.abs(z).max(axis=1) + np.log(nc)
    extra = max(nc - 10, 0) * U
    p = np.exp(z - lse[:, None])
    return (loss, dl, 2.0 ** -23 * span + extra + 2e-6 * np.abs(loss) + 1e-6,
            gs * (p * (2.0 ** -22 * span + extra)[:, None] + 2e-7))


def backward(cut, wq, dlq, keep, ks, share=256):
    """(dcut float64 = the bf16 the rule stores, slabs float32 [ceil(B / share), nc * 16384 + nc]) for exact sums."""
    k32 = np.float32(ks)
    dcut = np.where(keep, bf16(k32 * (dlq @ wq).astype(np.float32)), 0.0)
    d = cut * keep
    rows = []
    for lo in range(0, cut.shape[0], share):
        g = dlq[lo:lo + share]
        rows.append(np.concatenate([(k32 * (g.T @ d[lo:lo + share]).astype(np.float32)).reshape(-1),
                                    g.sum(axis=0).astype(np.float32)]))
    return dcut, np.stack(rows).astype(np.float32)


def eval_ref(z, y):
    """numpy's (pred, loss_i float64 with NaN for a bad label, bad mask) of float32 logits z [B, nc]."""
    nc = z.shape[1]
    pred = np.argmax(z, axis=1)   # first maximum; NaN counts as the maximum
    bad = (y < 0) | (y >= nc)
    loss = xent(z.astype(np.float64), np.where(bad, 0, y), 1.0)[0]
    return pred, np.where(bad, np.nan, loss), bad
