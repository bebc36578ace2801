"""Soft targets for the fused steps: label smoothing and CutMix's mixed labels (include/slk.h "soft targets").

A step's target stays one int64 [B] tensor. A *mixed label* packs two classes and a weight,

    y = a | (b << 8) | (float32_bits(wb) << 32)        a, b in [0, 10), wb in [0, 1] the weight of class b

so the graph caches, `register_inputs` and the loaders' buffer rings carry it unchanged. A plain label is the case
b = 0, wb = 0; a mixed label with wb != 0 is >= 2^32, which the hard-label heads flag as out of range (a trainer
built without `loss=` raises from check_labels instead of training on class a).

    SoftCrossEntropy(label_smoothing)   the loss= of SplitTrainer / WideTrainer and their server stages
    CutMix(prob)                        the mix= of the resident loaders (one slk_image_batch_mix launch per batch)
    CutMix(alpha=...) / MixUp / Mix     lam ~ Beta(alpha, alpha), MixUp, and a per-sample switch between the two (one
                                        slk_image_batch_blend launch per batch)
    pack_mixed / unpack_mixed           torch tensors on any device
    draw_chain                          the hash chain every draw of the batch kernels comes from (numpy)
    cutmix_draws                        the host twin of the kernel's box draws (numpy, integers only)
    beta_quantiles / mix_tables         the 1024-entry quantile tables slk_image_batch_blend reads
    mix_draws                           the host twin of slk_image_batch_blend's draws
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

NUM_CLASSES = 10
# what check_labels raises with: the hard-label heads flag a label outside [0, 10) (a mixed label with wb != 0 is one),
# the soft heads a malformed target
LABEL_ERROR = ("splitcnn: a label was out of range [0, 10), or a mixed-label target was malformed (class >= 10, "
               "reserved bits set, weight outside [0, 1]); a mixed batch needs a trainer built with loss=")


@dataclass(frozen=True)
class SoftCrossEntropy:
    """Cross-entropy on mixed labels with label smoothing eps in [0, 1]: per row
    t_j = (1 - eps) ((j == a) (1 - wb) + (j == b) wb) + eps / 10, loss = logsumexp(z) - sum_j t_j z_j (mean over the
    batch), i.e. torch's cross_entropy(z, probs, label_smoothing=eps). `label_smoothing` is a constructor constant
    that reaches the kernel by value: a captured graph keeps it, and there is no setter. With 0.0 and plain labels
    the step is bit for bit the default one."""
    label_smoothing: float = 0.0

    def __post_init__(self):
        eps = float(self.label_smoothing)
        if not 0.0 <= eps <= 1.0:   # NaN fails both compares
            raise ValueError(f"SoftCrossEntropy: label_smoothing must be in [0, 1], got {self.label_smoothing}")


MIX_TABLE = 1024   # entries of a quantile table (the kernel indexes it with the top ten bits of a hash)


def _check_alpha(who, name, alpha):
    if not 0.1 <= float(alpha) <= 32.0:   # NaN fails both compares
        raise ValueError(f"{who}: {name} must be in [0.1, 32], got {alpha}")


def _check_prob(who, name, p):
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"{who}: {name} must be in [0, 1], got {p}")


@dataclass(frozen=True)
class CutMix:
    """CutMix (Yun et al. 2019) with lam ~ Beta(alpha, alpha): with probability `prob` a sample gets a box of its
    partner (the previous sample of the batch, cyclically) pasted in, and the label becomes the area-weighted pair.
    The box is keyed on (dataset index, epoch, seed) like the crop; `seed` is used only by a loader without `augment`
    (with one, the Augment's seed keys every draw). alpha = 1.0 (the paper's setting) is one slk_image_batch_mix launch
    with its integer draw of the side; any other alpha in [0.1, 32] draws sqrt(1 - lam) from a 1024-entry quantile
    table in slk_image_batch_blend (other boxes than alpha = 1.0's, the same apply draws and centres)."""
    prob: float = 1.0
    seed: int = 0
    alpha: float = 1.0

    def __post_init__(self):
        _check_prob("CutMix", "prob", self.prob)
        _check_alpha("CutMix", "alpha", self.alpha)


@dataclass(frozen=True)
class MixUp:
    """MixUp (Zhang et al. 2018): with probability `prob` a sample becomes (1 - lam) * itself + lam * its partner (the
    previous sample of the batch, cyclically), blended in float32 after ToTensor and before Normalize, with lam drawn
    per SAMPLE from a 1024-entry quantile table of Beta(alpha, alpha) (timm's mode="elem"; not one lam per batch);
    the label is the pair weighted lam. `seed` as in CutMix."""
    alpha: float = 1.0
    prob: float = 1.0
    seed: int = 0

    def __post_init__(self):
        _check_prob("MixUp", "prob", self.prob)
        _check_alpha("MixUp", "alpha", self.alpha)


@dataclass(frozen=True)
class Mix:
    """CutMix and MixUp in one batch: a sample is mixed with probability `prob`, and a mixed sample is CutMix with
    probability `switch`, else MixUp (timm's Mixup(mixup_alpha, cutmix_alpha, prob, switch_prob, mode="elem")), each
    with its own Beta parameter. `seed` as in CutMix."""
    cutmix_alpha: float = 1.0
    mixup_alpha: float = 1.0
    prob: float = 1.0
    switch: float = 0.5
    seed: int = 0

    def __post_init__(self):
        _check_prob("Mix", "prob", self.prob)
        _check_prob("Mix", "switch", self.switch)
        _check_alpha("Mix", "cutmix_alpha", self.cutmix_alpha)
        _check_alpha("Mix", "mixup_alpha", self.mixup_alpha)


MIX_TYPES = (CutMix, MixUp, Mix)


def check_mix(mix):
    """The `mix=` argument of a resident loader: None, CutMix, MixUp or Mix."""
    if mix is not None and not isinstance(mix, MIX_TYPES):
        raise TypeError("mix: expected splitcnn.loss.CutMix, splitcnn.loss.MixUp, splitcnn.loss.Mix or None, got "
                        f"{type(mix).__name__}")
    return mix


def check_loss(loss):
    """The `loss=` argument of a trainer or server stage: None (hard labels) or a SoftCrossEntropy."""
    if loss is not None and not isinstance(loss, SoftCrossEntropy):
        raise TypeError(f"loss: expected splitcnn.loss.SoftCrossEntropy or None, got {type(loss).__name__}")
    return loss


# ------------------------------------------------------------------------------------ mixed labels
def pack_mixed(a: torch.Tensor, b: torch.Tensor, wb: torch.Tensor) -> torch.Tensor:
    """int64 mixed labels from classes a, b (integer tensors in [0, 10)) and the weight wb of b (float in [0, 1],
    rounded to float32). No validation beyond dtype: the soft heads validate every target on the device."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    wb = torch.as_tensor(wb, device=a.device)
    bits = wb.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return a.to(torch.int64) | (b.to(torch.int64) << 8) | (bits << 32)


def unpack_mixed(y: torch.Tensor):
    """(a, b, wb) of int64 mixed labels: int64, int64, float32. A plain label unpacks to (a, 0, 0.0)."""
    y = torch.as_tensor(y).to(torch.int64)
    wb = (y >> 32).to(torch.int32).contiguous().view(torch.float32)
    return y & 0xFF, (y >> 8) & 0xFF, wb


def soft_targets(y: torch.Tensor, label_smoothing: float = 0.0, dtype=torch.float64) -> torch.Tensor:
    """The [B, 10] target distribution of mixed labels y under label smoothing (for references and host-side checks)."""
    a, b, wb = unpack_mixed(y)
    wb = wb.to(dtype)
    t = torch.zeros((y.shape[0], NUM_CLASSES), dtype=dtype, device=y.device)
    t.scatter_add_(1, a.view(-1, 1), (1 - wb).view(-1, 1))
    t.scatter_add_(1, b.view(-1, 1), wb.view(-1, 1))
    return (1.0 - label_smoothing) * t + label_smoothing / NUM_CLASSES


# ------------------------------------------------------------------------------------ the kernels' draws (host twins)
def _lowbias32(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def draw_chain(idx, epoch: int, seed: int, n: int):
    """[h0, ..., h(n-1)]: the first n links of the hash chain the batch kernels key on (dataset index, epoch, seed)
    (include/slk.h), as uint32 arrays shaped like `idx`. h0..h2 are the crop and the flip, h3..h7 the mixing draws."""
    i = np.asarray(idx).astype(np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        hs = [_lowbias32(i * np.uint32(0x9E3779B1) + np.uint32(epoch & 0xFFFFFFFF) * np.uint32(0x85EBCA77)
                         + np.uint32(seed & 0xFFFFFFFF) * np.uint32(0xC2B2AE3D))]
        while len(hs) < n:
            hs.append(_lowbias32(hs[-1] + np.uint32(0x9E3779B9)))
    return hs


def _scaled(h, n):
    """(h * n) >> 32 in uint64, as int64: a 32-bit hash as a uniform draw from [0, n)."""
    return ((h.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _box(cy, cx, half, H, W):
    """(y1, y2, x1, x2): the box of half-side `half` centred on (cy, cx), clipped to the image."""
    return np.clip(cy - half, 0, H), np.clip(cy + half, 0, H), np.clip(cx - half, 0, W), np.clip(cx + half, 0, W)


def _below(h, p):
    """h < p * 2^32, the kernels' test of a draw against a probability."""
    return h.astype(np.uint64) < np.uint64(int(float(p) * 4294967296.0))


def cutmix_draws(idx, epoch: int, seed: int, H: int, W: int, prob: float = 1.0):
    """(apply, y1, y2, x1, x2, wb): the box slk_image_batch_mix pastes into the samples with dataset indices `idx` in
    `epoch` under `seed` (include/slk.h), in uint32 / uint64 numpy arithmetic. apply is bool; the box is rows
    [y1, y2) x columns [x1, x2) (int64, reported also where apply is False); wb is the float32 label weight of the
    partner, area / (H * W) where applied and 0 elsewhere."""
    h3, h4, h5, h6, h7 = draw_chain(idx, epoch, seed, 8)[3:]
    apply = _below(h3, prob)
    y1, y2, x1, x2 = _box(_scaled(h6, H), _scaled(h7, W), np.maximum(_scaled(h4, H), _scaled(h5, H)) // 2, H, W)
    area = np.where(apply, (y2 - y1) * (x2 - x1), 0)
    return apply, y1, y2, x1, x2, area.astype(np.float32) / np.float32(H * W)


# ------------------------------------------------------------------------------------ Beta(alpha, alpha) tables
def _betainc_sym(a: float, x: np.ndarray) -> np.ndarray:
    """The regularized incomplete beta I_x(a, a) for x in [0, 1/2] (float64), by the continued fraction (modified
    Lentz), which converges fast below the mean."""
    x = np.asarray(x, dtype=np.float64)
    tiny = 1e-300
    qab, qap, qam = 2.0 * a, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    for m in range(1, 400):
        m2 = 2 * m
        for aa in (m * (a - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
            c = 1.0 + aa / c
            c = np.where(np.abs(c) < tiny, tiny, c)
            delta = d * c
            h = h * delta
        if np.all(np.abs(delta - 1.0) < 3e-16):
            break
    with np.errstate(divide="ignore"):
        front = np.exp(a * (np.log(x) + np.log1p(-x)) + math.lgamma(2.0 * a) - 2.0 * math.lgamma(a))
    return np.where(x > 0, front * h / a, 0.0)


def beta_quantiles(alpha: float, n: int = MIX_TABLE) -> np.ndarray:
    """float64 [n]: the quantiles of Beta(alpha, alpha) at (k + 0.5) / n, by bisection on the regularized incomplete
    beta (no scipy). Only the lower half is solved; the upper is 1 - it, so q(1 - u) = 1 - q(u) holds exactly."""
    _check_alpha("beta_quantiles", "alpha", alpha)
    n = int(n)
    if n < 1:
        raise ValueError(f"beta_quantiles: n must be positive, got {n}")
    a = float(alpha)
    u = (np.arange(n // 2, dtype=np.float64) + 0.5) / n
    lo, hi = np.zeros_like(u), np.full_like(u, 0.5)
    for _ in range(1200):                      # down to the denormals at alpha = 0.1, then 53 bits
        mid = 0.5 * (lo + hi)
        if np.all((mid == lo) | (mid == hi)):
            break
        below = _betainc_sym(a, mid) < u
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    low = np.maximum.accumulate(0.5 * (lo + hi))
    q = np.empty(n, dtype=np.float64)
    q[:n // 2] = low
    q[n - n // 2:] = 1.0 - low[::-1]
    if n % 2:
        q[n // 2] = 0.5
    return q


def lam_table(alpha: float) -> np.ndarray:
    """float32 [1024]: MixUp's partner weights, the quantiles of Beta(alpha, alpha) rounded to float32."""
    return beta_quantiles(alpha, MIX_TABLE).astype(np.float32)


def cut_table(alpha: float) -> np.ndarray:
    """uint32 [1024]: CutMix's box side ratio sqrt(1 - lam) at the same quantiles as a 32-bit fraction,
    min(floor(sqrt(1 - q) * 2^32), 2^32 - 1), so that side = (entry * H) >> 32 like the kernel's other draws."""
    r = np.floor(np.sqrt(1.0 - beta_quantiles(alpha, MIX_TABLE)) * 4294967296.0)
    return np.minimum(r, 4294967295.0).astype(np.uint64).astype(np.uint32)


def mix_tables(mix, device):
    """(cut_table, lam_table) device tensors for a loader's `mix` (int32 holding the uint32 bits, float32), None for
    a table the mix does not use; CutMix(alpha=1.0) uses none (slk_image_batch_mix)."""
    check_mix(mix)

    def up(arr, view):
        return torch.from_numpy(np.ascontiguousarray(arr).view(view)).to(device)

    if isinstance(mix, CutMix):
        return (None, None) if float(mix.alpha) == 1.0 else (up(cut_table(mix.alpha), np.int32), None)
    if isinstance(mix, MixUp):
        return None, up(lam_table(mix.alpha), np.float32)
    if isinstance(mix, Mix):
        return up(cut_table(mix.cutmix_alpha), np.int32), up(lam_table(mix.mixup_alpha), np.float32)
    return None, None


def mix_draws(idx, epoch: int, seed: int, H: int, W: int, prob: float = 1.0, switch: float = 0.5, cut_table=None,
              lam_table=None):
    """(apply, cut, k, y1, y2, x1, x2, wb): slk_image_batch_blend's draws for the dataset indices `idx` (include/slk.h),
    in uint32 / uint64 numpy arithmetic. apply and cut are bool (cut as the rule defines it, whether or not the sample
    is applied); k is the table index; the box is rows [y1, y2) x columns [x1, x2) (int64; of side 0 where the sample
    is not a CutMix one); wb is the float32 label weight of the partner: area / (H * W) for an applied CutMix sample,
    lam_table[k] for an applied MixUp sample, 0 elsewhere."""
    if cut_table is None and lam_table is None:
        raise ValueError("mix_draws: needs cut_table, lam_table or both")
    h3, h4, h5, h6, h7 = draw_chain(idx, epoch, seed, 8)[3:]
    apply = _below(h3, prob)
    if cut_table is not None and lam_table is not None:
        cut = _below(h4, switch)
    else:
        cut = np.full(h3.shape, cut_table is not None)
    k = (h5 >> np.uint32(22)).astype(np.int64)
    side = np.zeros(h3.shape, dtype=np.int64)
    if cut_table is not None:
        side = np.where(cut, _scaled(np.asarray(cut_table).view(np.uint32)[k], H), 0)
    y1, y2, x1, x2 = _box(_scaled(h6, H), _scaled(h7, W), side // 2, H, W)
    area = np.where(apply & cut, (y2 - y1) * (x2 - x1), 0)
    wb = area.astype(np.float32) / np.float32(H * W)
    if lam_table is not None:
        wb = np.where(apply & ~cut, np.asarray(lam_table, dtype=np.float32)[k], wb).astype(np.float32)
    return apply, cut, k, y1, y2, x1, x2, wb
