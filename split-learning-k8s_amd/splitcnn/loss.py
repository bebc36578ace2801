"""Soft targets for the fused steps: label smoothing and CutMix's mixed labels (include/slk.h "soft targets").

A step's target stays one int64 [B] tensor. A *mixed label* packs two classes and a weight,

    y = a | (b << 8) | (float32_bits(wb) << 32)        a, b in [0, 10), wb in [0, 1] the weight of class b

so the graph caches, `register_inputs` and the loaders' buffer rings carry it unchanged. A plain label is the case
b = 0, wb = 0; a mixed label with wb != 0 is >= 2^32, which the hard-label heads flag as out of range (a trainer
built without `loss=` raises from check_labels instead of training on class a).

    SoftCrossEntropy(label_smoothing)   the loss= of SplitTrainer / WideTrainer and their server stages
    CutMix(prob)                        the mix= of the resident loaders (one slk_image_batch_mix launch per batch)
    pack_mixed / unpack_mixed           torch tensors on any device
    cutmix_draws                        the host twin of the kernel's box draws (numpy, integers only)
"""
from __future__ import annotations

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


@dataclass(frozen=True)
class CutMix:
    """CutMix (Yun et al. 2019) with lam ~ Beta(1, 1): with probability `prob` a sample gets a box of its partner
    (the previous sample of the batch, cyclically) pasted in, and the label becomes the area-weighted pair. The box is
    keyed on (dataset index, epoch, seed) like the crop; `seed` is used only by a loader without `augment` (with one,
    the Augment's seed keys every draw). Other Beta parameters and MixUp are not provided."""
    prob: float = 1.0
    seed: int = 0

    def __post_init__(self):
        if not 0.0 <= float(self.prob) <= 1.0:
            raise ValueError(f"CutMix: prob must be in [0, 1], got {self.prob}")


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


# ------------------------------------------------------------------------------------ CutMix draws (host twin)
def _lowbias32(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def cutmix_draws(idx, epoch: int, seed: int, H: int, W: int, prob: float = 1.0):
    """(apply, y1, y2, x1, x2, wb): the box slk_image_batch_mix pastes into the samples with dataset indices `idx` in
    `epoch` under `seed` (include/slk.h), in uint32 / uint64 numpy arithmetic. apply is bool; the box is rows
    [y1, y2) x columns [x1, x2) (int64, reported also where apply is False); wb is the float32 label weight of the
    partner, area / (H * W) where applied and 0 elsewhere."""
    i = np.asarray(idx).astype(np.int64).astype(np.uint32)
    g = np.uint32(0x9E3779B9)
    with np.errstate(over="ignore"):
        h = _lowbias32(i * np.uint32(0x9E3779B1) + np.uint32(epoch & 0xFFFFFFFF) * np.uint32(0x85EBCA77)
                       + np.uint32(seed & 0xFFFFFFFF) * np.uint32(0xC2B2AE3D))
        hs = [h]
        for _ in range(7):
            h = _lowbias32(h + g)
            hs.append(h)
    h3, h4, h5, h6, h7 = (v.astype(np.uint64) for v in hs[3:8])
    s32 = np.uint64(32)
    apply = h3 < np.uint64(int(float(prob) * 4294967296.0))
    side = np.maximum((h4 * np.uint64(H)) >> s32, (h5 * np.uint64(H)) >> s32).astype(np.int64)
    cy, cx = ((h6 * np.uint64(H)) >> s32).astype(np.int64), ((h7 * np.uint64(W)) >> s32).astype(np.int64)
    half = side // 2
    y1, y2 = np.clip(cy - half, 0, H), np.clip(cy + half, 0, H)
    x1, x2 = np.clip(cx - half, 0, W), np.clip(cx + half, 0, W)
    area = np.where(apply, (y2 - y1) * (x2 - x1), 0)
    wb = area.astype(np.float32) / np.float32(H * W)
    return apply, y1, y2, x1, x2, wb
