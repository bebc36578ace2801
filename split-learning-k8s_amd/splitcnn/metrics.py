"""Evaluation metrics accumulated on the device.

The reference builds a test split (src/client_part.py:52,73) and never evaluates on it. `EvalMetrics`
owns the 104-word accumulator that slk_eval_accumulate (include/slk.h) updates once per batch — sample
count, correct predictions, loss sum (float64) and the 10 x 10 confusion counts — so a whole dataset is
evaluated with no host sync until `result()` copies those 832 bytes back once.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops

NCLS = 10


@dataclass
class EvalResult:
    """Decoded metrics of an evaluation. confusion[label, pred]; loss = mean over the samples with a valid
    label; per_class_accuracy[c] = confusion[c, c] / samples of class c (NaN for a class never seen)."""
    n: int
    correct: int
    bad_labels: int
    accuracy: float
    loss: float
    confusion: np.ndarray
    per_class_accuracy: np.ndarray

    @classmethod
    def from_raw(cls, raw) -> "EvalResult":
        """Decode a raw accumulator (int64 [104], the layout of slk_eval_accumulate): a pure host function."""
        a = np.ascontiguousarray(np.asarray(raw, dtype=np.int64).reshape(-1))
        if a.size != ops.EVAL_ACC_WORDS:
            raise ValueError(f"accumulator: expected {ops.EVAL_ACC_WORDS} int64 words, got {a.size}")
        n, correct, bad = int(a[0]), int(a[1]), int(a[2])
        loss_sum = float(a[3:4].view(np.float64)[0])
        confusion = a[4:].reshape(NCLS, NCLS).copy()
        valid = n - bad
        rows = confusion.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            per_class = np.where(rows > 0, np.diag(confusion) / np.maximum(rows, 1), np.nan)
        return cls(n=n, correct=correct, bad_labels=bad,
                   accuracy=correct / valid if valid > 0 else float("nan"),
                   loss=loss_sum / valid if valid > 0 else float("nan"),
                   confusion=confusion, per_class_accuracy=per_class)

    def check(self) -> "EvalResult":
        """Raise if any evaluated label was outside [0, 10) (torch raises IndexError there)."""
        if self.bad_labels > 0:
            raise IndexError("splitcnn: a label was out of range [0, 10)")
        return self


class EvalMetrics:
    """The device-side metric accumulator: reset(), update(loss_i, pred, labels) per batch (one launch, no
    sync), result() -> EvalResult (one device-to-host copy)."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"splitcnn: EvalMetrics on {self.device}; the metrics accumulate on the MI355X HIP "
                               "kernels only. There is no CPU fallback.")
        self.acc = torch.zeros(ops.EVAL_ACC_WORDS, dtype=torch.int64, device=self.device)

    def reset(self) -> "EvalMetrics":
        self.acc.zero_()
        return self

    def update(self, loss_i: torch.Tensor, pred: torch.Tensor, labels: torch.Tensor) -> None:
        ops.eval_accumulate(loss_i, pred, labels, self.acc)

    def result(self) -> EvalResult:
        return EvalResult.from_raw(self.acc.cpu().numpy())


def evaluate_logits(logits: torch.Tensor, labels: torch.Tensor, metrics: Optional[EvalMetrics] = None):
    """Loss and prediction of f32 [B, 10] device logits from any path (the drop-in modules, the U-shaped head):
    returns (pred, loss_i) and adds the batch to `metrics` when given."""
    loss_i, pred = ops.eval_logits(logits, labels)
    if metrics is not None:
        metrics.update(loss_i, pred, labels)
    return pred, loss_i
