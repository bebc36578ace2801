"""Optimizer recipes and learning-rate schedules for the stage engines (engine.py: K2, wide.py: K5).

The reference trains with two fixed recipes (optim.SGD(lr=0.01): src/client_part.py:17,133,
src/server_part.py:15,52; the widened config with Adam(lr=1e-3)). `SGD` and `Adam` here are plain config
objects with torch's semantics (torch.optim.SGD; torch.optim.Adam / AdamW) for the fused reduce + step
kernels slk_sgdm_* and slk_adamw_*; `LRSchedule` is the learning rate as a device table those kernels
index with the stage's device step counter, so a captured HIP graph follows a schedule (or `set_lr`)
without being recaptured and without a host sync.

    from splitcnn import optim
    sched = optim.LRSchedule.warmup_cosine(0.05, warmup=100, total=2000)
    tr = SplitTrainer(client, server, optim=optim.SGD(0.05, momentum=0.9, nesterov=True, weight_decay=5e-4),
                      schedule=sched, clip=optim.ClipNorm(1.0))

`ClipNorm` is torch.nn.utils.clip_grad_norm_ (L2 norm, error_if_nonfinite=False) in front of every optimizer
step, per stage: each stage clips by the norm of its own gradient (the reference's two parties have two
optimizers and the client never sees the server's gradient), also in the fused one-GPU trainers. With it the
fused reduce + step launch becomes two (slk_reduce_sqnorm_multi, then slk_sgdm_clip_multi /
slk_adamw_clip_multi): the whole norm must exist before the first parameter moves. Norm, coefficient and
threshold stay on the device; trainer.grad_norms() reads the last step's. One deviation from torch:
`stage.grads` keeps the UNCLIPPED reduced gradient (torch scales p.grad in place); the gradient the optimizer
consumed is coef * grads. The clip tensors are no optimizer state (optimizer_state() keeps its keys).

`LARS` (an SGD, for the K2 stages) and `LAMB` (an Adam, for the K5 stages) scale every tensor's step by a trust
ratio of two of its own norms; a tensor is one weight or one bias, and `exclude_bias` (the default) keeps the
biases at ratio 1 without weight decay. They run as two launches like a clipped step (slk_reduce_tnorm_multi ->
slk_lars_multi, slk_lamb_moments_multi -> slk_lamb_multi), inside the captured graph and at the schedule's rate;
trainer.trust_ratios() reads the last step's norms and ratios. The optimizer state keeps its keys (momentum
buffer, or m and v, plus the counter). Not combined with clip=, and not taken by dist.py, the U-shaped or the
federated paths: those raise ValueError.

`EMA` keeps an exponential moving average of a stage's parameters, updated by one launch (slk_ema_multi) after the
optimizer launch(es) of every step and before the counter's tick, inside the captured graph; the trainers evaluate
on it (evaluate / eval_batch / predict with weights="ema") and ema_state_dict() reads it. Its decay is device
memory (`set_decay`), `warmup` and `start` are by-value constants a captured graph keeps. The averaged blocks join
optimizer_state() as client.ema / server.ema only when ema= was given. Not taken by dist.py, the U-shaped or the
federated paths: those raise ValueError.

Limits: one rate and one recipe per stage (the only per-parameter distinction is weight / bias under the
layer-wise recipes), L2 norm only (no clip_grad_value_), and the multi-GPU classes of dist.py take only stages
built without a config.
"""
from __future__ import annotations

import math
from typing import Callable, Sequence, Tuple

import numpy as np
import torch


class SGD:
    """torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov) as a config."""

    def __init__(self, lr: float, momentum: float = 0.0, dampening: float = 0.0, nesterov: bool = False,
                 weight_decay: float = 0.0):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.lr, self.momentum, self.dampening = float(lr), float(momentum), float(dampening)
        self.nesterov, self.weight_decay = bool(nesterov), float(weight_decay)

    def kernel_args(self) -> dict:
        return {"momentum": self.momentum, "dampening": self.dampening, "weight_decay": self.weight_decay,
                "nesterov": self.nesterov}

    def __repr__(self):
        return (f"SGD(lr={self.lr}, momentum={self.momentum}, dampening={self.dampening}, "
                f"nesterov={self.nesterov}, weight_decay={self.weight_decay})")


class Adam:
    """torch.optim.AdamW (decoupled=True, the default) or torch.optim.Adam(weight_decay=...) (decoupled=False)
    as a config; with weight_decay 0 the two are the same update."""

    def __init__(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled: bool = True):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled = float(weight_decay), bool(decoupled)

    def kernel_args(self) -> dict:
        return {"beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps, "weight_decay": self.weight_decay,
                "decoupled": self.decoupled}

    def __repr__(self):
        return (f"Adam(lr={self.lr}, betas={self.betas}, eps={self.eps}, weight_decay={self.weight_decay}, "
                f"decoupled={self.decoupled})")


class LARS(SGD):
    """Layer-wise adaptive rate scaling (You, Gitman, Ginsburg 2017; timm's Lars with trust_clip=False) on the
    SGD family: per tensor ratio = trust_coef * |w| / (|g| + weight_decay * |w| + eps), 1 where |w| or |g| is 0,
    and torch.optim.SGD's momentum arithmetic on ratio * (g + weight_decay * w). With exclude_bias a bias runs
    at ratio 1 and weight decay 0: plain momentum SGD at lr."""

    def __init__(self, lr: float, momentum: float = 0.9, dampening: float = 0.0, nesterov: bool = False,
                 weight_decay: float = 0.0, trust_coef: float = 1e-3, eps: float = 1e-8, exclude_bias: bool = True):
        super().__init__(lr, momentum, dampening, nesterov, weight_decay)
        if not trust_coef > 0.0:
            raise ValueError(f"Invalid trust_coef value: {trust_coef}")
        if not eps >= 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        self.trust_coef, self.eps, self.exclude_bias = float(trust_coef), float(eps), bool(exclude_bias)

    def kernel_args(self) -> dict:
        return dict(super().kernel_args(), trust_coef=self.trust_coef, eps=self.eps, exclude_bias=self.exclude_bias)

    def __repr__(self):
        return (f"LARS(lr={self.lr}, momentum={self.momentum}, dampening={self.dampening}, nesterov={self.nesterov}, "
                f"weight_decay={self.weight_decay}, trust_coef={self.trust_coef}, eps={self.eps}, "
                f"exclude_bias={self.exclude_bias})")


class LAMB(Adam):
    """LAMB (You et al. 2019, algorithm 2; apex FusedLAMB and timm's Lamb without their gradient pre-clipping) on
    the Adam family: u = m-hat / (sqrt(v-hat) + eps) + weight_decay * w, per tensor ratio = |w| / |u| (1 where
    either is 0) and w -= lr * ratio * u. With exclude_bias a bias runs at ratio 1 and weight decay 0: plain
    Adam at lr."""

    def __init__(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, exclude_bias: bool = True):
        super().__init__(lr, betas, eps, weight_decay, decoupled=True)
        self.exclude_bias = bool(exclude_bias)

    def kernel_args(self) -> dict:
        return {"beta1": self.betas[0], "beta2": self.betas[1], "eps": self.eps, "weight_decay": self.weight_decay,
                "exclude_bias": self.exclude_bias}

    def __repr__(self):
        return (f"LAMB(lr={self.lr}, betas={self.betas}, eps={self.eps}, weight_decay={self.weight_decay}, "
                f"exclude_bias={self.exclude_bias})")


def is_layerwise(optim) -> bool:
    """Whether a config is one of the layer-wise recipes (the two trust-ratio launches instead of the fused one)."""
    return isinstance(optim, (LARS, LAMB))


def refuse_layerwise(optim, who: str):
    """A path that cannot run the layer-wise launches must not run plain SGD / Adam in their place."""
    if is_layerwise(optim):
        raise ValueError(f"{who}: {type(optim).__name__} (layer-wise trust ratios) is not supported here; it runs "
                         "on the one-GPU stages and trainers without clip=")


class ClipNorm:
    """torch.nn.utils.clip_grad_norm_(stage parameters, max_norm) (L2) before every optimizer step of a
    stage, as a config: the threshold is a device f32[1] the clipped-step kernels read, so a captured HIP
    graph follows `set_max_norm` without being recaptured. max_norm = inf clips nothing (coef = 1: bitwise
    the unclipped configured step) but still measures the norms (trainer.grad_norms())."""

    def __init__(self, max_norm: float, device="cuda"):
        self.max_norm = self._checked(max_norm)
        self.value = torch.full((1,), self.max_norm, dtype=torch.float32, device=device)

    @staticmethod
    def _checked(max_norm) -> float:
        if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float, np.integer, np.floating)):
            raise ValueError(f"Invalid max_norm: {max_norm!r}")
        if not max_norm > 0.0:   # NaN fails this too
            raise ValueError(f"Invalid max_norm: {max_norm} (need max_norm > 0; inf clips nothing)")
        return float(max_norm)

    def to(self, device) -> "ClipNorm":
        """Move the threshold (a no-op on its own device); captured graphs hold its address, so move a
        ClipNorm before the first step only."""
        if self.value.device != torch.device(device):
            self.value = self.value.to(device)
        return self

    def set_max_norm(self, max_norm: float) -> None:
        """Overwrite the threshold in place: an asynchronous device write on the current stream, so the next
        step — eager or a replay of an already captured graph — clips at `max_norm`."""
        self.max_norm = self._checked(max_norm)
        self.value.fill_(self.max_norm)

    def __repr__(self):
        return f"ClipNorm(max_norm={self.max_norm})"


def check_clip(clip):
    if clip is not None and not isinstance(clip, ClipNorm):
        raise TypeError(f"clip: expected splitcnn.optim.ClipNorm or None, got {type(clip).__name__}")
    return clip


class EMA:
    """An exponential moving average of a stage's parameters, kept after every optimizer step, as a config:
    e <- e + (1 - d)(p - e) in float32 (torch.optim.swa_utils.AveragedModel's lerp), in one launch (slk_ema_multi)
    between the stage's optimizer launches and the tick of its step counter k. With t = k - start: t < 0 copies
    the parameters (the average starts at step `start`); otherwise n = t + 1 and d = min(decay, (1 + n) / (10 + n))
    under `warmup` (TensorFlow's / torch_ema's num_updates form), else d = decay. The decay is a device f32[1] the
    kernel reads, so a captured HIP graph follows `set_decay` without being recaptured. `warmup` and `start` are
    constructor constants passed to the kernel by value: a captured graph keeps them, and there is no setter."""

    def __init__(self, decay: float = 0.999, warmup: bool = True, start: int = 0, device="cuda"):
        self.decay = self._checked(decay)
        if not isinstance(warmup, (bool, np.bool_)):
            raise ValueError(f"Invalid warmup: {warmup!r} (a bool)")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < 2 ** 31:
            raise ValueError(f"Invalid start: {start!r} (an optimizer step count >= 0)")
        self.warmup, self.start = bool(warmup), int(start)
        self.value = torch.full((1,), self.decay, dtype=torch.float32, device=device)

    @staticmethod
    def _checked(decay) -> float:
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)):
            raise ValueError(f"Invalid decay: {decay!r}")
        if not 0.0 <= decay < 1.0 or not float(np.float32(decay)) < 1.0:   # NaN fails this too; so does 1 - 1e-9 in f32
            raise ValueError(f"Invalid decay: {decay} (need 0 <= decay < 1 in float32)")
        return float(decay)

    def to(self, device) -> "EMA":
        """Move the decay (a no-op on its own device); captured graphs hold its address, so move an EMA before
        the first step only."""
        if self.value.device != torch.device(device):
            self.value = self.value.to(device)
        return self

    def set_decay(self, decay: float) -> None:
        """Overwrite the decay in place: an asynchronous device write on the current stream, so the next step —
        eager or a replay of an already captured graph — averages at `decay`."""
        self.decay = self._checked(decay)
        self.value.fill_(self.decay)

    def __repr__(self):
        return f"EMA(decay={self.decay}, warmup={self.warmup}, start={self.start})"


def check_ema(ema):
    if ema is not None and not isinstance(ema, EMA):
        raise TypeError(f"ema: expected splitcnn.optim.EMA or None, got {type(ema).__name__}")
    return ema


class LRSchedule:
    """The learning rate of every optimizer step as an f32 device table: step k (0-based, the stage's device
    counter) runs at table[min(k, len - 1)]. The host fills the table once; the kernels read it."""

    def __init__(self, values: Sequence[float], device="cuda"):
        v = np.asarray(values, dtype=np.float32).reshape(-1)
        if v.size < 1:
            raise ValueError("LRSchedule: needs at least one rate")
        if not np.all(np.isfinite(v)) or np.any(v < 0):
            raise ValueError("LRSchedule: rates must be finite and >= 0")
        self.values = v.copy()
        self.table = torch.from_numpy(v.copy()).to(device)

    def __len__(self):
        return int(self.values.size)

    def lr_at(self, step: int) -> float:
        """The rate of optimizer step `step` (host copy of the table; past the end the last value holds)."""
        return float(self.values[min(max(int(step), 0), len(self) - 1)])

    def to(self, device) -> "LRSchedule":
        """Move the table (a no-op on its own device); captured graphs hold the table's address, so move
        a schedule before the first step only."""
        if self.table.device != torch.device(device):
            self.table = self.table.to(device)
        return self

    def set_lr(self, lr: float) -> None:
        """Overwrite a constant (one-entry) table in place: an asynchronous device write on the current
        stream, so the next step — eager or a replay of an already captured graph — runs at `lr`."""
        if len(self) != 1:
            raise ValueError("LRSchedule.set_lr: only a constant (one-entry) schedule can be overwritten")
        if not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError(f"Invalid learning rate: {lr}")
        self.values[0] = lr
        self.table.fill_(float(lr))

    # ---- constructors
    @classmethod
    def constant(cls, lr: float, device="cuda") -> "LRSchedule":
        return cls([lr], device)

    @classmethod
    def from_values(cls, seq: Sequence[float], device="cuda") -> "LRSchedule":
        return cls(seq, device)

    @classmethod
    def from_torch(cls, make_scheduler: Callable, base_lr: float, steps: int, device="cuda") -> "LRSchedule":
        """Record a torch.optim.lr_scheduler: make_scheduler(optimizer) -> scheduler runs on a dummy CPU
        parameter at `base_lr`; entry k is get_last_lr()[0] after k scheduler steps."""
        if steps < 1:
            raise ValueError("LRSchedule.from_torch: steps must be >= 1")
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
        sched = make_scheduler(opt)
        vals = []
        for k in range(steps):
            vals.append(sched.get_last_lr()[0])
            if k + 1 < steps:   # a scheduler with a fixed length (OneCycleLR) refuses a step past its end
                opt.step()
                sched.step()
        return cls(vals, device)

    @classmethod
    def warmup_cosine(cls, base_lr: float, warmup: int, total: int, min_lr: float = 0.0,
                      device="cuda") -> "LRSchedule":
        """Linear warm-up over `warmup` steps (base_lr * (k + 1) / warmup), then a half cosine from base_lr
        to min_lr at step total - 1 (a LambdaLR)."""
        if not 0 <= warmup < total:
            raise ValueError("LRSchedule.warmup_cosine: need 0 <= warmup < total")
        floor = min_lr / base_lr if base_lr > 0 else 0.0
        span = max(1, total - 1 - warmup)

        def factor(k):
            if k < warmup:
                return (k + 1) / warmup
            return floor + (1.0 - floor) * 0.5 * (1.0 + math.cos(math.pi * min(k - warmup, span) / span))
        return cls.from_torch(lambda o: torch.optim.lr_scheduler.LambdaLR(o, factor), base_lr, total, device)

    @classmethod
    def step_decay(cls, base_lr: float, step_size: int, gamma: float, steps: int, device="cuda") -> "LRSchedule":
        """base_lr * gamma ** (k // step_size) (a StepLR)."""
        return cls.from_torch(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size, gamma), base_lr, steps, device)
