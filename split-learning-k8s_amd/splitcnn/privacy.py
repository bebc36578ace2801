"""A noise defence on the cut of the widened model (csrc/slk_cut_noise.hip; the rule is in include/slk.h, "Cut noise").

Split learning keeps the raw data on the client, but the cut activations still leak it to model inversion. The usual
defence (Titcombe et al. 2021; Vepakomma et al.) is additive noise on the cut, with a per-sample norm bound in front of
it so that the noise scale means something. CutNoise is that pair as a config of one launch: clip every sample of
16,384 bf16 elements to an L2 norm of at most `clip`, then add Laplace or Gaussian noise of scale `scale`, drawn from a
1,024-entry quantile table under a counter-based hash keyed on (seed, a device step counter, the global row, the
element). It is a defence to experiment with, NOT a certified differential-privacy mechanism: no epsilon is claimed
for either law, and nothing here accounts for privacy over steps.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .ops import _dev, _stream

NOISE_SAMPLE = 16384        # bf16 elements of one K5 cut [256,8,8] or of one cut-gradient row
NOISE_TABLE = 1024          # strata of the table
NOISE_KINDS = ("laplace", "gaussian")
_M32 = 0xFFFFFFFF


def _halfnormal_quantile(p: float) -> float:
    """q with erf(q / sqrt 2) = p, 0 < p < 1, by bisection in float64."""
    lo, hi = 0.0, 10.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return mid
        if math.erf(mid / math.sqrt(2.0)) < p:
            lo = mid
        else:
            hi = mid


def noise_tables(kind: str):
    """(table, tail) of a law: the float64 [1024] magnitudes at unit scale and the float64 weight of the geometric
    draw G. A noise magnitude is scale * (tail * G + table[k]).
    "laplace":  -ln U = G ln 2 + (-ln U'), G geometric and U' uniform on (1/2, 1): tail = ln 2 and table[k] =
                -log1p(-(k + 0.5) / 2048), the value of -ln U' at the middle of stratum k. Exact in distribution up
                to the 1,024 strata; G stops at 32, which cuts the tail at about 32 ln 2 with probability 2^-32.
    "gaussian": tail = 0 and table[k] = the half-normal quantile at (k + 0.5) / 1024: 2,048 values with the sign, the
                support ends at 3.487 and the variance is 0.99936 (a unit normal's tails beyond 3.49 are missing)."""
    if kind == "laplace":
        return np.array([-math.log1p(-(k + 0.5) / 2048.0) for k in range(NOISE_TABLE)], dtype=np.float64), math.log(2.0)
    if kind == "gaussian":
        return np.array([_halfnormal_quantile((k + 0.5) / NOISE_TABLE) for k in range(NOISE_TABLE)],
                        dtype=np.float64), 0.0
    raise ValueError(f"noise_tables: kind={kind!r}; expected one of {list(NOISE_KINDS)}")


def _hash32(x: np.ndarray) -> np.ndarray:
    """lowbias32 on uint64 arrays holding uint32 values."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def noise_draws(rows, t: int, seed: int):
    """The host twin of the kernel's draws for the global rows `rows` (row0 + row in the launch) at counter value t:
    (neg, k, G), each [len(rows), 16384] — the sign bit, the stratum and the geometric count of every element. The
    noise of an element is (-1)^neg * scale * (tail * G + table[k]), each operation rounded to float32."""
    g = np.asarray(rows, dtype=np.uint64).reshape(-1, 1) & _M32
    i = np.arange(NOISE_SAMPLE, dtype=np.uint64).reshape(1, -1)
    key = ((int(t) & _M32) * 0x85EBCA77 + (int(seed) & _M32) * 0xC2B2AE3D + 3 * 0x27D4EB2F) & _M32
    base = _hash32((g * 0x9E3779B1 + key) & _M32)
    r = _hash32((base + i * 0x9E3779B1) & _M32)
    r2 = _hash32((r + 0x9E3779B9) & _M32)
    G = 32 - np.frexp(r2.astype(np.float64))[1]   # frexp's exponent is the bit length (0 for 0): clz, 32 for r2 = 0
    return (r >> 31).astype(np.int64), ((r >> 21) & 1023).astype(np.int64), G.astype(np.int64)


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


class CutNoise:
    """Clip, then noise, on the K5 cut, as a config (slk_cut_noise; its backward is slk_cut_scale_rows).

    `scale` (the Laplace b or the Gaussian sigma) and `clip` (the per-sample L2 bound) live in device f32[1] scalars
    the kernel reads, so a captured HIP graph follows `set_scale` / `set_clip` without being recaptured. clip=None
    builds no clip at all: no reduction runs, no backward launch exists, and a later set_clip raises; clip=inf clips
    nothing but still measures the norms. `kind`, `seed`, the table and `tail` are constructor constants passed to
    the kernel by value (the table by its pointer): a captured graph keeps them, and there is no setter. A table of
    your own (`table`, float32 [1024], with `tail`, default 0) replaces the law's; its values are not validated on
    the device, and the noise magnitude of an element is scale * (tail * G + table[k]).

    The clip coefficient is treated as a constant in the backward pass (detached, as the FP8 codec is straight
    through): the client back-propagates coef_row * dcut. Differentiating through the norm would add a term along the
    sample; this deviation is deliberate and documented.

    A sample is 16,384 contiguous bf16 elements: x / out are [n, ...] with 16,384 elements per row. Every method
    works on caller-visible buffers and launches on the tensor's current stream."""

    def __init__(self, kind: str = "laplace", scale: float = 0.0, clip=None, seed: int = 0, table=None, tail=None,
                 device="cuda"):
        if not isinstance(kind, str) or kind not in NOISE_KINDS:
            raise ValueError(f"CutNoise: kind={kind!r}; expected one of {list(NOISE_KINDS)}")
        self.scale = self._checked_scale(scale)
        self.clip = None if clip is None else self._checked_clip(clip)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"CutNoise: seed={seed!r}; expected an integer in [0, 2^32)")
        self.seed = int(seed)
        if table is None:
            if tail is not None:
                raise ValueError("CutNoise: tail= goes with a table of your own (table=)")
            t64, tail = noise_tables(kind)
            tab = t64.astype(np.float32)
            self.kind = kind
        else:
            if isinstance(table, torch.Tensor):
                table = table.detach().cpu().numpy()
            if not isinstance(table, np.ndarray) or table.dtype != np.float32 or table.shape != (NOISE_TABLE,):
                raise ValueError(f"CutNoise: table must be float32 [{NOISE_TABLE}]")
            tail = 0.0 if tail is None else tail
            if not _number(tail) or not math.isfinite(tail):
                raise ValueError(f"CutNoise: tail={tail!r}; expected a finite number")
            tab = np.ascontiguousarray(table)
            self.kind = "table"
        self.tail = float(np.float32(tail))
        self.table = torch.from_numpy(tab.copy()).to(device)
        self.scale_value = torch.full((1,), self.scale, dtype=torch.float32, device=device)
        self.clip_value = (None if self.clip is None else
                           torch.full((1,), self.clip, dtype=torch.float32, device=device))

    @staticmethod
    def _checked_scale(scale) -> float:
        if not _number(scale) or not 0.0 <= scale < math.inf:   # NaN fails this too
            raise ValueError(f"CutNoise: scale={scale!r}; expected a finite number >= 0")
        return float(scale)

    @staticmethod
    def _checked_clip(clip) -> float:
        if not _number(clip) or not clip > 0.0:   # NaN fails this too
            raise ValueError(f"CutNoise: clip={clip!r}; expected a number > 0 (inf clips nothing) or None")
        return float(clip)

    def to(self, device) -> "CutNoise":
        """Move the table and the scalars (a no-op on their own device); captured graphs hold their addresses, so
        move a CutNoise before the first step only."""
        if self.table.device != torch.device(device):
            self.table, self.scale_value = self.table.to(device), self.scale_value.to(device)
            if self.clip_value is not None:
                self.clip_value = self.clip_value.to(device)
        return self

    def set_scale(self, scale: float) -> None:
        """Overwrite the noise scale in place: an asynchronous device write on the current stream, so the next
        launch — eager or a replay of an already captured graph — draws at `scale`."""
        self.scale = self._checked_scale(scale)
        self.scale_value.fill_(self.scale)

    def set_clip(self, clip: float) -> None:
        """Overwrite the norm bound in place, like set_scale. A CutNoise built with clip=None has no clip to set."""
        if self.clip_value is None:
            raise RuntimeError("CutNoise: built with clip=None — there is no clip launch to retarget; build one with "
                               "clip= (inf clips nothing)")
        self.clip = self._checked_clip(clip)
        self.clip_value.fill_(self.clip)

    def __repr__(self):
        return f"CutNoise(kind={self.kind!r}, scale={self.scale}, clip={self.clip}, seed={self.seed})"

    @staticmethod
    def _rows(t, name) -> int:
        _dev(t, name, dtype=torch.bfloat16)
        if t.dim() < 1 or t.numel() != t.shape[0] * NOISE_SAMPLE:
            raise ValueError(f"{name}: expected [n, ...] with {NOISE_SAMPLE} elements per sample, got {tuple(t.shape)}")
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: the base address must be 16-byte aligned")
        return int(t.shape[0])

    @staticmethod
    def _stats(stats, n, like):
        _dev(stats, "stats", (n, 2), torch.float32)
        if stats.device != like.device:
            raise ValueError(f"stats: on {stats.device}, the tensor is on {like.device}")
        if stats.data_ptr() % 8:
            raise ValueError("stats: the base address must be 8-byte aligned")
        return stats.data_ptr()

    def _mine(self, x):
        if self.table.device != x.device:
            raise ValueError(f"CutNoise: its table and scalars are on {self.table.device}, the tensor is on {x.device} "
                             "(CutNoise.to(device) before the first step)")

    def apply(self, x, out, step=None, row0: int = 0, stats=None, noise: bool = True):
        """out = noise(clip(x)); out may be x. `step` is a device int32[1] counter the kernel reads at run time (a
        stage's step_ctr; a captured graph follows it) and `row0` the global row of x[0], so a slice of a batch gives
        the bits of the whole batch. With a clip, `stats` (f32 [n, 2]) receives (norm, coef) per sample; None keeps
        none. noise=False applies the clip alone (evaluation): nothing is drawn and step / row0 are not read."""
        n = self._rows(x, "x")
        if self._rows(out, "out") != n:
            raise ValueError(f"out: expected {n} samples like x, got {out.shape[0]}")
        if out.device != x.device:
            raise ValueError(f"out: on {out.device}, x is on {x.device}")
        self._mine(x)
        table = scale = step_p = clip = stats_p = None
        if noise:
            if step is None:
                raise ValueError("CutNoise.apply: noise needs step=, a device int32[1] counter (a stage's step_ctr)")
            _dev(step, "step", (1,), torch.int32)
            if step.device != x.device:
                raise ValueError(f"step: on {step.device}, the tensor is on {x.device}")
            if isinstance(row0, bool) or not isinstance(row0, int) or not 0 <= row0 < 2 ** 31:
                raise ValueError(f"row0={row0!r}; expected an integer in [0, 2^31)")
            table, scale, step_p = self.table.data_ptr(), self.scale_value.data_ptr(), step.data_ptr()
        else:
            row0 = 0
        if self.clip_value is not None:
            clip = self.clip_value.data_ptr()
            if stats is not None:
                stats_p = self._stats(stats, n, x)
        elif stats is not None:
            raise ValueError("CutNoise.apply: stats= without a clip (built with clip=None): nothing would write it")
        _lib.call("slk_cut_noise", x.data_ptr(), n, table, self.tail, scale, clip, self.seed, step_p, row0,
                  out.data_ptr(), stats_p, _stream(x))
        return out

    def scale_rows(self, dcut, stats, out):
        """out = coef_row * dcut, coef_row = stats[row, 1] of the forward apply: the backward of the clip with the
        coefficient held constant; out may be dcut."""
        n = self._rows(dcut, "dcut")
        if self._rows(out, "out") != n:
            raise ValueError(f"out: expected {n} samples like dcut, got {out.shape[0]}")
        if out.device != dcut.device:
            raise ValueError(f"out: on {out.device}, dcut is on {dcut.device}")
        _lib.call("slk_cut_scale_rows", dcut.data_ptr(), n, self._stats(stats, n, dcut), out.data_ptr(), _stream(dcut))
        return out


def check_cut_noise(noise):
    """A trainer's / hub's noise argument: a CutNoise or None."""
    if noise is not None and not isinstance(noise, CutNoise):
        raise TypeError(f"expected splitcnn.privacy.CutNoise or None, got {type(noise).__name__}")
    return noise
