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

from . import _lib, ops
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


# ------------------------------------------------------------------------------------ DP-SGD on the client's weights
DP_ORDERS = tuple(range(2, 257))   # the integer Renyi orders the accountant minimises over


class DPSGD:
    """DP-SGD (Abadi et al. 2016) on the K5 client's weights, as a config of WideClientStage / WideTrainer(dp=...):
    every sample's client gradient is clipped to an L2 norm of at most `max_grad_norm` (C), the clipped gradients are
    summed and N(0, (noise_multiplier * C)^2) is added to the sum (include/slk.h, "DP-SGD on the K5 client").

    C and sigma live in device f32[1] scalars the kernels read, so a captured HIP graph follows `set_max_grad_norm` /
    `set_noise_multiplier` without being recaptured. `seed` is passed by value: a captured graph keeps it. A stage
    built with noise_multiplier == 0 has no noise row at all (a later set_noise_multiplier raises); max_grad_norm=inf
    clips nothing but still measures the norms.

    The stage takes the cut gradient of the MEAN loss over its batch (grad_scale = 1 / B, what WideTrainer and
    WideServerStage.step_request hand it): norms are reported as B x the measured ones and the noise is scaled by 1 / B.
    A dcut at any other scale is clipped and noised at the wrong sensitivity, without an error.

    Deviations: the clipped gradient is the backward of bf16(coef_b * dcut_b), so the sensitivity bound holds up to
    bf16 rounding; the norm is measured on the unscaled pass; the Gaussian's support ends at 5.77 sigma; only the
    client stage is covered (the server is the other party, with its own optimizer)."""

    def __init__(self, max_grad_norm: float, noise_multiplier: float, seed: int = 0, device="cuda"):
        self.max_grad_norm = self._checked_norm(max_grad_norm)
        self.noise_multiplier = self._checked_sigma(noise_multiplier)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"DPSGD: seed={seed!r}; expected an integer in [0, 2^32)")
        self.seed = int(seed)
        self.noisy = self.noise_multiplier > 0.0
        self.norm_value = torch.full((1,), self.max_grad_norm, dtype=torch.float32, device=device)
        self.sigma_value = torch.full((1,), self.noise_multiplier, dtype=torch.float32, device=device)

    @staticmethod
    def _checked_norm(c) -> float:
        if not _number(c) or not c > 0.0:   # NaN fails this too
            raise ValueError(f"DPSGD: max_grad_norm={c!r}; expected a number > 0 (inf clips nothing)")
        return float(c)

    @staticmethod
    def _checked_sigma(s) -> float:
        if not _number(s) or not 0.0 <= s < math.inf:   # NaN fails this too
            raise ValueError(f"DPSGD: noise_multiplier={s!r}; expected a finite number >= 0")
        return float(s)

    def to(self, device) -> "DPSGD":
        """Move the scalars (a no-op on their own device); captured graphs hold their addresses, so move a DPSGD
        before the first step only."""
        if self.norm_value.device != torch.device(device):
            self.norm_value, self.sigma_value = self.norm_value.to(device), self.sigma_value.to(device)
        return self

    def set_max_grad_norm(self, c: float) -> None:
        """Overwrite C in place: an asynchronous device write on the current stream, so the next launch — eager or a
        replay of an already captured graph — clips at `c`."""
        self.max_grad_norm = self._checked_norm(c)
        self.norm_value.fill_(self.max_grad_norm)

    def set_noise_multiplier(self, sigma: float) -> None:
        """Overwrite sigma in place, like set_max_grad_norm. A DPSGD built with noise_multiplier == 0 has no noise
        row to retarget."""
        if not self.noisy:
            raise RuntimeError("DPSGD: built with noise_multiplier == 0 — there is no noise launch to retarget; "
                               "build one with noise_multiplier > 0")
        self.noise_multiplier = self._checked_sigma(sigma)
        self.sigma_value.fill_(self.noise_multiplier)

    def __repr__(self):
        return (f"DPSGD(max_grad_norm={self.max_grad_norm}, noise_multiplier={self.noise_multiplier}, "
                f"seed={self.seed})")

    def noise_draws(self, idx, step: int) -> np.ndarray:
        """The host twin of slk_dp_noise's unit draws z for the flat parameter indices `idx` at counter value `step`,
        in float64 on the kernel's own integers (the kernel evaluates the same expression in float32)."""
        j = np.asarray(idx, dtype=np.uint64) & _M32
        key = ((int(step) & _M32) * 0x85EBCA77 + self.seed * 0xC2B2AE3D) & _M32
        h0 = _hash32((j * 0x9E3779B1 + key) & _M32)
        h1 = _hash32((h0 + 0x9E3779B9) & _M32)
        u1 = ((h0 >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
        u2 = (h1 >> 8).astype(np.float64) * 2.0 ** -24
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

    def epsilon(self, steps: int, sample_rate: float, delta: float) -> float:
        """epsilon of (epsilon, delta)-DP after `steps` steps at this noise multiplier: the Renyi-DP accountant of the
        subsampled Gaussian mechanism over the integer orders DP_ORDERS (Mironov, Talwar, Zhang 2019, the binomial
        expansion), composed over the steps and converted as eps = min_a (steps * rdp(a) + log(1 / delta) / (a - 1)).
        It ASSUMES Poisson sampling at `sample_rate` while the loaders here shuffle and cut fixed-size batches (Opacus
        carries the same caveat), and it knows nothing of the bf16 rounding of the clipped gradient or of the noise's
        finite support. Infinite for noise_multiplier == 0."""
        if not 0.0 < sample_rate <= 1.0 or not 0.0 < delta < 1.0 or steps < 0:
            raise ValueError("epsilon: expected steps >= 0, 0 < sample_rate <= 1 and 0 < delta < 1")
        return rdp_epsilon(self.noise_multiplier, steps, sample_rate, delta)


def subsampled_gaussian_rdp(sigma: float, q: float, alpha: int) -> float:
    """Renyi divergence of order alpha (an integer >= 2) of one step of the Poisson-subsampled Gaussian mechanism:
    log(sum_i C(alpha, i) (1 - q)^(alpha - i) q^i exp((i^2 - i) / (2 sigma^2))) / (alpha - 1), in log space."""
    i = np.arange(alpha + 1, dtype=np.float64)
    logc = np.array([math.lgamma(alpha + 1) - math.lgamma(k + 1) - math.lgamma(alpha - k + 1) for k in range(alpha + 1)])
    with np.errstate(divide="ignore", invalid="ignore"):
        rest = np.where(alpha - i > 0, (alpha - i) * np.log1p(-q), 0.0)
    terms = logc + rest + i * math.log(q) + (i * i - i) / (2.0 * sigma * sigma)
    return float(np.logaddexp.reduce(terms)) / (alpha - 1)


def rdp_epsilon(sigma: float, steps: int, sample_rate: float, delta: float, orders=DP_ORDERS) -> float:
    if sigma <= 0.0:
        return math.inf
    return min(steps * subsampled_gaussian_rdp(sigma, sample_rate, a) + math.log(1.0 / delta) / (a - 1) for a in orders)


def check_dpsgd(dp):
    """A stage's / trainer's dp argument: a DPSGD or None."""
    if dp is not None and not isinstance(dp, DPSGD):
        raise TypeError(f"expected splitcnn.privacy.DPSGD or None, got {type(dp).__name__}")
    return dp


# ------------------------------------------------------------------------------------ what a defence buys
class DistanceCorrelation:
    """The four numbers of one distance_correlation call: dcor, dcov2, dvar_x, dvar_z (Python floats). They are read
    back from the device on first access, with one host sync (like WideTrainer.cut_stats); `values` is the f32 [4]
    device tensor itself, in that order, for a caller that stays on the device (inside a graph capture)."""

    _FIELDS = ("dcor", "dcov2", "dvar_x", "dvar_z")

    def __init__(self, values: torch.Tensor):
        self.values = values
        self._host = None

    def __getattr__(self, name):
        if name in DistanceCorrelation._FIELDS:
            if self._host is None:
                self._host = tuple(float(v) for v in self.values.cpu())
            return self._host[DistanceCorrelation._FIELDS.index(name)]
        raise AttributeError(name)

    def __repr__(self):
        return "DistanceCorrelation(" + ", ".join(f"{k}={getattr(self, k):.6g}" for k in self._FIELDS) + ")"


_DCOR_WORKSPACES: dict = {}


def dcor_tau(which: str) -> float:
    """The resolution constant of an operand ("x" or "z"): a squared distance at or below tau * (s_i + s_j) counts as
    0 (include/slk.h, "Distance correlation")."""
    return _lib.query("slk_dcor_tau", {"x": 0, "z": 1}[which]) * 2.0 ** -24


def _dcor_width(t, name, dtype) -> int:
    """Elements per sample of t, after the rules that need no device: dtype, [n, ...], a multiple of 64."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() < 2:
        raise ValueError(f"{name}: expected [n, ...] with at least 2 dimensions, got {tuple(t.shape)}")
    d = int(np.prod(t.shape[1:]))
    if d == 0 or d % 64:
        raise ValueError(f"{name}: {d} elements per sample; expected a positive multiple of 64")
    return d


def _dcor_rows(t, name, d):
    """t as [n, d] once it is on a device, contiguous and 16-byte aligned."""
    _dev(t, name, dtype=t.dtype)
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: the base address must be 16-byte aligned")
    return t.view(t.shape[0], d)


def distance_correlation(x, z, out=None) -> DistanceCorrelation:
    """The sample distance correlation between the raw inputs x (float32 [n, ...]) and the cut z (bf16 [n, ...]), both
    flattened per sample to a multiple of 64 elements: slk_dcor, the biased (V-statistic) form that NoPeek reports,
    with Gram-based float32 distances and the resolution rule of include/slk.h. 0 means independent, 1 a similarity
    transform. The metric alone: DcorLoss below adds its gradient to a cut gradient.

    Three launches on x's current stream, no host sync (the result object syncs on first access) and no allocation
    once the workspace for this (device, n) exists, so a call can be captured in a HIP graph: pass out= (f32 [4]) then
    and read result.values after a replay. For a noisy cut, apply your own CutNoise first and pass its output."""
    dx, dz = _dcor_width(x, "x", torch.float32), _dcor_width(z, "z", torch.bfloat16)
    x2, z2 = _dcor_rows(x, "x", dx), _dcor_rows(z, "z", dz)
    n = int(x2.shape[0])
    if int(z2.shape[0]) != n:
        raise ValueError(f"z: expected {n} samples like x, got {z2.shape[0]}")
    if z.device != x.device:
        raise ValueError(f"z: on {z.device}, x is on {x.device}")
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=x.device)
    else:
        _dev(out, "out", (4,), torch.float32)
        if out.device != x.device:
            raise ValueError(f"out: on {out.device}, x is on {x.device}")
        if out.data_ptr() % 16:
            raise ValueError("out: the base address must be 16-byte aligned")
    if n == 0:
        raise ValueError("distance_correlation: an empty batch has no statistic")
    key = (x.device, n)
    ws = _DCOR_WORKSPACES.get(key)
    if ws is None:
        ws = _DCOR_WORKSPACES[key] = torch.empty(ops.dcor_workspace_bytes(n), dtype=torch.uint8, device=x.device)
    ops.dcor(x2, z2, ws, out)
    return DistanceCorrelation(out)


# ------------------------------------------------------------------------------------ training against leakage
_DCOR_GRAD_WORKSPACES: dict = {}   # (device, n) -> slk_dcor_grad's workspace, like _DCOR_WORKSPACES


class DcorLoss:
    """The NoPeek term (Vepakomma et al.) on the K5 cut, as a config of one entry, slk_dcor_grad: the client trains on
    task loss + alpha * dCor^2(x, cut) by adding alpha * d dCor^2 / d cut to the cut gradient it back-propagates. The
    term is client-local (x and the raw cut never leave the client) and inherits the metric's rule (include/slk.h,
    "Distance correlation gradient"). squared=False differentiates dCor itself.

    `alpha` lives in a device f32[1] the kernel reads, so a captured HIP graph follows `set_alpha` without being
    recaptured; `squared` is passed by value: a captured graph keeps it, and there is no setter."""

    def __init__(self, alpha: float, squared: bool = True, device="cuda"):
        self.alpha = self._checked_alpha(alpha)
        if not isinstance(squared, bool):
            raise ValueError(f"DcorLoss: squared={squared!r}; expected a bool")
        self.squared = squared
        self.alpha_value = torch.full((1,), self.alpha, dtype=torch.float32, device=device)

    @staticmethod
    def _checked_alpha(alpha) -> float:
        if not _number(alpha) or not 0.0 <= alpha < math.inf:   # NaN fails this too
            raise ValueError(f"DcorLoss: alpha={alpha!r}; expected a finite number >= 0")
        return float(alpha)

    def to(self, device) -> "DcorLoss":
        """Move the scalar (a no-op on its own device); captured graphs hold its address, so move a DcorLoss before
        the first step only."""
        if self.alpha_value.device != torch.device(device):
            self.alpha_value = self.alpha_value.to(device)
        return self

    def set_alpha(self, alpha: float) -> None:
        """Overwrite the weight in place: an asynchronous device write on the current stream, so the next launch —
        eager or a replay of an already captured graph — runs at `alpha`."""
        self.alpha = self._checked_alpha(alpha)
        self.alpha_value.fill_(self.alpha)

    def __repr__(self):
        return f"DcorLoss(alpha={self.alpha}, squared={self.squared})"

    def add_grad(self, x, cut, dcut, out=None, stats=None):
        """out = dcut + alpha * d dCor^2(x, cut) / d cut; out=None writes dcut in place. x is float32 [n, ...], cut and
        dcut bf16 [n, ...] of one shape, flattened per sample to multiples of 64 elements. `stats` (f32 [4]) receives
        the metric's four values (DistanceCorrelation(stats) reads them). Six launches on x's current stream, no host
        sync, and no allocation once the workspace for this (device, n) exists. Returns out."""
        dx, dz = _dcor_width(x, "x", torch.float32), _dcor_width(cut, "cut", torch.bfloat16)
        x2, z2 = _dcor_rows(x, "x", dx), _dcor_rows(cut, "cut", dz)
        n = int(x2.shape[0])
        if n == 0:
            raise ValueError("DcorLoss.add_grad: an empty batch has no statistic")
        out = dcut if out is None else out
        rows = [z2]
        for t, name in ((dcut, "dcut"), (out, "out")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
                raise TypeError(f"{name}: expected a {torch.bfloat16} torch.Tensor")
            if tuple(t.shape) != tuple(cut.shape):
                raise ValueError(f"{name}: expected {tuple(cut.shape)} like cut, got {tuple(t.shape)}")
            rows.append(_dcor_rows(t, name, dz))
        if int(z2.shape[0]) != n:
            raise ValueError(f"cut: expected {n} samples like x, got {z2.shape[0]}")
        if stats is None:
            stats = torch.empty(4, dtype=torch.float32, device=x.device)
        else:
            _dev(stats, "stats", (4,), torch.float32)
            if stats.data_ptr() % 16:
                raise ValueError("stats: the base address must be 16-byte aligned")
        for t, name in ((cut, "cut"), (dcut, "dcut"), (out, "out"), (stats, "stats"), (self.alpha_value, "alpha")):
            if t.device != x.device:
                raise ValueError(f"{name}: on {t.device}, x is on {x.device}")
        key = (x.device, n)
        ws = _DCOR_GRAD_WORKSPACES.get(key)
        if ws is None:
            ws = _DCOR_GRAD_WORKSPACES[key] = torch.empty(ops.dcor_grad_workspace_bytes(n), dtype=torch.uint8,
                                                          device=x.device)
        ops.dcor_grad(x2, z2, rows[1], self.alpha_value, self.squared, ws, rows[2], stats)
        return out


def check_dcor_loss(loss):
    """A trainer's leak_loss argument: a DcorLoss or None."""
    if loss is not None and not isinstance(loss, DcorLoss):
        raise TypeError(f"expected splitcnn.privacy.DcorLoss or None, got {type(loss).__name__}")
    return loss
