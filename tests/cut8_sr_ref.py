"""Host restatement of the stochastic rounding of the FP8 cut records (include/slk.h, "FP8 cut records: stochastic
rounding"), on top of tests/cut8_ref.py's helpers and sample set. Independent of csrc/slk_cut8.h's integer arithmetic:
y = x * 2^-e is held exactly in float64, the quantum comes from floor(log2 |y|), k and the fraction rem / 2^s from a
float64 division (exact: y has 8 significant bits), the random word from a numpy lowbias32, and the code of the chosen
neighbour from torch's float8 cast of its (representable) value."""
import numpy as np
import torch

import cut8_ref as R

NB = {name: 23 - R.FORMATS[name][3] for name in R.FORMATS}   # random bits the rule uses: 20 (e4m3), 21 (e5m2)
VARIANTS = (None, "nearest", "truncate", "shared_word")      # None is the rule; the rest are deliberately wrong


def lowbias32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def words(name: str, seed: int, step: int, rows) -> np.ndarray:
    """uint64 [len(rows), 16384] (values < 2^32): r_i of each global row under (seed, step)."""
    g = np.asarray(rows, dtype=np.uint64) & 0xFFFFFFFF
    rest = ((step & 0xFFFFFFFF) * 0x85EBCA77 + (seed & 0xFFFFFFFF) * 0xC2B2AE3D
            + (R.FORMATS[name][0] + 1) * 0x27D4EB2F) & 0xFFFFFFFF
    key = (((g * 0x9E3779B1) & 0xFFFFFFFF) + np.uint64(rest)) & 0xFFFFFFFF
    base = lowbias32(key)
    i = np.arange(R.SAMPLE, dtype=np.uint64)
    return lowbias32((base[:, None] + i[None, :] * 0x9E3779B1) & 0xFFFFFFFF)


def threshold(frac, nb: int) -> np.ndarray:
    """T of the rule from frac = rem / 2^s in [0, 1): floor(frac * 2^nb) (float64, exact for 8-bit rem)."""
    return np.floor(np.asarray(frac, dtype=np.float64) * 2.0 ** nb).astype(np.uint64)


def up_bits(frac, bits, nb: int) -> np.ndarray:
    """Whether a value a fraction `frac` of a quantum above its lower neighbour goes up under the nb random bits
    `bits`: bits + T carries out of nb bits."""
    return (np.asarray(bits, dtype=np.uint32) + threshold(frac, nb).astype(np.uint32)) >> np.uint32(nb)


def up(frac, r, nb: int) -> np.ndarray:
    """up_bits under the top nb bits of the random word r."""
    return up_bits(frac, (np.asarray(r, dtype=np.uint64) >> (32 - nb)).astype(np.uint32), nb)


def split(y: np.ndarray, name: str):
    """|y| = (k + frac) * quantum: (k, frac, quantum) in float64, the quantum from floor(log2 |y|) (1 for y = 0)."""
    _, _, _, m, emin = R.FORMATS[name]
    a = np.abs(y)
    _, ex = np.frexp(a)                       # a = f * 2^ex, f in [0.5, 1): floor(log2 a) = ex - 1
    quantum = 2.0 ** (np.maximum(ex - 1, emin) - m).astype(np.float64)
    quantum = np.where(a == 0, 1.0, quantum)
    units = a / quantum
    k = np.floor(units)
    return k, units - k, quantum


def encode(x: torch.Tensor, name: str, seed: int, step: int, row0: int = 0, variant=None) -> np.ndarray:
    """bf16 [n, 16384] -> uint8 [n, 16400]: cut8_ref.encode's records with the payload rounded stochastically."""
    assert variant in VARIANTS
    rec = R.encode(x, name)                   # headers, poisoned rows, and the nearest payload
    if variant == "nearest":
        return rec
    dt, nb = R.FORMATS[name][1], NB[name]
    x = x.detach().cpu().reshape(x.shape[0], R.SAMPLE)
    e = R.record_e(rec)
    for lo in range(0, x.shape[0], 64):
        rows = [i for i in range(lo, min(lo + 64, x.shape[0])) if e[i] != R.POISON]
        if not rows:
            continue
        xv = x[rows].double().numpy()
        y = xv * 2.0 ** -e[rows].astype(np.float64)[:, None]
        k, frac, quantum = split(y, name)
        r = words(name, seed, step, [row0 + i for i in rows])
        if variant == "shared_word":
            r = np.repeat(r[:, :1], R.SAMPLE, axis=1)
        u = np.zeros_like(k) if variant == "truncate" else up(frac, r, nb).astype(np.float64)
        v = np.copysign((k + u) * quantum, xv)   # representable; a zero keeps the sign of x
        codes = torch.from_numpy(v).float().to(dt)
        assert np.array_equal(codes.float().double().numpy(), v)
        rec[rows, R.HEADER:] = codes.view(torch.uint8).numpy()
    return rec


def roundtrip(x: torch.Tensor, name: str, seed: int, step: int, row0: int = 0, variant=None) -> torch.Tensor:
    """cut8_ref.decode(encode(x)) in x's shape."""
    out, flag = R.decode(encode(x, name, seed, step, row0, variant), name)
    assert flag == 0
    return out.reshape(x.shape)


def quanta(x: torch.Tensor, name: str) -> np.ndarray:
    """float64 [n, 16384]: the distance of each element's two neighbouring values, in x's units (finite rows only)."""
    x = x.detach().cpu().reshape(x.shape[0], R.SAMPLE)
    e = R.record_e(R.encode(x, name)).astype(np.float64)[:, None]
    return split(x.double().numpy() * 2.0 ** -e, name)[2] * 2.0 ** e


# Unbiasedness (CPU and GPU tests): one row repeated over UNBIASED_ROWS rows at row0 = 0. Every decoded value lies
# within one quantum, so by Hoeffding the mean of n of them leaves its expectation by more than t quanta with
# probability at most 2 exp(-2 n t^2) per element; over 16,384 elements 2 exp(-2 * 1024 * 0.11^2) * 16384 <= 1e-6.
UNBIASED_ROWS, UNBIASED_T = 1024, 0.11
UNBIASED_SAMPLE = "amax_ex127_man00"
UNBIASED_KEY = (5, 3)   # (seed, step)
assert 2 * np.exp(-2 * UNBIASED_ROWS * UNBIASED_T ** 2) * R.SAMPLE <= 1e-6
