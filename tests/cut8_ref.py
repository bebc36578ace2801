"""Host restatement of the FP8 cut record rule (include/slk.h, "FP8 cut records") and the input generator of its
tests. Independent of the kernels' arithmetic: numpy / torch on the CPU, torch's float8_e4m3fn / float8_e5m2 casts
as the rounding oracle, the scale exponent found by search (no bit tricks), float32 products of a value and a power
of two (exact) exactly where the rule has them."""
import numpy as np
import torch

SAMPLE = 16384
HEADER = 16
RECORD = HEADER + SAMPLE
E_MIN, E_MAX = -100, 127
POISON = 0x7FFFFFFF
BF16_MAX = 255.0 * 2.0 ** 120   # 0x7F7F
# name -> (fmt word, torch dtype, F_MAX, mantissa bits m, exponent of the smallest normal emin)
FORMATS = {"e4m3": (0, torch.float8_e4m3fn, 448.0, 3, -6), "e5m2": (1, torch.float8_e5m2, 57344.0, 2, -14)}


def from_bits(bits) -> torch.Tensor:
    """uint16 array -> bf16 tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def to_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def finite_values(name: str) -> np.ndarray:
    """Every finite value of the format, float64, one per code (both zeros), with its codes: (values, codes)."""
    dt = FORMATS[name][1]
    codes = np.arange(256, dtype=np.uint8)
    v = torch.from_numpy(codes.copy()).view(dt).float().double().numpy()
    keep = np.isfinite(v)
    return v[keep], codes[keep]


def find_e(amax: float, fmax: float) -> int:
    """The smallest integer e >= E_MIN with amax * 2^-e <= fmax, by search (float64: exact for these operands)."""
    if amax == 0.0:
        return 0
    e = E_MIN
    while amax * 2.0 ** -e > fmax:
        e += 1
    return e


def encode(x: torch.Tensor, name: str) -> np.ndarray:
    """bf16 [n, 16384] (any trailing shape of 16,384 elements) -> uint8 [n, 16400]."""
    fmt, dt, fmax, _, _ = FORMATS[name]
    x = x.detach().cpu().reshape(x.shape[0], SAMPLE)
    rec = np.zeros((x.shape[0], RECORD), dtype=np.uint8)
    for i in range(x.shape[0]):
        xf = x[i].float()
        head = rec[i, :HEADER].view(np.uint32)
        head[1] = fmt
        if not bool(torch.isfinite(xf).all()):
            head[0] = POISON
            continue
        e = find_e(float(xf.abs().max().double()), fmax)
        head[0] = np.int32(e).view(np.uint32)
        y = xf * (2.0 ** -e)   # float32 times a power of two
        rec[i, HEADER:] = y.to(dt).view(torch.uint8).numpy()
    return rec


def decode(rec: np.ndarray, name: str):
    """uint8 [n, 16400] -> (bf16 [n, 16384], err flag 0 / 1)."""
    fmt, dt, _, _, _ = FORMATS[name]
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    out = torch.full((rec.shape[0], SAMPLE), float("nan"), dtype=torch.bfloat16)
    flag = 0
    for i in range(rec.shape[0]):
        head = rec[i, :HEADER].copy().view(np.uint32)
        e = int(head[0].view(np.int32))
        if int(head[1]) != fmt or head[2] or head[3] or (e != POISON and not E_MIN <= e <= E_MAX):
            flag = 1
            continue
        if e == POISON:
            continue
        codes = torch.from_numpy(rec[i, HEADER:].copy())
        c = codes.view(dt).float().double()
        v = c * (2.0 ** e)   # float64: exact, and 448 * 2^127 does not overflow
        # a finite code never becomes inf: at or past 2^128 it is the largest finite bf16 of its sign
        v = torch.where(torch.isfinite(c), v.clamp(-BF16_MAX, BF16_MAX), v)
        out[i] = v.to(torch.bfloat16)
        assert bool(((out[i].double() == v) | torch.isnan(v)).all())   # the rest is exact
    return out, flag


def roundtrip(x: torch.Tensor, name: str) -> torch.Tensor:
    """decode(encode(x)) in x's shape."""
    out, flag = decode(encode(x, name), name)
    assert flag == 0
    return out.reshape(x.shape)


def record_e(rec: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rec[:, :4]).view(np.int32).reshape(-1)


MALFORMED = ("fmt", "reserved", "e_low", "e_high")


def malform(rec_row: np.ndarray, kind: str) -> np.ndarray:
    """A copy of one record made malformed in one way."""
    r = rec_row.copy()
    head = r[:HEADER].view(np.uint32)
    if kind == "fmt":
        head[1] ^= 1
    elif kind == "reserved":
        r[13] = 1
    elif kind == "e_low":
        head[0] = np.int32(E_MIN - 1).view(np.uint32)
    elif kind == "e_high":
        head[0] = np.int32(E_MAX + 1).view(np.uint32)
    else:
        raise ValueError(kind)
    return r


# ---------------------------------------------------------------------------------------------- inputs
def _random_bits(g, amax_bits: int, signed: bool = True) -> np.ndarray:
    """16,384 bf16 values of magnitude bits <= amax_bits — uniform in the bits, so log-uniform in value over up to
    30 binades below amax — with amax planted once (negative when signed)."""
    lo = max(0, amax_bits - 30 * 128)
    mag = torch.randint(lo, amax_bits + 1, (SAMPLE,), generator=g).numpy().astype(np.uint16)
    if signed:
        mag |= (torch.randint(0, 2, (SAMPLE,), generator=g).numpy().astype(np.uint16) << 15)
    mag[int(torch.randint(0, SAMPLE, (1,), generator=g))] = amax_bits | (0x8000 if signed else 0)
    return mag


def _sweep(g, name: str, shift: int) -> np.ndarray:
    """Every finite value of the format times 2^shift, the midpoints of neighbouring values (exact ties), both
    zeros, and amax = F_MAX * 2^shift, so that e = shift; the rest random below amax."""
    vals, _ = finite_values(name)
    pos = np.unique(np.abs(vals))
    mids = (pos[:-1] + pos[1:]) / 2
    planted = np.concatenate([vals, mids, -mids]) * 2.0 ** shift
    t = torch.from_numpy(planted).to(torch.bfloat16)
    assert np.array_equal(t.double().numpy(), planted)   # all exactly representable
    amax_bits = int(to_bits(torch.tensor([FORMATS[name][2] * 2.0 ** shift], dtype=torch.bfloat16))[0])
    bits = _random_bits(g, amax_bits)
    bits[100:100 + len(planted)] = to_bits(t)
    bits[0] = amax_bits
    return bits


def samples():
    """[(name, uint16 bits [16384])]: the generator's set."""
    g = torch.Generator().manual_seed(2024)
    out = []
    # amax on both sides of the F_MAX boundary (mantissa 0x60 | 0x61), at the binade's ends, at several exponents;
    # exponent field 20 is 2^-107, below 2^-100, where the clamp binds; 254 | 0x7f is the largest finite bf16
    for ex in (20, 60, 127, 140, 254):
        for man in (0x00, 0x60, 0x61, 0x7f):
            out.append((f"amax_ex{ex}_man{man:02x}", _random_bits(g, (ex << 7) | man)))
    out.append(("subnormal_amax", _random_bits(g, 0x0055)))
    out.append(("all_zero", np.zeros(SAMPLE, dtype=np.uint16)))
    out.append(("non_negative", _random_bits(g, (130 << 7) | 0x23, signed=False)))
    out.append(("sweep_e4m3", _sweep(g, "e4m3", 3)))
    out.append(("sweep_e5m2", _sweep(g, "e5m2", -9)))
    nan = _random_bits(g, (127 << 7) | 0x10)
    nan[777] = 0x7FC0
    out.append(("has_nan", nan))
    inf = _random_bits(g, (127 << 7) | 0x10)
    inf[16383] = 0xFF80
    out.append(("has_inf", inf))
    return out


def sample_tensor() -> torch.Tensor:
    """The whole set as bf16 [N, 16384] (CPU)."""
    return from_bits(np.stack([b for _, b in samples()]))
