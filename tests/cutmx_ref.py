"""Host restatement of the MX cut record rule (include/slk.h, "MX cut records") and the input generator of its tests.
Independent of the kernels' arithmetic: numpy / torch on the CPU in float64, the block exponent found by search (no
bit tricks), e2m1 rounded by nearest-of-eight with ties to the even mantissa, e4m3 by torch's float8_e4m3fn cast of
the float32 product of a value and a power of two (exact). `variant=` selects one of the deliberately wrong rules
that tests/test_cutmx_cpu.py shows the comparisons catch."""
import numpy as np
import torch

SAMPLE, BLOCK = 16384, 32
BLOCKS = SAMPLE // BLOCK            # 512
HEADER = 16
PAYLOAD = HEADER + BLOCKS           # 528
E_MIN = -100
BF16_MAX = 255.0 * 2.0 ** 120       # 0x7F7F
E2M1_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])   # index = exp << 1 | man
# name -> (fmt, F_MAX, mantissa bits m, exponent of the smallest normal emin, bits per code, largest element exponent)
FORMATS = {"e2m1": (0, 6.0, 1, 0, 4, 2), "e4m3": (1, 448.0, 3, -6, 8, 8)}
RECORD = {"e2m1": PAYLOAD + SAMPLE // 2, "e4m3": PAYLOAD + SAMPLE}   # 8720, 16912
VARIANTS = ("ocp_floor", "swap_nibbles", "ties_away", "per_sample", "bias128")


def from_bits(bits) -> torch.Tensor:
    """uint16 array -> bf16 tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def to_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def find_e(amax: np.ndarray, fmax: float) -> np.ndarray:
    """Per entry the smallest integer e >= E_MIN with amax * 2^-e <= fmax, by search; 0 where amax == 0."""
    amax = np.asarray(amax, dtype=np.float64)
    e = np.full(amax.shape, E_MIN, dtype=np.int64)
    while True:
        over = amax * np.exp2(-e.astype(np.float64)) > fmax
        if not over.any():
            break
        e[over] += 1
    e[amax == 0] = 0
    return e


def e2m1_codes(y: np.ndarray, negative: np.ndarray, ties_away: bool = False) -> np.ndarray:
    """float64 y with |y| <= 6 (beyond it: saturated to 6, only the OCP-floor variant gets there) -> 4-bit codes:
    the nearest of the eight magnitudes, a tie to the one with the even mantissa (away from zero in the wrong
    variant); the sign bit is that of the source element, also for a zero result."""
    a = np.minimum(np.abs(y), 6.0)
    d = np.abs(a[..., None] - E2M1_GRID)
    lo = d.argmin(-1)                       # the first minimum: the lower neighbour on a tie
    hi = np.minimum(lo + 1, 7)
    tie = np.take_along_axis(d, hi[..., None], -1)[..., 0] == np.take_along_axis(d, lo[..., None], -1)[..., 0]
    tie &= hi != lo
    idx = np.where(tie & ((lo & 1 == 1) | ties_away), hi, lo)
    return (idx | (negative.astype(np.int64) << 3)).astype(np.uint8)


def e4m3_codes(y32: torch.Tensor, ties_away: bool = False) -> np.ndarray:
    c = y32.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    if ties_away:   # a tie that went down to the even code goes up instead
        down = torch.from_numpy(c).view(torch.float8_e4m3fn).float().double().numpy()
        up = torch.from_numpy((c + 1).astype(np.uint8)).view(torch.float8_e4m3fn).float().double().numpy()
        y = y32.double().numpy()
        fix = np.isfinite(up) & (np.abs(y) > np.abs(down)) & (np.abs(up) - np.abs(y) == np.abs(y) - np.abs(down))
        c[fix] += 1
    return c


def block_exponents(x64: np.ndarray, name: str, variant=None):
    """x64 float64 [n, 512, 32] -> (e int64 [n, 512], poisoned bool [n, 512])."""
    _, fmax, _, _, _, emax = FORMATS[name]
    poisoned = ~np.isfinite(x64).all(-1)
    amax = np.where(poisoned[..., None], 0.0, np.abs(np.nan_to_num(x64, nan=0.0, posinf=0.0, neginf=0.0))).max(-1)
    if variant == "per_sample":
        amax = np.broadcast_to(amax.max(-1, keepdims=True), amax.shape)
    if variant == "ocp_floor":
        e = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))).astype(np.int64) - emax, 0)
        e = np.maximum(e, E_MIN)
    else:
        e = find_e(amax, fmax)
    return e, poisoned


def encode(x: torch.Tensor, name: str, variant=None) -> np.ndarray:
    """bf16 [n, ...] of 16,384 elements per row -> uint8 [n, R]."""
    assert variant is None or variant in VARIANTS
    fmt, fmax, _, _, bits, _ = FORMATS[name]
    n = x.shape[0]
    xb = x.detach().cpu().reshape(n, BLOCKS, BLOCK)
    x64 = xb.double().numpy()
    e, poisoned = block_exponents(x64, name, variant)
    rec = np.zeros((n, RECORD[name]), dtype=np.uint8)
    head = rec[:, :HEADER].view(np.uint32)
    head[:, 0], head[:, 1] = BLOCK, 0x10 + fmt
    rec[:, HEADER:PAYLOAD] = np.where(poisoned, 0xFF, e + (128 if variant == "bias128" else 127)).astype(np.uint8)
    negative = np.signbit(x64)
    clean = np.where(poisoned[..., None], 0.0, x64)
    if name == "e2m1":
        c = e2m1_codes(clean * np.exp2(-e.astype(np.float64))[..., None], negative, variant == "ties_away")
        c[poisoned] = 0
        c = c.reshape(n, SAMPLE // 2, 2)
        first, second = (1, 0) if variant == "swap_nibbles" else (0, 1)
        rec[:, PAYLOAD:] = c[..., first] | (c[..., second] << 4)
    else:
        scale = torch.from_numpy(np.exp2(-e.astype(np.float64))).float()[..., None]
        y32 = torch.from_numpy(clean).float() * scale   # float32 times a power of two
        if variant == "ocp_floor":
            y32 = y32.clamp(-fmax, fmax)
        c = e4m3_codes(y32, variant == "ties_away").reshape(n, BLOCKS, BLOCK)
        c[poisoned] = 0
        rec[:, PAYLOAD:] = c.reshape(n, SAMPLE)
    return rec


def code_values(name: str) -> np.ndarray:
    """float64 value of every code (16 or 256 entries; NaN for e4m3's two NaN codes)."""
    if name == "e2m1":
        return np.concatenate([E2M1_GRID, -E2M1_GRID])
    return torch.arange(256, dtype=torch.int16).to(torch.uint8).view(torch.float8_e4m3fn).float().double().numpy()


def decode(rec: np.ndarray, name: str):
    """uint8 [n, R] -> (bf16 [n, 16384], err flag 0 / 1)."""
    fmt = FORMATS[name][0]
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    n = rec.shape[0]
    assert rec.shape[1] == RECORD[name]
    head = rec[:, :HEADER].copy().view(np.uint32)
    bad_head = (head[:, 0] != BLOCK) | (head[:, 1] != 0x10 + fmt) | (head[:, 2] != 0) | (head[:, 3] != 0)
    sb = rec[:, HEADER:PAYLOAD].astype(np.int64)
    bad_scale = (sb < E_MIN + 127) & ~bad_head[:, None]
    nan_block = bad_head[:, None] | bad_scale | (sb == 0xFF)
    pay = rec[:, PAYLOAD:]
    codes = np.stack([pay & 0xF, pay >> 4], -1).reshape(n, SAMPLE) if name == "e2m1" else pay
    c = code_values(name)[codes].reshape(n, BLOCKS, BLOCK)
    v = c * np.exp2((sb - 127).astype(np.float64))[..., None]   # float64: exact, and 448 * 2^127 does not overflow
    v = np.where(np.isfinite(c), np.clip(v, -BF16_MAX, BF16_MAX), v)
    v = np.where(nan_block[..., None], np.nan, v)
    out = torch.from_numpy(v.reshape(n, SAMPLE)).to(torch.bfloat16)
    ok = (out.double().numpy() == v.reshape(n, SAMPLE)) | np.isnan(v.reshape(n, SAMPLE))
    assert ok.all()   # the rest is exact
    bits = to_bits(out)
    bits[np.isnan(v.reshape(n, SAMPLE))] = 0x7FC0
    return from_bits(bits), int(bad_head.any() or bad_scale.any())


def roundtrip(x: torch.Tensor, name: str, variant=None) -> torch.Tensor:
    """decode(encode(x)) in x's shape."""
    out, flag = decode(encode(x, name, variant), name)
    assert flag == 0
    return out.reshape(x.shape)


def scale_bytes(rec: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rec[:, HEADER:PAYLOAD])


def block_payload(rec: np.ndarray, name: str, k: int) -> np.ndarray:
    w = BLOCK * FORMATS[name][4] // 8
    return rec[:, PAYLOAD + k * w:PAYLOAD + (k + 1) * w]


# ---------------------------------------------------------------------------------------------- inputs
def _random_block(g, amax_bits: int, signed: bool = True) -> np.ndarray:
    """32 bf16 values of magnitude bits <= amax_bits, uniform in the bits over up to 12 binades below amax, with amax
    planted once."""
    lo = max(0, amax_bits - 12 * 128)
    mag = torch.randint(lo, amax_bits + 1, (BLOCK,), generator=g).numpy().astype(np.uint16)
    if signed:
        mag |= (torch.randint(0, 2, (BLOCK,), generator=g).numpy().astype(np.uint16) << 15)
    mag[int(torch.randint(0, BLOCK, (1,), generator=g))] = amax_bits | (0x8000 if signed and amax_bits & 1 else 0)
    return mag


def _spread(g, signed=True) -> np.ndarray:
    """One sample whose 512 blocks have amax exponents spread over the whole bf16 range (fields 0..254, every
    mantissa class around both formats' F_MAX boundaries)."""
    mans = (0x00, 0x40, 0x41, 0x60, 0x61, 0x7f)
    blocks = [_random_block(g, max(1, ((k * 255) // BLOCKS << 7) | mans[k % 6]), signed) for k in range(BLOCKS)]
    return np.concatenate(blocks)


def _planted(g, name: str, shifts) -> np.ndarray:
    """Every grid point and every midpoint of neighbouring grid points (exact ties) of the format times 2^shift, both
    signs, in blocks whose amax is F_MAX * 2^shift so that e = shift; the other blocks random."""
    fmax = FORMATS[name][1]
    pos = np.unique(np.abs(code_values(name)[np.isfinite(code_values(name))]))
    mids = (pos[:-1] + pos[1:]) / 2
    vals = np.concatenate([pos, -pos, mids, -mids])
    row = _spread(g)
    k = 3
    for shift in shifts:
        for i in range(0, len(vals), BLOCK - 1):
            chunk = vals[i:i + BLOCK - 1] * 2.0 ** shift
            blk = np.concatenate([[fmax * 2.0 ** shift], chunk, np.zeros(BLOCK - 1 - len(chunk))])
            t = torch.from_numpy(blk).to(torch.bfloat16)
            assert np.array_equal(t.double().numpy(), blk)   # all exactly representable
            row[k * BLOCK:(k + 1) * BLOCK] = to_bits(t)
            k += 5
    assert k < BLOCKS + 5
    return row


def _boundaries(g) -> np.ndarray:
    """amax exactly F_MAX * 2^e and one ulp above, for both formats, at several exponents (the ends of the range
    included); the bf16-subnormal block; all-zero, all -0 and mixed-zero blocks; the all-0x7F7F block."""
    row = _spread(g)
    k = 1
    for ex in (1, 24, 27, 30, 100, 127, 130, 200, 254):
        for man in (0x40, 0x41, 0x60, 0x61, 0x00, 0x7f):
            if (ex << 7 | man) < 0x7f80:
                row[k * BLOCK:(k + 1) * BLOCK] = _random_block(g, (ex << 7) | man)
                k += 3
    row[k * BLOCK:(k + 1) * BLOCK] = _random_block(g, 0x0055)             # bf16 subnormals only
    row[(k + 2) * BLOCK:(k + 3) * BLOCK] = 0                               # +0
    row[(k + 4) * BLOCK:(k + 5) * BLOCK] = 0x8000                          # -0
    row[(k + 6) * BLOCK:(k + 7) * BLOCK] = np.tile([0x0000, 0x8000], 16)   # both zeros
    row[(k + 8) * BLOCK:(k + 9) * BLOCK] = 0x7F7F                          # rounds to 2^128: the top clamp
    row[(k + 10) * BLOCK:(k + 11) * BLOCK] = np.tile([0x7F7F, 0xFF7F, 0x7F00, 0x0001], 8)
    assert k + 11 <= BLOCKS
    return row


def model_rows():
    """(cut, dcut) bits of sample 0 of the seeded widened model's first step at B = 2, by the float64 CPU oracle with
    the bf16 roundings on (oracle/wide_step.py): a real post-ReLU cut and its signed, dropout-masked gradient."""
    from oracle import wide_step as W
    from splitcnn.wide import SyntheticCIFAR, init_wide_models
    a, b = init_wide_models(seed=0)
    P = {k: v.detach().double().numpy() for k, v in list(a.state_dict().items()) + list(b.state_dict().items())}
    x, y = SyntheticCIFAR(23).batch(2)
    cut, _ = W.client_forward(P, x.double().numpy())
    s = W.server_step(P, cut, y.numpy(), W.dropout_keep(0, 0, 2))
    return tuple(to_bits(torch.from_numpy(np.ascontiguousarray(t[0])).to(torch.bfloat16)).reshape(SAMPLE)
                 for t in (cut, s["dcut"]))


def samples():
    """[(name, uint16 bits [16384])]: the generator's set, a dozen samples."""
    g = torch.Generator().manual_seed(4242)
    out = [("spread_signed", _spread(g)), ("spread_non_negative", _spread(g, signed=False)),
           ("planted_e2m1", _planted(g, "e2m1", (0, -7, 60, -100))), ("planted_e4m3", _planted(g, "e4m3", (3, -100, 100))),
           ("boundaries", _boundaries(g)), ("all_zero", np.zeros(SAMPLE, dtype=np.uint16))]
    cut, dcut = model_rows()
    out += [("model_cut", cut), ("model_cut_gradient", dcut)]
    grad = torch.randn(SAMPLE, generator=g) * 1e-4 * torch.exp2(torch.randn(SAMPLE, generator=g) * 3)
    out.append(("gradient_like", to_bits(grad.to(torch.bfloat16))))
    for nm, pos, val in (("has_nan", 777, 0x7FC0), ("has_pos_inf", 16383, 0x7F80), ("has_neg_inf", 0, 0xFF80)):
        row = _spread(g)
        row[pos] = val
        out.append((nm, row))
    three = _spread(g)
    three[40], three[5000], three[9001] = 0xFFC1, 0x7F80, 0xFF80   # three poisoned blocks of one sample
    out.append(("three_non_finite", three))
    return out


def sample_tensor() -> torch.Tensor:
    """The whole set as bf16 [N, 16384] (CPU)."""
    return from_bits(np.stack([b for _, b in samples()]))
