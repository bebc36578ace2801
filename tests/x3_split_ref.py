"""Test infrastructure: the x3 conv2 kernels' documented arithmetic (csrc/slk_x3.hip, head comment) restated in
float64, and operand classes on which that arithmetic is EXACT although the operands' low halves are not zero.

The contract. Every f32 operand v is scaled by an exact power of two 2^s (x3_exp of the sample's, or of W2's,
max |.|: the maximum lands in [2^13, 2^14)) and split into h = f16(v 2^s) and l = f16(v 2^s - h), both round to
nearest even. A product a b is formed as h_a h_b + h_a l_b + l_a h_b by three f16 MFMAs into one f32 accumulator;
l_a l_b is dropped by design. `split` states the split through float16 casts, `three_term` the three kept terms
of the forward, the input gradient and the weight gradient (tests/ref64.py supplies the float64 convolutions, the
routing and the route).

What makes it exact. In the scaled domain f16's ulp at the maximum is 8. Three classes have l != 0 and still
give f32 sums without a rounding:
  14-bit   nonzero values are integers uniform in [2^13, 2^14) (signed where the operand is): h is a multiple of 8,
           l in [-4, 4]; one value in 8 is an exact tie (v = 4 mod 8: pins round-to-nearest-EVEN), 7 in 8 have l != 0.
  18-bit   n 2^-4 with n uniform in [2^17, 2^18): l takes 129 values, down to 2^-4; every addend is a multiple of
           2^-4 times the partner's granule. (6 fractional bits overflow the bound below; 4 are kept.)
  both     both operands are m 2^11 + r, m in {2, 3}, r in {-1, 0, 1} (or 0): h = m 2^11, l = r, every kept
           addend is a multiple of 2^11, and the expected value is the three-term sum, sum (a b - r_a r_b), NOT
           float64's sum a b: this class pins the dropped term. A kernel that adds the fourth MFMA changes this
           expectation on purpose.
When only one operand carries an l its partner is an exact f16 value (small integers, +-1; l = 0): the three terms
are then the whole product and the expectation is plain float64.
`assert_exact` bounds, per output, the sum of the absolute values of ALL kept addends (and of the bias) below
2^24 in units of the finest addend granule (the largest power of two that divides every addend, from the operands'
own granules). Every partial sum, in any order, is then a multiple of that granule below 2^24 granules: an f32
value, so no addition rounds. This rests on the MFMA adder losing no bits while addends and sums fit 24 bits
- with addends up to 14 binades apart in one chain here, against 7 in tests/test_x3_exact_gpu.py.
Densities are inputs chosen so that the bound holds (float64 on the CPU, B = 5 unless noted): forward 14-bit act
at 0.15 against +-1 weights at 0.3: 2^18.6, 18-bit: 2^22.6; forward / dgrad with a dense signed 14-bit W2 against
{1, 2, 3} at 0.15 / 0.3: 2^20.8 / 2^21.3; weight gradient 14-bit act 0.15, +-1 dpooled 0.3: 2^19.4 at B = 5 and
2^23.5 at B = 130, hence 0.05 / 0.05 there (2^19.9).

`decode_act16` reads the act16 images from the layout comment in csrc/slk_x3.hip and from nothing else."""
import numpy as np
import torch
import torch.nn.functional as F

from ref64 import dgrad64, route64, wgrad64

X3_SMAX = 126
LIMIT = 2.0 ** 24
ACT16_SAMPLE = 86528          # bytes: an h plane then an l plane of 676 pixels x 32 ci f16


# ----------------------------------------------------------------------------- scale and split
def x3_exp(amax):
    """s with amax 2^s in [2^13, 2^14): frexp, 14 - e, clamped at 126; 0 for a zero or non-finite maximum."""
    a = np.asarray(amax, dtype=np.float32)
    ok = np.isfinite(a) & (a > 0)
    _, e = np.frexp(np.where(ok, a, np.float32(1)))
    return np.where(ok, np.minimum(14 - e.astype(np.int64), X3_SMAX), 0).astype(np.int64)


def _chop_np(a):
    """f32 -> the f32 holding its 11 leading significant bits, the rest cut off (round toward zero; normal f16
    range only): what a truncating f16 conversion would give."""
    return (a.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)


def split_np(v, s, trunc=False):
    """numpy statement of the split: v f32 [B, ...], s int [B] -> (h, l) float16 in the scaled domain.
    trunc = True is the WRONG variant that converts by truncation."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    sc = np.ldexp(np.float32(1), np.asarray(s, dtype=np.int32)).astype(np.float32)
    a = (v * sc.reshape((-1,) + (1,) * (v.ndim - 1))).astype(np.float32)
    if trunc:
        h = _chop_np(a).astype(np.float16)
        return h, _chop_np(a - h.astype(np.float32)).astype(np.float16)
    h = a.astype(np.float16)
    return h, (a - h.astype(np.float32)).astype(np.float16)


def split(v, amax=None, per_sample=True, trunc=False):
    """torch statement of the split (any device): v f32 -> (h, l, rem) float64 in v's own (unscaled) domain with
    h + l + rem == v. per_sample: one scale per v[b] from amax[b] (default: the row's max |v|); otherwise one
    scale from max |v| (W2)."""
    v = v.float()
    rows = v.reshape(v.shape[0], -1) if per_sample else v.reshape(1, -1)
    am = rows.abs().max(dim=1).values if amax is None else amax.float().reshape(-1)
    # the powers of two are made on the host: an exact ldexp is not promised on every device
    s = x3_exp(am.cpu().numpy()).astype(np.int32)
    a = rows * torch.from_numpy(np.ldexp(np.float32(1), s)).to(v.device)[:, None]
    assert torch.equal(a.double(), rows.double() * torch.from_numpy(np.ldexp(1.0, s)).to(v.device)[:, None])
    if trunc:
        chop = lambda t: (t.view(torch.int32) & -8192).view(torch.float32)          # noqa: E731
        h = chop(a).half()
        l = chop(a - h.float()).half()
    else:
        h = a.half()
        l = (a - h.float()).half()
    un = torch.from_numpy(np.ldexp(1.0, -s)).to(v.device)[:, None]
    h64, l64 = h.double() * un, l.double() * un
    return h64.reshape(v.shape), l64.reshape(v.shape), (rows.double() - h64 - l64).reshape(v.shape)


# ----------------------------------------------------------------------------- the three kept terms
def conv64(act, W2):
    """conv2d(act, W2) in float64, no bias, no ReLU: [B,32,26,26] -> [B,64,24,24] (ref64.conv_relu64's GEMM)."""
    B = act.shape[0]
    cols = F.unfold(act.double(), 3)
    return torch.matmul(W2.double().reshape(64, 288), cols).reshape(B, 64, 24, 24)


def _bilinear(op):
    if op == "fwd":
        return conv64                                    # a = act,      b = W2
    if op == "dgrad":
        return dgrad64                                   # a = routed dY, b = W2
    if op == "wgrad":
        return lambda a, b: wgrad64(a, b)[0]             # a = act,      b = routed dY
    raise ValueError(op)


def three_term(a_h, a_l, b_h, b_l, op, drop=(), add_ll=False):
    """h_a h_b + h_a l_b + l_a h_b summed over the operation's K in float64. `drop` ("hl": h_a l_b, "lh": l_a h_b)
    and add_ll (the fourth term) are the WRONG variants the CPU tests show to be visible."""
    f = _bilinear(op)
    out = f(a_h, b_h)
    if "hl" not in drop:
        out = out + f(a_h, b_l)
    if "lh" not in drop:
        out = out + f(a_l, b_h)
    if add_ll:
        out = out + f(a_l, b_l)
    return out


def gran_exp(*ts):
    """e such that 2^e is the largest power of two dividing every nonzero element of the tensors (None if all zero)."""
    best = None
    for t in ts:
        t = t.double().reshape(-1)
        t = t[t != 0]
        if not t.numel():
            continue
        m, e = torch.frexp(t)
        M = (m.abs() * 2.0 ** 53).to(torch.int64)        # exact: a float64 mantissa is a 53-bit integer
        low = (M & -M).double().log2().round().to(torch.int64)
        g = int((e.to(torch.int64) - 53 + low).min())
        best = g if best is None else min(best, g)
    return best


def assert_exact(a_h, a_l, b_h, b_l, op, extra=None, what=""):
    """The exactness bound: per output, sum |kept addends| (+ |extra|, e.g. the bias) < 2^24 in units of the finest
    addend granule. Returns log2 of the largest sum in those units."""
    f = _bilinear(op)
    tot = f(a_h.abs(), b_h.abs()) + f(a_h.abs(), b_l.abs()) + f(a_l.abs(), b_h.abs())
    ga, gal, gb, gbl = gran_exp(a_h), gran_exp(a_l), gran_exp(b_h), gran_exp(b_l)
    cands = [x + y for x, y in ((ga, gb), (ga, gbl), (gal, gb)) if x is not None and y is not None]
    if extra is not None:
        tot = tot + extra.double().abs()
        if gran_exp(extra) is not None:
            cands.append(gran_exp(extra))
    if not cands:
        return float("-inf")
    units = float(tot.max()) / 2.0 ** min(cands)
    assert units < LIMIT, f"{what}: sum of |addends| is 2^{np.log2(max(units, 1)):.2f} granules: not exact in f32"
    return float(np.log2(max(units, 1.0)))


def assert_sum_exact(t, dims, what=""):
    """The same bound for a plain f32 sum of the elements of t over dims (db2, conv1's gradient sums)."""
    g = gran_exp(t)
    if g is None:
        return
    units = float(t.double().abs().sum(dim=dims).max()) / 2.0 ** g
    assert units < LIMIT, f"{what}: sum of |addends| is 2^{np.log2(units):.2f} granules: not exact in f32"


def kept_addends(a_h, a_l, b_h, b_l, op, idx):
    """Every kept addend of ONE output as a float64 vector (each an exact product of two f16 values), for the
    float32 emulation: idx = (b, co, y, x) of the forward, (b, ci, y, x) of the dgrad, (co, ci, ky, kx) of the
    weight gradient."""
    def prods(a, b):
        if op == "fwd":
            bb, co, y, x = idx
            return (a[bb, :, y:y + 3, x:x + 3].double() * b[co].double()).reshape(-1)
        if op == "dgrad":
            bb, ci, y, x = idx
            out = []
            for ky in range(3):
                for kx in range(3):
                    if 0 <= y - ky < 24 and 0 <= x - kx < 24:
                        out.append(a[bb, :, y - ky, x - kx].double() * b[:, ci, ky, kx].double())
            return torch.cat(out)
        co, ci, ky, kx = idx
        return (a[:, ci, ky:ky + 24, kx:kx + 24].double() * b[:, co].double()).reshape(-1)
    return torch.cat([prods(a_h, b_h), prods(a_h, b_l), prods(a_l, b_h)])


# ----------------------------------------------------------------------------- operand classes
def _where_p(g, shape, p, v):
    return torch.where(torch.rand(shape, generator=g) < p, v, torch.zeros(shape))


def _sign(g, shape, signed):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() if signed else torch.ones(shape)


def gen14(g, shape, p, signed):
    """nonzero with probability p: an integer uniform in [2^13, 2^14), with a random sign if signed."""
    v = torch.randint(2 ** 13, 2 ** 14, shape, generator=g).float() * _sign(g, shape, signed)
    return _where_p(g, shape, p, v)


def gen18(g, shape, p, signed):
    """nonzero with probability p: n 2^-4 with n uniform in [2^17, 2^18)."""
    v = torch.randint(2 ** 17, 2 ** 18, shape, generator=g).float() * 2.0 ** -4 * _sign(g, shape, signed)
    return _where_p(g, shape, p, v)


def gen_both(g, shape, p, signed):
    """nonzero with probability p: m 2^11 + r, m in {2, 3}, r in {-1, 0, 1}."""
    m = torch.randint(2, 4, shape, generator=g).float()
    r = torch.randint(-1, 2, shape, generator=g).float()
    return _where_p(g, shape, p, (m * 2048 + r) * _sign(g, shape, signed))


def gen_small(g, shape, p, mags, signed):
    """The l = 0 partner: nonzero with probability p, magnitude uniform over `mags` (small integers)."""
    mags = torch.tensor(mags, dtype=torch.float32)
    v = mags[torch.randint(0, len(mags), shape, generator=g)] * _sign(g, shape, signed)
    return _where_p(g, shape, p, v)


# ----------------------------------------------------------------------------- act16 images
def decode_act16(img_bytes, B):
    """The act16 images (uint8, 86,528 B a sample) -> (h, l) float64 [B, 32, 26, 26] in the scaled domain.
    Per sample an h plane then an l plane; a plane is [pixel p = 26 y + x][32 ci] f16, 64-byte pixels, and the
    16-byte chunk c8 (channels 8 c8 .. 8 c8 + 7) of a pixel is stored in slot c8 ^ (x & 2)."""
    raw = np.ascontiguousarray(np.asarray(img_bytes, dtype=np.uint8)).reshape(B, ACT16_SAMPLE)
    f = raw.view(np.float16).reshape(B, 2, 676, 4, 8)                       # sample, plane, pixel, slot, element
    x = np.arange(676) % 26
    slot = np.arange(4)[None, :] ^ (x & 2)[:, None]                         # [pixel, c8] -> slot
    v = np.take_along_axis(f, slot[None, None, :, :, None], axis=3)         # [B, 2, pixel, c8, j]
    v = v.reshape(B, 2, 26, 26, 32).transpose(0, 1, 4, 2, 3).astype(np.float64)
    return v[:, 0], v[:, 1]
