"""GPU: the launch heads of the x3 conv2 kernels — the part of each launch before its first unit, where a workgroup
reads W2 once, takes max |W2| for the weight scale, stages the values in LDS and gathers its MFMA fragments from there
(forward, dgrad), or reduces the per-sample scale arrays (wgrad).

The other x3 tests cannot tell a weight that reached the wrong fragment slot from rounding noise, or (integer
operands) a wrong `lo` part from a right one: here every product stands alone.

Split reference. The kernels scale W2 by 2^s (s = 14 - e, max |W2| = m 2^e with m in [0.5, 1)), round to f16 (RNE)
for the hi part and round the f32 remainder to f16 for the lo part: h = f16(v 2^s), l = f16(v 2^s - h). With
|W2| in [0.25, 1) of one binade pair, v 2^s lies in [2^12, 2^14): h and v 2^s are multiples of 2^-11, so is l (no f16
subnormals), and h + l is a multiple of 2^-11 below 2^14 — an f32 value. A product of it with a one-hot operand of
1.0 (scaled to 2^13, lo part 0) is therefore exact in the f32 accumulator, and the kernels' unscale is a power of two:
each output must EQUAL (h + l) 2^-s times the operand, as float64 computes it from the split-rounded weights.

All references are tests/ref64.py on those weights; outputs are pre-filled with NaN.
"""
import math

import pytest
import torch

from ref64 import conv_relu64, dgrad64, route64, routing64, wgrad64
from test_x3_exact_gpu import _assert_bound, _c1_ref64, _exact_case, encode_relu_bits

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- operands and the split reference
def _w2_full_mantissa(seed):
    """W2 [64,32,3,3] f32: random signs, magnitudes in [0.25, 1) with random 23-bit mantissas, all distinct."""
    g = torch.Generator().manual_seed(seed)
    n = 64 * 32 * 9
    mant = torch.randperm(1 << 23, generator=g)[:n]                      # distinct mantissas
    expo = torch.randint(-2, 0, (n,), generator=g)                       # 2^-2 or 2^-1
    mag = (1.0 + mant.double() / (1 << 23)) * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo.double())
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    w = (mag * sign).float()
    assert torch.equal(w.double(), mag * sign)                           # every value an f32 with its full mantissa
    assert w.abs().unique().numel() == n
    return w.reshape(64, 32, 3, 3)


def _split64(W2):
    """(h + l) 2^-s in float64 for every element of W2 (CPU f32), by the documented split."""
    wm = float(W2.abs().max())
    _, e = math.frexp(wm)
    s = min(14 - e, 126)
    v = W2 * (2.0 ** s)                                                  # exact: a power of two, no overflow
    assert torch.equal(v.double(), W2.double() * 2.0 ** s)
    h = v.half()                                                         # RNE
    r = v - h.float()
    assert torch.equal(r.double(), v.double() - h.double())              # the f32 remainder is exact
    lo = r.half()
    return (h.double() + lo.double()) * 2.0 ** -s, h, lo


@pytest.fixture(scope="module")
def w2case():
    W2 = _w2_full_mantissa(4100)
    ws, h, lo = _split64(W2)
    assert int((lo != 0).sum()) > 18000                                  # the lo parts carry information
    assert torch.equal((h.double() + lo.double()).float().double(), h.double() + lo.double())  # h + l is an f32
    return W2, ws


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), device=gpu)


# ----------------------------------------------------------------------------- 1. every W2 slot, dgrad
def test_dgrad_every_w2_slot(gpu, w2case):
    """B = 2, dpooled one-hot (one window per co, 1.0), the routed dY positions 4 pixels apart: every cut-gradient
    element under a footprint is ONE product W2[co][ci][tap] x 1, and must equal the split-rounded weight."""
    from splitcnn import ops
    W2c, ws = w2case
    B = 2
    dp = torch.zeros(B, 64, 12, 12)
    code = torch.empty(B, 64, 12, 12, dtype=torch.uint8)
    wy, wx, cc = torch.meshgrid(torch.arange(12), torch.arange(12), torch.arange(64), indexing="ij")
    code[:] = ((wy + 2 * wx + cc) % 4).permute(2, 0, 1).to(torch.uint8)[None]   # fixed codes, all four positions
    for co in range(64):
        b, k = divmod(co, 32)
        a, c = divmod(k, 6)                       # slot (a, c) of the 6 x 6 grid of dY positions 4 apart
        pos = co % 4                              # the routed position inside its window
        dp[b, co, 2 * a, 2 * c] = 1.0             # dY (4 a + (pos >> 1), 4 c + (pos & 1))
        code[b, co, 2 * a, 2 * c] = pos
    assert sorted(set(code[dp != 0].tolist())) == [0, 1, 2, 3]
    W2, dp, code = W2c.to(gpu).contiguous(), dp.to(gpu), code.to(gpu)
    dc = route64(dp, code)
    want = dgrad64(dc, ws.to(gpu))
    assert int((want != 0).sum()) == 64 * 32 * 9                         # disjoint footprints: one slot per element
    assert int((dgrad64(dc.abs(), torch.ones_like(ws).to(gpu)) > 1).sum()) == 0
    g = ops.conv2_dgrad(dp, code, W2, impl="x3", out=_nan((B, 32, 26, 26), gpu))
    bad = g.double() != want
    assert not bad.any(), f"{int(bad.sum())} cut-gradient elements differ from the split-rounded weight"
    # the fused client backward on the same operands, every ReLU bit set: dW1 / db1 against float64
    x = torch.randn(B, 1, 28, 28, generator=torch.Generator().manual_seed(7)).to(gpu)
    bits = encode_relu_bits(torch.ones(B, 32, 26, 26, dtype=torch.bool, device=gpu))
    slabs = ops.conv2_dgrad_client_slabs(dp, code, W2, x, bits, slabs=_nan((ops.conv2_dgrad_c1w_nslab(B), 320), gpu))
    got, ref = slabs.double().sum(0), _c1_ref64(x, want)
    for sl in (slice(0, 288), slice(288, 320)):
        err = float((got[sl] - ref[sl]).abs().max() / ref[sl].abs().max())
        assert err <= 1e-5, err


# ----------------------------------------------------------------------------- 2. every W2 slot, forward
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["w", "negw"])
def test_fwd_every_w2_slot(gpu, w2case, sign):
    """B = 4, act one-hot (one pixel per ci, 1.0, pixels 4 apart), b2 = 0, four placements (sample = the pixel grid's
    parity offset) so that every tap meets every pool position: each pre-pool value is one product. pooled and codes
    of all five forward entry points == float64's on the split-rounded weights. -W2 shows the weights the ReLU hid."""
    from splitcnn import ops
    W2c, ws = w2case
    B = 4
    act = torch.zeros(B, 32, 26, 26)
    for s in range(B):
        for ci in range(32):
            a, c = divmod(ci, 6)
            act[s, ci, 2 + 4 * a + (s >> 1), 2 + 4 * c + (s & 1)] = 1.0
    W2 = (sign * W2c).to(gpu).contiguous()
    ws = (sign * ws).to(gpu)
    b2 = torch.zeros(64, device=gpu)
    act = act.to(gpu)
    r = conv_relu64(act, ws, b2)
    assert int((conv_relu64(act, torch.ones_like(ws), b2) > 1).sum()) == 0   # one product per pre-pool value
    want_c, win = routing64(r)
    want_p = win.max(-1).values
    seen = {(t, int(q)) for t in range(9) for q in routing_positions(act, t)}
    assert len(seen) == 36                                                # every tap at every pool position
    am = ops.row_amax(act)
    assert torch.equal(am, torch.ones(B, device=gpu))

    def check(pooled, code, what):
        bad = pooled.double() != want_p
        assert not bad.any(), f"{what}: {int(bad.sum())} pooled values differ from the split-rounded product"
        if code is not None:
            bad = code.long() != want_c
            assert not bad.any(), f"{what}: {int(bad.sum())} routing codes differ"

    def outs():
        return dict(pooled=_nan((B, 64, 12, 12), gpu), code=torch.full((B, 64, 12, 12), 0xEE, dtype=torch.uint8, device=gpu))

    nb = ops.conv2_act16_bytes(B)
    check(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, **outs()), "x3")
    a16 = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
    check(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16, **outs()), "x3s")
    check(*ops.conv2_fwd_pool_x3i(a16, am, W2, b2, **outs()), "x3i")
    check(ops.conv2_fwd_pool_x3p(a16, am, W2, b2, pooled=_nan((B, 64, 12, 12), gpu)), None, "x3p")
    a16b = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
    am1 = torch.full((B,), -1.0, device=gpu)
    check(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act16=a16b, act_amax_out=am1, **outs()), "x3sa")
    assert torch.equal(am1, am)


def routing_positions(act, tap):
    """Pool positions (2 (Y & 1) + (X & 1)) at which tap (ky, kx) of the one-hot pixels lands, over the batch."""
    ky, kx = divmod(tap, 3)
    _, _, y, x = torch.nonzero(act, as_tuple=True)
    return set((2 * ((y - ky) & 1) + ((x - kx) & 1)).tolist())


# ----------------------------------------------------------------------------- 3. W2 at every 4-B alignment
@pytest.mark.parametrize("B", [1, 86])
def test_w2_alignment(gpu, B):
    """W2 as a contiguous view at element offsets 0-3 of a larger buffer (the heads read it by dwords), integer
    operands (test_x3_exact_gpu's regime): forward and dgrad == float64 at every offset. B = 1 leaves 253 of the
    256 workgroups without a unit; B = 86 gives 258 units, ranges of 2 and 0."""
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=4300 + B)
    act, W2, b2, dp, code, x, relu = (c[k] for k in ("act", "W2", "b2", "dp", "code", "x", "relu"))
    _assert_bound(conv_relu64(act.abs(), W2.abs(), b2.abs()))
    want_c, win = routing64(conv_relu64(act, W2, b2))
    want_p = win.max(-1).values
    dc = route64(dp, code)
    g64 = dgrad64(dc, W2)
    _assert_bound(dgrad64(dc.abs(), W2.abs()))
    gm = torch.where(relu, g64, torch.zeros_like(g64))
    c1 = _c1_ref64(x, gm)
    _assert_bound(_c1_ref64(x.abs(), gm.abs()))
    bits = encode_relu_bits(relu)
    am, dpa = ops.row_amax(act), ops.row_amax(dp)
    nb = ops.conv2_act16_bytes(B)
    buf = torch.full((W2.numel() + 8,), float("nan"), device=gpu)
    for off in range(4):
        buf.fill_(float("nan"))
        Wv = buf[off:off + W2.numel()].view(64, 32, 3, 3)
        Wv.copy_(W2)
        assert Wv.is_contiguous() and Wv.data_ptr() == buf.data_ptr() + 4 * off
        a16 = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
        for what, (p, cd) in (
                ("x3", ops.conv2_fwd_pool(act, Wv, b2, impl="x3", act_amax=am, pooled=_nan((B, 64, 12, 12), gpu))),
                ("x3s", ops.conv2_fwd_pool(act, Wv, b2, impl="x3", act_amax=am, act16=a16, pooled=_nan((B, 64, 12, 12), gpu))),
                ("x3i", ops.conv2_fwd_pool_x3i(a16, am, Wv, b2, pooled=_nan((B, 64, 12, 12), gpu)))):
            assert torch.equal(cd.long(), want_c), f"{what} codes, W2 offset {off}"
            assert torch.equal(p.double(), want_p), f"{what} pooled, W2 offset {off}"
        g = ops.conv2_dgrad(dp, code, Wv, impl="x3", dp_amax=dpa, out=_nan((B, 32, 26, 26), gpu))
        assert torch.equal(g.double(), g64), f"x3 dgrad, W2 offset {off}"
        slabs = ops.conv2_dgrad_client_slabs(dp, code, Wv, x, bits, dp_amax=dpa,
                                             slabs=_nan((ops.conv2_dgrad_c1w_nslab(B), 320), gpu))
        assert torch.equal(slabs.double().sum(0), c1), f"fused client backward, W2 offset {off}"


# ----------------------------------------------------------------------------- 4. wgrad launch scales
@pytest.fixture(scope="module")
def wgrad_case(gpu):
    """B = 513 (the second 512-stride of the scale reduction holds one element), narrow integer operands."""
    B = 513
    c = _exact_case(gpu, B, seed=4400, narrow=True, small_grad=True)
    return B, c


@pytest.mark.parametrize("big", [512, 0, 511])
def test_wgrad_launch_scales(gpu, wgrad_case, big):
    """One sample's act and dpooled 2^8 times the others': the launch scales come from that sample alone, at the last
    index (the lone element of the reduction's second 512-stride), the first and the end of the first stride. Slabs
    of the images-fed x3 wgrad == float64. A maximum missed at that index overflows f16."""
    from splitcnn import ops
    B, c = wgrad_case
    act, dp = c["act"].clone(), c["dp"].clone()     # the shared case stays unchanged
    W2, b2, code = c["W2"], c["b2"], c["code"]
    act[big] *= 256.0
    dp[big] *= 256.0
    assert bool((act[big] != 0).any()) and bool((route64(dp[big:big + 1], code[big:big + 1]) != 0).any())
    for v in (act, dp):                             # still exact f16 values
        assert torch.equal(v, v.round()) and torch.equal(v.half().float(), v)
    dc = route64(dp, code)
    dW, db = wgrad64(act, dc)
    w64 = torch.cat([dW.reshape(-1), db])
    dWa, dba = wgrad64(act.abs(), dc.abs())
    _assert_bound(torch.cat([dWa.reshape(-1), dba]))
    am, dpa = ops.row_amax(act), ops.row_amax(dp)
    assert int(am.argmax()) == big and int(dpa.argmax()) == big
    assert float(am[big]) >= 128 * float(torch.cat([am[:big], am[big + 1:]]).max())
    a16 = torch.full((ops.conv2_act16_bytes(B),), 0x5A, dtype=torch.uint8, device=gpu)
    ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16)
    s = ops.conv2_wgrad_slabs(None, dp, code, impl="x3", act_amax=am, dp_amax=dpa, act16=a16,
                              slabs=_nan((ops.conv2_wgrad_nslab(B, impl="x3"), ops.CONV2_SLAB), gpu))
    assert bool(torch.isfinite(s).all()), "non-finite slab values: a launch scale missed the large sample"
    assert torch.equal(s.double().sum(0), w64)
    assert torch.equal(ops.reduce_slabs(s).double(), w64)
