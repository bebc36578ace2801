"""GPU: the K2 conv2 kernels on routing codes their own forward did not produce, and on integer operands where
their result must equal float64 exactly (tests/ref64.py: conv_relu64, routing64, route64, dgrad64, wgrad64).

Random codes. tests/test_x3_gpu.py takes `code` from ops.conv2_fwd_pool on a seeded-init network, so the backward
kernels never see other patterns. Here `code` is uniform over 0..4 (every position, blocked windows, one channel routed
differently from its neighbours), with one sample all blocked and one with a single routed window, at the existing
bars: 1e-5 of max |ref| overall and per sample.

Exact regime. act in [0, 15], W2 in [-7, 7], b2 in [-31, 31], dpooled in [-15, 15], codes uniform, x and the ReLU bits
random. Every operand is an integer of at most 11 significant bits, so after the x3 kernels' power-of-two scaling it
is an f16 value exactly: its `lo` part is zero, the hi x hi products are exact, and (absolute-value sums below 2^24,
asserted on the reference side) the f32 accumulation is exact in any order. pooled, codes, the cut gradient and the
slab sums must then EQUAL float64's, every element, no tie excused. The narrow variant (act nonzero with probability
0.15 in {1, 2, 3}, W2 nonzero with probability 0.3 in {-1, +1}, b2 in [-2, 2]) makes exact ties and zero maxima by the
thousand; they must route as routing64 says. The scale bounds act_amax / dp_amax are passed tight (ops.row_amax) and
loose (x 16): only their power of two is used and the operands keep 11 bits at either, so the results are identical.

The fused client backward multiplies the (exact) cut gradient by x and sums over the whole batch, so its operands are
chosen to keep that sum below 2^24: x nonzero with probability 0.25 in {-1, +1}, ReLU bits set with probability 0.25
(the ranges above are unchanged); the bound is asserted like the others.

direct / Winograd. The same exact operands through impl="direct" (plain f32 MFMA sums: exact under the same bound) and
the Winograd default. F(2x2,3x3) (csrc/slk_wino.hip) transforms the input by B^T d B (entries +-1: sums of 4 inputs,
integers), the filter by G g G^T (G holds 1/2: every halving is exact in binary floating point, U is a multiple of
2^-2 with |U| <= 2.25 max|w|) and the product by A^T M A (entries +-1, 9 terms); the weight gradient applies G^T dU G
(two more halvings). Every intermediate is therefore a multiple of 2^-4 at the finest, and an f32 holds multiples of
2^-4 exactly below 2^20. Bounds from the operands' maxima: forward 9 x 32 x (4 x 15) x (2.25 x 7) + 31 = 272 k, dgrad
9 x 64 x (4 x 15) x (2.25 x 7) = 544 k, both below 2^20 with the wide ranges. The weight gradient sums Z_t V_t over
every tile of the batch (|Z_t| <= the routed |dY|, |V_t| <= the sum of |act| over the tile's 4 x 4 patch) and the
output transform gains (1 + 1/2 + 1/2)^2 = 4; the wide ranges do not fit 2^20 at B = 130, so the Winograd weight
gradient runs on narrow activations and gradients of magnitude <= 3, with the bound computed from the operands.
"""
import pytest
import torch
import torch.nn.functional as F

from ref64 import conv_relu64, dgrad64, route64, routing64, wgrad64

pytestmark = pytest.mark.gpu

BATCHES = [1, 5, 130]


# ----------------------------------------------------------------------------- operands
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse(g, shape, p, lo, hi):
    """nonzero with probability p, then uniform over the nonzero integers of [lo, hi]."""
    v = _ints(g, shape, lo, hi)
    while (v == 0).any():
        v = torch.where(v == 0, _ints(g, shape, lo, hi), v)
    return torch.where(torch.rand(shape, generator=g) < p, v, torch.zeros(shape))


def encode_relu_bits(mask):
    """bool [B, 32, 26, 26] -> the cut's ReLU bit map int32 [B, 676]: bit 4 (c & 7) + u of word (c >> 3, t) = pixel
    4 t + u of channel c (the inverse of test_x3_gpu._decode_bits)."""
    B = mask.shape[0]
    m = mask.reshape(B, 4, 8, 169, 4).long()
    sh = (4 * torch.arange(8, device=mask.device))[None, None, :, None, None] + \
        torch.arange(4, device=mask.device)[None, None, None, None, :]
    w = (m << sh).sum(dim=(2, 4))                                   # B, 4, 169
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w)
    return w.to(torch.int32).reshape(B, 676).contiguous()


def _exact_case(gpu, B, seed, narrow=False, small_grad=False, relu_p=0.25):
    """relu_p: the density of the ReLU bits (the last draw, so every other operand is the same at any value)."""
    g = torch.Generator().manual_seed(seed)
    if narrow:
        act = _sparse(g, (B, 32, 26, 26), 0.15, 1, 3)
        W2, b2 = _sparse(g, (64, 32, 3, 3), 0.3, -1, 1), _ints(g, (64,), -2, 2)
    else:
        act, W2, b2 = _ints(g, (B, 32, 26, 26), 0, 15), _ints(g, (64, 32, 3, 3), -7, 7), _ints(g, (64,), -31, 31)
    dp = _ints(g, (B, 64, 12, 12), -3, 3) if small_grad else _ints(g, (B, 64, 12, 12), -15, 15)
    code = torch.randint(0, 5, (B, 64, 12, 12), generator=g).to(torch.uint8)
    x = _sparse(g, (B, 1, 28, 28), 0.25, -1, 1)
    relu = torch.rand((B, 32, 26, 26), generator=g) < relu_p
    c = dict(act=act, W2=W2, b2=b2, dp=dp, code=code, x=x, relu=relu)
    c = {k: v.to(gpu).contiguous() for k, v in c.items()}
    for k in ("act", "W2", "b2", "dp", "x"):         # integers of at most 11 significant bits: exact f16 values
        v = c[k]
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2048
        assert torch.equal(v.half().float(), v)
    return c


def _assert_bound(abs_sum, limit=2.0 ** 24):
    m = float(abs_sum.max())
    assert m < limit, f"absolute-value sum {m} reaches {limit}: the f32 accumulation is not exact"


def _c1_ref64(x, gm):
    """conv1's [dW1 (32 x 9) | db1] in float64 from the masked cut gradient gm [B,32,26,26] and x [B,1,28,28]."""
    B = x.shape[0]
    win = F.unfold(x.double(), 3)                                    # B, 9, 676
    dW = torch.einsum("bcp,bkp->ck", gm.reshape(B, 32, 676), win)
    return torch.cat([dW.reshape(-1), gm.sum(dim=(0, 2, 3))])


def _amax_forms(t):
    """The per-sample scale bound, tight (the exact max) and loose (x 16)."""
    from splitcnn import ops
    am = ops.row_amax(t)
    return (("tight", am), ("loose", am * 16))


# ----------------------------------------------------------------------------- random codes, real-valued
def _real_case(gpu, B, seed):
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import ClientStage
    a, b = init_models(seed=seed)
    x, _ = SyntheticMNIST(seed + 1).batch(B)
    x = x.to(gpu)
    act = ClientStage(a, device=gpu).forward(x).clone()
    g = torch.Generator().manual_seed(seed + 2)
    dp = torch.randn(B, 64, 12, 12, generator=g) * 1e-3
    code = torch.randint(0, 5, (B, 64, 12, 12), generator=g).to(torch.uint8)
    if B >= 5:
        code[1] = 4                                  # a sample that is blocked everywhere
        code[2] = 4                                  # a sample with a single routed window, holding its largest |dp|
        code[2, 17, 5, 7] = 2
        i = dp[2].abs().argmax()
        big = dp[2].reshape(-1)[i].clone()
        dp[2].reshape(-1)[i] = dp[2, 17, 5, 7]
        dp[2, 17, 5, 7] = big
    relu = torch.rand((B, 32, 26, 26), generator=g) < 0.5
    return dict(x=x.contiguous(), act=act, W2=b.conv2.weight.detach().to(gpu).contiguous(),
                b2=b.conv2.bias.detach().to(gpu).contiguous(), dp=dp.to(gpu).contiguous(), code=code.to(gpu).contiguous(),
                relu=relu.to(gpu))


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("B", BATCHES)
def test_x3_backward_random_codes(gpu, B):
    """ops.conv2_dgrad(impl="x3"), ops.conv2_dgrad_client_slabs and ops.conv2_wgrad_slabs(impl="x3", f32 act and
    images-fed) on uniform random codes against float64: 1e-5 of max |ref|, the cut gradient also per sample."""
    from splitcnn import ops
    c = _real_case(gpu, B, seed=900 + B)
    dc = route64(c["dp"], c["code"])
    g64 = dgrad64(dc, c["W2"])
    gx = ops.conv2_dgrad(c["dp"], c["code"], c["W2"], impl="x3")
    assert _rel(gx, g64) <= 1e-5
    num = (gx.double() - g64).abs().flatten(1).max(dim=1).values
    den = g64.abs().flatten(1).max(dim=1).values.clamp_min(1e-30)
    assert float((num / den).max()) <= 1e-5, (num / den).tolist()[:8]
    if B >= 5:
        assert float(gx[1].abs().max()) == 0.0      # all blocked: exactly no gradient
        assert int((gx[2] != 0).sum()) <= 32 * 9    # one routed window reaches 9 pixels of every input channel
    # the fused client backward
    slabs = ops.conv2_dgrad_client_slabs(c["dp"], c["code"], c["W2"], c["x"], encode_relu_bits(c["relu"]))
    assert slabs.shape == (min(3 * B, 256), 320)
    got = slabs.double().sum(0)
    want = _c1_ref64(c["x"], torch.where(c["relu"], g64, torch.zeros_like(g64)))
    for sl in (slice(0, 288), slice(288, 320)):
        assert _rel(got[sl], want[sl]) <= 1e-5
    # the weight gradient, loading act itself and fed the forward's images
    dW, db = wgrad64(c["act"], dc)
    want = torch.cat([dW.reshape(-1), db])
    am = ops.row_amax(c["act"])
    a16 = torch.empty(ops.conv2_act16_bytes(B), dtype=torch.uint8, device=gpu)
    ops.conv2_fwd_pool(c["act"], c["W2"], c["b2"], impl="x3", act_amax=am, act16=a16)
    s1 = ops.conv2_wgrad_slabs(c["act"], c["dp"], c["code"], impl="x3", act_amax=am)
    s2 = ops.conv2_wgrad_slabs(c["act"], c["dp"], c["code"], impl="x3", act_amax=am, act16=a16)
    s3 = ops.conv2_wgrad_slabs(None, c["dp"], c["code"], impl="x3", act_amax=am, act16=a16)
    assert s1.shape == s2.shape == (min(6 * B, 256), ops.CONV2_SLAB)
    assert torch.equal(s2, s3)
    g1, g2 = (ops.reduce_slabs(s).double() for s in (s1, s2))
    assert _rel(g2, g1) <= 2e-6
    for got in (g1, g2):
        for sl in (slice(0, 18432), slice(18432, 18496)):
            assert _rel(got[sl], want[sl]) <= 1e-5


# ----------------------------------------------------------------------------- exact regime, x3
def _assert_fwd(pooled, code, want_p, want_c, what):
    bad = code.long() != want_c
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} routing codes differ from routing64"
    bad = pooled.double() != want_p
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} pooled values differ from float64"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
def test_x3_fwd_exact(gpu, B, narrow):
    """impl="x3", the forward writing the images (x3s), reading them (x3i) and computing the amax itself (x3sa):
    pooled and code == float64's in every window, at a tight and a loose scale bound."""
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=1100 + B, narrow=narrow)
    act, W2, b2 = c["act"], c["W2"], c["b2"]
    _assert_bound(conv_relu64(act.abs(), W2.abs(), b2.abs()))
    r = conv_relu64(act, W2, b2)
    want_c, win = routing64(r)
    want_p = win.max(-1).values
    if narrow and B > 1:     # what makes this variant discriminate (B = 1 is too small to promise shares)
        m = want_p
        assert float((((win == m[..., None]).sum(-1) > 1) & (m > 0)).double().mean()) >= 0.01
        assert float((m == 0).double().mean()) >= 0.01
    nb = ops.conv2_act16_bytes(B)
    for name, am in _amax_forms(act):
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am), want_p, want_c, f"x3 {name}")
        a16 = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16), want_p, want_c, f"x3s {name}")
        _assert_fwd(*ops.conv2_fwd_pool_x3i(a16, am, W2, b2), want_p, want_c, f"x3i {name}")
    a16 = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
    am1 = torch.full((B,), -1.0, device=gpu)
    _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act16=a16, act_amax_out=am1), want_p, want_c, "x3sa")
    assert torch.equal(am1, ops.row_amax(act))


@pytest.mark.parametrize("B", BATCHES)
def test_x3_backward_exact(gpu, B):
    """x3 dgrad, fused client backward and x3 weight gradient (f32 act and images-fed) on integer operands and random
    codes: cut gradient and float64 slab sums == float64's exactly, identical at tight and loose scale bounds."""
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=1200 + B)
    act, W2, b2, dp, code, x, relu = (c[k] for k in ("act", "W2", "b2", "dp", "code", "x", "relu"))
    dc = route64(dp, code)
    g64 = dgrad64(dc, W2)
    gabs = dgrad64(dc.abs(), W2.abs())
    _assert_bound(gabs)
    gm = torch.where(relu, g64, torch.zeros_like(g64))
    c1 = _c1_ref64(x, gm)
    _assert_bound(_c1_ref64(x.abs(), gm.abs()))
    dW, db = wgrad64(act, dc)
    w64 = torch.cat([dW.reshape(-1), db])
    dWa, dba = wgrad64(act.abs(), dc.abs())
    _assert_bound(torch.cat([dWa.reshape(-1), dba]))
    bits = encode_relu_bits(relu)
    nb = ops.conv2_act16_bytes(B)
    for dname, dpa in _amax_forms(dp):
        gx = ops.conv2_dgrad(dp, code, W2, impl="x3", dp_amax=dpa)
        assert torch.equal(gx.double(), g64), f"x3 dgrad ({dname} dp_amax)"
        slabs = ops.conv2_dgrad_client_slabs(dp, code, W2, x, bits, dp_amax=dpa)
        assert torch.equal(slabs.double().sum(0), c1), f"fused client backward ({dname} dp_amax)"
        assert torch.equal(ops.reduce_slabs(slabs).double(), c1)
        for aname, am in _amax_forms(act):
            a16 = torch.full((nb,), 0x5A, dtype=torch.uint8, device=gpu)
            ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16)
            for form, s in (("f32 act", ops.conv2_wgrad_slabs(act, dp, code, impl="x3", act_amax=am, dp_amax=dpa)),
                            ("images", ops.conv2_wgrad_slabs(None, dp, code, impl="x3", act_amax=am, dp_amax=dpa,
                                                             act16=a16))):
                assert torch.equal(s.double().sum(0), w64), f"x3 wgrad {form} ({aname} act_amax, {dname} dp_amax)"
                assert torch.equal(ops.reduce_slabs(s).double(), w64)


# ----------------------------------------------------------------------------- exact regime, direct and Winograd
WINO_LIMIT = 2.0 ** 20     # multiples of 2^-4 are exact in f32 below 2^20 (module docstring)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("impl", ["direct", "wino"])
@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
def test_f32_fwd_exact(gpu, impl, B, narrow):
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=1300 + B, narrow=narrow)
    act, W2, b2 = c["act"], c["W2"], c["b2"]
    _assert_bound(conv_relu64(act.abs(), W2.abs(), b2.abs()))
    if impl == "wino":
        bound = 9 * 32 * (4 * float(act.abs().max())) * (2.25 * float(W2.abs().max())) + float(b2.abs().max())
        assert bound < WINO_LIMIT, bound
    want_c, win = routing64(conv_relu64(act, W2, b2))
    _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl=impl), win.max(-1).values, want_c, impl)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("impl", ["direct", "wino"])
def test_f32_backward_exact(gpu, impl, B):
    """The cut gradient on the wide operands; the weight gradient on the wide operands (direct) or on narrow
    activations and gradients <= 3 (Winograd, whose transform-domain sums must stay below 2^20)."""
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=1400 + B)
    W2, dp, code = c["W2"], c["dp"], c["code"]
    dc = route64(dp, code)
    _assert_bound(dgrad64(dc.abs(), W2.abs()))
    if impl == "wino":
        bound = 9 * 64 * (4 * float(dp.abs().max())) * (2.25 * float(W2.abs().max()))
        assert bound < WINO_LIMIT, bound
    g = ops.conv2_dgrad(dp, code, W2, impl=impl)
    assert torch.equal(g.double(), dgrad64(dc, W2)), f"{impl} dgrad"

    if impl == "wino":
        c = _exact_case(gpu, B, seed=1500 + B, narrow=True, small_grad=True)
        act, dp, code = c["act"], c["dp"], c["code"]
        dc = route64(dp, code)
        # sum over the batch's tiles of |routed dY| x (sum of |act| over the tile's 4 x 4 patch), x 4 for G^T . G
        patch = F.avg_pool2d(act.double().abs(), 4, stride=2) * 16                       # B, 32, 12, 12
        routed = torch.where(code < 4, dp.double().abs(), torch.zeros_like(dp, dtype=torch.float64))
        bound = 4 * torch.einsum("bot,bct->oc", routed.reshape(B, 64, 144), patch.reshape(B, 32, 144))
        _assert_bound(bound, WINO_LIMIT)
    else:
        act = c["act"]
    dWa, dba = wgrad64(act.abs(), dc.abs())
    _assert_bound(torch.cat([dWa.reshape(-1), dba]))
    dW, db = wgrad64(act, dc)
    want = torch.cat([dW.reshape(-1), db])
    s = ops.conv2_wgrad_slabs(act, dp, code, impl=impl)
    assert torch.equal(s.double().sum(0), want), f"{impl} wgrad"
    assert torch.equal(ops.reduce_slabs(s).double(), want)
