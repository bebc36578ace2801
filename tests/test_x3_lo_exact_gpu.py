"""GPU: the x3 conv2 kernels (csrc/slk_x3.hip) EXACTLY on operands whose low halves are not zero, and the act16
images against an independent statement of the split.

tests/test_x3_exact_gpu.py is exact only where every operand is an f16 value already (l = 0) and every sample has
the same scale: the l planes of the images and their slot swizzle, the l weight fragments, the l half of the routed
dY of the 2:4-sparse weight gradient and the per-sample 2^(sd + sx - s_b) compensation of dY are invisible to it.
Here the operands come from the three classes of tests/x3_split_ref.py (14-bit, 18-bit, both-sided; its docstring
holds the exactness argument, tests/test_x3_split_ref_cpu.py pins it and shows that five wrong variants of the
arithmetic change the expectation). Expected values are the float64 three-term sums; the bound (sum of |kept
addends| < 2^24 finest granules per output) is asserted for every case before a kernel runs, so pooled, codes, the
cut gradient and the slab sums must EQUAL the expectation as float64, no element excused. Outputs are pre-filled
with NaN and images with 0x5A; every case runs at a tight (ops.row_amax) and a loose (x 16) scale bound.

Densities (inputs, chosen for the bound, x3_split_ref's docstring): forward act 0.15 / W2 0.3 (the l-carrying W2 is
dense); dgrad dpooled 0.3 on uniform codes 0..4 / W2 0.3; weight gradient act 0.15 / dpooled 0.3 up to B = 5 and
0.05 / 0.05 at B = 130 (a 14-bit dpooled 0.02 there: db2 sums the values themselves). The fused client backward
sums the (exact, up to 2^21 granules) cut gradient over the batch: x is nonzero with probability 0.25 in {-1, +1}
as in test_x3_exact_gpu, and the ReLU bits are set with probability min(0.25, 8 / (676 B)), about 8 addends per
channel and 2 per tap (40 a channel already reach 2^24.7 granules in the 18-bit class), so that its sums keep the
bound (asserted).

Mixed exponents (weight gradient): sample b's act is multiplied by 2^ka[b], its dpooled by 2^kd[b], ka = (0, 2, 1)
and kd = (1, 0, 2) by b mod 3: three values of each in a batch, a total spread of 4 binades, and neighbouring
samples always differ in both. A K share of either kernel holds 2 to 4 units of 3 (or 6) a sample at B = 130, so at
most two samples: every share that spans two samples mixes two scales of each operand (three distinct values cannot
meet in one share at this batch; tests/test_steady_exact_gpu.py runs the same variant at B = 171 to 342, where three
do). These two files hold the only exact checks of the dY compensation.

Images: real-valued operands (randn-based ReLU outputs at per-sample magnitudes from 1e-3 to 1e3, SyntheticMNIST
through conv1) with planted elements in every sample - exact ties both ways, an l that is subnormal in f16, an
element 2^-20 of the maximum, -0.0 where the producer takes it - and a sample whose maximum is 0. The images of the
forward (x3s, x3sa), of ops.conv1_fwd_x3 and of ops.cut_unpack_x3 are decoded (x3_split_ref.decode_act16) and
compared bit for bit with the numpy split at 2^x3_exp(amax). (The -0.0 element is what found the one deviation:
h = +0, l = -0 from a compiler-chosen v_fma_mixlo_f16(v, sc, +0); x3_split8_img in csrc/slk_x3.hip has the story.)

Measured on the MI355X: every class exact in every kernel above; nothing of the adder's to record."""
import numpy as np
import pytest
import torch

from ref64 import dgrad64, route64, routing64, wgrad64
from test_x3_exact_gpu import _c1_ref64, encode_relu_bits
from x3_split_ref import (assert_exact, assert_sum_exact, conv64, decode_act16, gen14, gen18, gen_both, gen_small,
                          gran_exp, split, split_np, three_term, x3_exp)

pytestmark = pytest.mark.gpu

BATCHES = [1, 5, 130]


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _img(B, dev):
    from splitcnn import ops
    return torch.full((ops.conv2_act16_bytes(B),), 0x5A, dtype=torch.uint8, device=dev)


def _amax_forms(t):
    from splitcnn import ops
    am = ops.row_amax(t)
    return (("tight", am), ("loose", am * 16))


def _parts(v, per_sample=True):
    h, l, rem = split(v, per_sample=per_sample)
    assert not rem.any(), "the class must split without a remainder"
    return h, l


# ----------------------------------------------------------------------------- forward
def fwd_case(cls, B, seed, dev):
    """Operands of one forward class and the expected pooled / code (three-term float64), bound asserted."""
    g = torch.Generator().manual_seed(seed)
    a_shape, w_shape = (B, 32, 26, 26), (64, 32, 3, 3)
    bscale = 1.0
    if cls == "act14":
        act, W2 = gen14(g, a_shape, 0.15, False), gen_small(g, w_shape, 0.3, [1], True)
    elif cls == "act18":
        act, W2 = gen18(g, a_shape, 0.15, False), gen_small(g, w_shape, 0.3, [1], True)
    elif cls == "w14":
        act, W2 = gen_small(g, a_shape, 0.15, [1, 2, 3], False), gen14(g, w_shape, 1.0, True)
    else:
        act, W2 = gen_both(g, a_shape, 0.15, False), gen_both(g, w_shape, 0.3, True)
        bscale = 2048.0                                   # the bias on the addends' granule
    b2 = torch.randint(-2, 3, (64,), generator=g).float() * bscale
    act, W2, b2 = (t.to(dev).contiguous() for t in (act, W2, b2))
    ah, al = _parts(act)
    wh, wl = _parts(W2, per_sample=False)
    assert_exact(ah, al, wh, wl, "fwd", extra=b2.double()[None, :, None, None], what=f"forward {cls}")
    y = three_term(ah, al, wh, wl, "fwd")
    if cls == "both":
        if B > 1:
            assert float((y != conv64(act, W2)).double().mean()) >= 0.005     # the dropped term is visible
    else:
        assert torch.equal(y, conv64(act, W2))            # one-sided: three terms are the whole product
    want_c, win = routing64((y + b2.double()[None, :, None, None]).clamp_min(0.0))
    return act, W2, b2, win.max(-1).values, want_c


def _assert_fwd(pooled, code, want_p, want_c, what):
    if code is not None:
        bad = code.long() != want_c
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} routing codes differ from routing64"
    bad = pooled.double() != want_p
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} pooled values differ from the three-term sum"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("cls", ["act14", "act18", "w14", "both"])
def test_x3_fwd_lo_exact(gpu, cls, B):
    """impl="x3", images written (x3s), images read (x3i), in-kernel amax (x3sa) and the code-less evaluation
    forward (x3p): pooled and code == the three-term float64 expectation in every window."""
    from splitcnn import ops
    act, W2, b2, want_p, want_c = fwd_case(cls, B, 2100 + B, gpu)
    assert float((want_p > 0).double().mean()) >= 0.05
    shp = (B, 64, 12, 12)

    def outs():
        return dict(pooled=_nan(shp, gpu), code=torch.full(shp, 0xEE, dtype=torch.uint8, device=gpu))

    for name, am in _amax_forms(act):
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, **outs()), want_p, want_c, f"x3 {name}")
        a16 = _img(B, gpu)
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16, **outs()), want_p, want_c,
                    f"x3s {name}")
        _assert_fwd(*ops.conv2_fwd_pool_x3i(a16, am, W2, b2, **outs()), want_p, want_c, f"x3i {name}")
        _assert_fwd(ops.conv2_fwd_pool_x3p(a16, am, W2, b2, pooled=_nan(shp, gpu)), None, want_p, want_c, f"x3p {name}")
    a16 = _img(B, gpu)
    am1 = torch.full((B,), -1.0, device=gpu)
    _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act16=a16, act_amax_out=am1, **outs()), want_p, want_c,
                "x3sa")
    assert torch.equal(am1, ops.row_amax(act))
    _assert_fwd(*ops.conv2_fwd_pool_x3i(a16, am1, W2, b2, **outs()), want_p, want_c, "x3i of x3sa's images")


# ----------------------------------------------------------------------------- input gradient
def relu_density(B):
    return min(0.25, 8.0 / (676 * B))


def dgrad_case(cls, B, seed, dev, special=False):
    """special: sample 1 is blocked everywhere and sample 2 has a single routed window (drawn operands unchanged)."""
    g = torch.Generator().manual_seed(seed)
    d_shape, w_shape = (B, 64, 12, 12), (64, 32, 3, 3)
    if cls == "dp14":
        dp, W2 = gen14(g, d_shape, 0.3, True), gen_small(g, w_shape, 0.3, [1], True)
    elif cls == "dp18":
        dp, W2 = gen18(g, d_shape, 0.3, True), gen_small(g, w_shape, 0.3, [1], True)
    elif cls == "w14":
        dp, W2 = gen_small(g, d_shape, 0.3, [1, 2, 3], True), gen14(g, w_shape, 1.0, True)
    else:
        dp, W2 = gen_both(g, d_shape, 0.3, True), gen_both(g, w_shape, 0.3, True)
    code = torch.randint(0, 5, d_shape, generator=g).to(torch.uint8)
    if special:
        code[1:3] = 4
        code[2, 17, 5, 7] = 2
    x = gen_small(g, (B, 1, 28, 28), 0.25, [1], True)
    relu = torch.rand((B, 32, 26, 26), generator=g) < relu_density(B)
    cut = torch.randn((B, 32, 26, 26), generator=g).clamp_min(0.0)            # its zero pattern is the codec mask
    dp, W2, code, x, relu, cut = (t.to(dev).contiguous() for t in (dp, W2, code, x, relu, cut))
    dh, dl = _parts(dp)
    wh, wl = _parts(W2, per_sample=False)
    rh, rl = route64(dh, code), route64(dl, code)
    assert_exact(rh, rl, wh, wl, "dgrad", what=f"dgrad {cls}")
    g64 = three_term(rh, rl, wh, wl, "dgrad")
    if cls == "both":
        if B > 1:
            assert float((g64 != dgrad64(route64(dp, code), W2)).double().mean()) >= 0.005
    else:
        assert torch.equal(g64, dgrad64(route64(dp, code), W2))
    gm = torch.where(relu, g64, torch.zeros_like(g64))
    c1 = _c1_ref64(x, gm)
    ge = gran_exp(gm)
    if ge is not None:
        units = float(_c1_ref64(x.abs(), gm.abs()).max()) / 2.0 ** ge
        assert units < 2.0 ** 24, f"fused client backward {cls}: 2^{np.log2(max(units, 1)):.2f} granules"
    return dp, W2, code, x, relu, cut, g64, c1


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("cls", ["dp14", "dp18", "w14", "both"])
def test_x3_dgrad_lo_exact(gpu, cls, B):
    """ops.conv2_dgrad(impl="x3"), the fused client backward and the packed dgrad on uniform random codes: the cut
    gradient, the client's slab sums and the packed values == the three-term float64 expectation."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    dp, W2, code, x, relu, cut, g64, c1 = dgrad_case(cls, B, 2200 + B, gpu)
    bits = encode_relu_bits(relu)
    n = cut.numel()
    codec = CutCodec()
    bk = codec.buffers("lo", n, gpu)
    codec.encode(cut, bk)
    rk = codec.ranks("lo", n, bk)
    set_ = cut.reshape(-1) != 0
    t = int(set_.sum())
    assert int(bk[3].item()) == t and 0 < t < n
    want_vals = g64.reshape(-1)[set_]
    for name, dpa in _amax_forms(dp):
        gx = ops.conv2_dgrad(dp, code, W2, impl="x3", dp_amax=dpa, out=_nan((B, 32, 26, 26), gpu))
        bad = gx.double() != g64
        assert not bad.any(), f"x3 dgrad ({name}): {int(bad.sum())} of {bad.numel()} differ"
        slabs = ops.conv2_dgrad_client_slabs(dp, code, W2, x, bits, dp_amax=dpa,
                                             slabs=_nan((ops.conv2_dgrad_c1w_nslab(B), 320), gpu))
        assert torch.equal(slabs.double().sum(0), c1), f"fused client backward ({name})"
        assert torch.equal(ops.reduce_slabs(slabs).double(), c1)
        got = _nan((n,), gpu)
        ops.conv2_dgrad_x3_pack(dp, code, W2, dpa, bk[0], rk, got)
        assert torch.equal(got[:t].double(), want_vals), f"packed dgrad ({name})"
        assert torch.isnan(got[t:]).all()


# ----------------------------------------------------------------------------- weight gradient
KA, KD = (0, 2, 1), (1, 0, 2)


def wgrad_densities(cls, B):
    pa, pd = (0.15, 0.3) if B <= 5 else (0.05, 0.05)
    if B > 5 and cls in ("dp14", "mixed_dp"):
        pd = 0.02          # db2 adds 14-bit values themselves: 0.05 x 2^kd reaches 2^24.5 granules at B = 130
    return pa, pd


def wgrad_case(cls, B, seed, dev, densities=None):
    """densities: (act, dpooled) nonzero probabilities; default wgrad_densities(cls, B)."""
    g = torch.Generator().manual_seed(seed)
    a_shape, d_shape = (B, 32, 26, 26), (B, 64, 12, 12)
    pa, pd = wgrad_densities(cls, B) if densities is None else densities
    if cls in ("act14", "mixed_act"):
        act, dp = gen14(g, a_shape, pa, False), gen_small(g, d_shape, pd, [1], True)
    elif cls in ("dp14", "mixed_dp"):
        act, dp = gen_small(g, a_shape, pa, [1, 2, 3], False), gen14(g, d_shape, pd, True)
    else:
        act, dp = gen_both(g, a_shape, pa, False), gen_both(g, d_shape, pd, True)
    if cls.startswith("mixed"):
        b = torch.arange(B)
        ka, kd = torch.tensor(KA)[b % 3], torch.tensor(KD)[b % 3]
        assert len(set(ka.tolist())) == 3 and len(set(kd.tolist())) == 3
        assert (ka[1:] != ka[:-1]).all() and (kd[1:] != kd[:-1]).all()
        act = act * (2.0 ** ka.float())[:, None, None, None]
        dp = dp * (2.0 ** kd.float())[:, None, None, None]
    code = torch.randint(0, 5, d_shape, generator=g).to(torch.uint8)
    act, dp, code = (t.to(dev).contiguous() for t in (act, dp, code))
    if cls.startswith("mixed"):     # the samples' scale exponents really differ, for both operands
        assert len(set(x3_exp(act.flatten(1).abs().max(1).values.cpu().numpy()).tolist())) >= 3
        assert len(set(x3_exp(dp.flatten(1).abs().max(1).values.cpu().numpy()).tolist())) >= 3
    xh, xl = _parts(act)
    dh, dl = _parts(dp)
    rh, rl = route64(dh, code), route64(dl, code)
    assert_exact(xh, xl, rh, rl, "wgrad", what=f"wgrad {cls}")
    dc = route64(dp, code)
    assert_sum_exact(dc, (0, 2, 3), what=f"db2 {cls}")
    dW = three_term(xh, xl, rh, rl, "wgrad")
    full, db = wgrad64(act, dc)
    if cls == "both":
        if B > 1:
            assert float((dW != full).double().mean()) >= 0.005
    else:
        assert torch.equal(dW, full)
    return act, dp, code, torch.cat([dW.reshape(-1), db])


WGRAD_CASES = [(c, B) for c in ("act14", "dp14", "both") for B in BATCHES] + \
              [(c, B) for c in ("mixed_act", "mixed_dp") for B in (5, 130)]


@pytest.mark.parametrize("cls,B", WGRAD_CASES)
def test_x3_wgrad_lo_exact(gpu, cls, B):
    """The x3 weight gradient loading the f32 act and fed the forward's images (the 2:4-sparse kernel): the float64
    slab sum and ops.reduce_slabs == [dW2 | db2] of the three-term expectation, at every pairing of tight and loose
    scale bounds."""
    from splitcnn import ops
    act, dp, code, want = wgrad_case(cls, B, 2300 + B, gpu)
    W2 = torch.zeros(64, 32, 3, 3, device=gpu)
    W2[:, 0, 1, 1] = 1.0
    b2 = torch.zeros(64, device=gpu)
    nslab = ops.conv2_wgrad_nslab(B, impl="x3")
    for dname, dpa in _amax_forms(dp):
        for aname, am in _amax_forms(act):
            a16 = _img(B, gpu)
            ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16)
            s1 = ops.conv2_wgrad_slabs(act, dp, code, impl="x3", act_amax=am, dp_amax=dpa,
                                       slabs=_nan((nslab, ops.CONV2_SLAB), gpu))
            s2 = ops.conv2_wgrad_slabs(None, dp, code, impl="x3", act_amax=am, dp_amax=dpa, act16=a16,
                                       slabs=_nan((nslab, ops.CONV2_SLAB), gpu))
            for form, s in (("f32 act", s1), ("images", s2)):
                what = f"x3 wgrad {cls} {form} ({aname} act_amax, {dname} dp_amax)"
                bad = s.double().sum(0) != want
                assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} slab sums differ"
                assert torch.equal(ops.reduce_slabs(s).double(), want), what


# ----------------------------------------------------------------------------- images
TIE_DOWN, TIE_UP = 1024.5, 1025.5          # scaled domain, f16 ulp 1: -> 1024 (even) + 0.5 and 1026 - 0.5
LO_SUBNORMAL = 0.125 + 3 * 2.0 ** -20      # h = 0.125, l = 3 * 2^-20: subnormal in f16 (below 2^-14), exact


def _plant(v, s, where, negzero):
    """Plant the special elements into sample v (numpy f32, flat) at scale exponent s, all below its maximum and not
    on it; returns the positions used."""
    top = int(np.abs(v).argmax())
    amax = float(np.abs(v).max())
    where = [i + 1 if i == top else i for i in where]
    sc = 2.0 ** -float(s)
    vals = [TIE_DOWN * sc, TIE_UP * sc, LO_SUBNORMAL * sc, amax * 2.0 ** -20 * 1.2345]
    if negzero:
        vals.append(-0.0)
    for k, (i, val) in enumerate(zip(where, vals)):
        v[i] = np.float32(val)
        assert k == 3 or float(v[i]) == val, "the planted value must be an f32"
    assert float(np.abs(v).max()) == amax
    return where


def _check_images(img, B, act, amax, what):
    """decode_act16(img) == split_np(act, x3_exp(amax)) bit for bit (float16 patterns, the sign of zero included)."""
    h, l = decode_act16(img.cpu().numpy(), B)
    a = act.cpu().numpy()
    wh, wl = split_np(a, x3_exp(amax.cpu().numpy()))
    for name, got, want in (("h", h, wh), ("l", l, wl)):
        got16 = got.astype(np.float16)
        assert np.array_equal(got16.astype(np.float64), got)
        bad = got16.view(np.uint16) != want.view(np.uint16)
        first = [(tuple(int(i) for i in ix), float(a[tuple(ix)]).hex(), hex(int(got16.view(np.uint16)[tuple(ix)])),
                  hex(int(want.view(np.uint16)[tuple(ix)]))) for ix in np.argwhere(bad)[:4]]
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} {name} values differ from the numpy split; "
                               f"(index, act, got, want): {first}")


def _real_act(B, seed):
    g = torch.Generator().manual_seed(seed)
    act = torch.randn((B, 32, 26, 26), generator=g).clamp_min(0.0)
    act = act * (10.0 ** torch.linspace(-3, 3, B))[:, None, None, None] if B > 1 else act
    if B >= 5:
        act[1] = 0.0                                                     # a sample whose maximum is 0
    return act.contiguous()


@pytest.mark.parametrize("B", BATCHES)
def test_x3_images_match_the_numpy_split(gpu, B):
    """The images written by the forward (x3s tight and loose, x3sa) and by ops.cut_unpack_x3 of the encoded cut."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    act = _real_act(B, 2400 + B)
    a = act.numpy().reshape(B, -1)
    where = [26 * 5 + 3, 676 * 9 + 26 * 11 + 6, 676 * 17 + 26 * 25 + 25, 676 * 31 + 2, 676 * 24 + 26 * 7 + 23]
    used = {}
    for b in range(B):
        if np.abs(a[b]).max() > 0:
            used[b] = _plant(a[b], x3_exp(np.abs(a[b]).max()), where, negzero=True)
    assert len(used) >= max(1, B - 1)
    act = act.to(gpu)
    W2 = torch.randn(64, 32, 3, 3, device=gpu) * 0.05
    b2 = torch.zeros(64, device=gpu)
    am = ops.row_amax(act)
    assert (am == 0).any() or B < 5
    # tight: the planted ties are ties of THIS scale; loose: the same elements, no longer ties, still the split
    for name, amx in (("tight", am), ("loose", am * 16)):
        img = _img(B, gpu)
        ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=amx, act16=img)
        _check_images(img, B, act, amx, f"x3s {name}")
        if name == "tight":
            h, l = (t.reshape(B, -1) for t in decode_act16(img.cpu().numpy(), B))
            for b, w in used.items():
                assert (h[b, w[0]], l[b, w[0]]) == (1024.0, 0.5) and (h[b, w[1]], l[b, w[1]]) == (1026.0, -0.5)
                assert (h[b, w[2]], l[b, w[2]]) == (0.125, 3 * 2.0 ** -20)
                assert np.signbit(h[b, w[4]]) and h[b, w[4]] == 0 and not np.signbit(l[b, w[4]])
        # the received cut: mask + values + ranks -> images at the same scales
        n = act.numel()
        codec = CutCodec()
        bk = codec.buffers("img", n, gpu)
        codec.encode(act, bk)
        rk = codec.ranks("img", n, bk)
        img2 = _img(B, gpu)
        ops.cut_unpack_x3(bk[4], bk[0], rk, amx, img2)
        _check_images(img2, B, act, amx, f"cut_unpack_x3 {name}")
    img = _img(B, gpu)
    am1 = torch.full((B,), -1.0, device=gpu)
    ops.conv2_fwd_pool(act, W2, b2, impl="x3", act16=img, act_amax_out=am1)
    assert torch.equal(am1, am)
    _check_images(img, B, act, am1, "x3sa")


@pytest.mark.parametrize("B", BATCHES)
def test_conv1_x3_images_match_the_numpy_split(gpu, B):
    """ops.conv1_fwd_x3 on SyntheticMNIST: its images == the numpy split of the f32 act it returns at the amax it
    returns. Channel 0 is made the identity tap (W1[0] = centre 1, b1[0] = 0: act[:, 0] = relu(x) exactly), so
    elements planted into x - ties of the returned scale, a subnormal l, 2^-20 of the maximum - reach the split."""
    from splitcnn import ops
    from splitcnn.data import SyntheticMNIST, init_models
    a, _ = init_models(seed=7)
    W1, b1 = a.conv1.weight.detach().clone(), a.conv1.bias.detach().clone()
    W1[0] = 0.0
    W1[0, 0, 1, 1] = 1.0
    b1[0] = 0.0
    W1, b1 = W1.to(gpu).contiguous(), b1.to(gpu).contiguous()
    x, _ = SyntheticMNIST(2500 + B).batch(B)
    x = x.clone()
    am0 = torch.full((B,), -1.0, device=gpu)
    ops.conv1_fwd_x3(x.to(gpu), W1, b1, am0, _img(B, gpu))                # the scale bound depends on max |x| only
    s = x3_exp(am0.cpu().numpy())
    pix = [(3, 4), (10, 21), (17, 9), (25, 25)]                           # cut pixels (y, x) of channel 0
    xn = x.numpy()
    spots = []
    for b in range(B):
        sc = 2.0 ** -float(s[b])
        xmax = float(np.abs(xn[b]).max())
        vals = [TIE_DOWN * sc, TIE_UP * sc, LO_SUBNORMAL * sc, float(am0[b]) * 2.0 ** -20 * 1.2345]
        assert max(vals) < xmax
        top = divmod(int(np.abs(xn[b, 0]).argmax()), 28)
        spots.append([(yy, xx - 1) if (yy + 1, xx + 1) == top else (yy, xx) for yy, xx in pix])   # never on the max
        for (yy, xx), v in zip(spots[b], vals):
            xn[b, 0, yy + 1, xx + 1] = np.float32(v)
        assert float(np.abs(xn[b]).max()) == xmax
    x = x.to(gpu).contiguous()
    am = torch.full((B,), -1.0, device=gpu)
    img = _img(B, gpu)
    act = ops.conv1_fwd_x3(x, W1, b1, am, img, act=_nan((B, 32, 26, 26), gpu))
    assert torch.equal(am, am0)
    assert torch.equal(act[:, 0], x[:, 0, 1:27, 1:27].clamp_min(0.0))
    _check_images(img, B, act, am, "conv1_fwd_x3")
    h, l = decode_act16(img.cpu().numpy(), B)
    for b in range(B):
        (t0, t1, t2, _) = spots[b]
        assert (h[b, 0][t0], l[b, 0][t0]) == (1024.0, 0.5) and (h[b, 0][t1], l[b, 0][t1]) == (1026.0, -0.5)
        assert (h[b, 0][t2], l[b, 0][t2]) == (0.125, 3 * 2.0 ** -20)
