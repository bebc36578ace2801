"""GPU: the persistent conv kernels EXACTLY (torch.equal against float64) at the smallest batches where their
operand pipelines reach the steady state. The older exact tests stop at two units per workgroup (K2: B = 130,
per = 2) and two tiles per K share (K5: B = 37); every buffer or ring slot is then written once and read once.

Operands, references and exactness arguments are the existing ones: tests/test_x3_exact_gpu.py (integer operands
that are f16 values: wide and narrow), tests/test_x3_lo_exact_gpu.py with tests/x3_split_ref.py (operands with
nonzero low halves; expectation = the three-term float64 sum), tests/wide_ref64.py (K5, magnitudes <= 3). The
precondition (absolute-value sums below 2^24, or 2^24 finest granules) is asserted on the reference side before any
launch. Outputs are pre-filled with NaN, images with 0x5A, codes with 0xEE / 0xFF (K5).

Batches, re-derived from the launch code (csrc/slk_x3.hip; restated in tests/unit_partition.py and asserted claim by
claim in tests/test_unit_partition_cpu.py). A workgroup or K share walks the contiguous range of per = ceil(n / G)
units starting at i per; forward, dgrad pairs and the images-fed weight gradient have n = 3 B and G = 256:
  B = 171  per = 3: 171 workgroups of 3 units (one whole sample each), 85 idle. Position 2 is the first to read a
           REFILLED two-slot buffer: dgrad's x / ReLU-bit buffer (c1w) and mask words (pack), the f32 forward's raw
           rows, the images-fed weight gradient's (x3p) image and dY record buffers. The f32-act weight gradient
           (128 shares) has per = 5 (102 shares of 5, one of 3, 25 idle): a share such as units 5..9 spans three
           samples.
  B = 258  per = 4: 193 workgroups of 4, one of 2, 62 idle; sample boundaries fall inside ranges. The act16-reading
           forward (x3i, x3p) keeps three ring slots (read k % 3, request unit u + 2 into (k + 2) % 3): the request
           at position 1 is the first that is not the clamped "never read" one and lands in a slot read before
           (slot 0, read again at position 3). The deferred epilogue (pend, p_o, p_pre, p_us) crosses three unit
           boundaries, one of them a sample boundary with another scale. The amax forward (x3sa, G = min(B, 256),
           whole samples) has per = 6 in 129 workgroups (two samples each; the 127 others idle). f32-act weight
           gradient: per = 7.
  B = 342  per = 5: 205 workgroups of 5, one of 1, 50 idle. A range such as units 5..9 spans three samples: three
           distinct dY scale exponents meet in one x3p share (its LDS table sbt holds three entries). The x3i ring
           refills slots 0 and 1. x3sa: 171 workgroups of 6. f32-act weight gradient: per = 9 (three samples).
  B = 512  per = 6, all 256 workgroups busy, no short range: the x3i ring refills all three slots (a full turn).
           Forward and dgrad only (per-sample outputs: their bounds do not grow with B).
Direct and Winograd presets on the f16-exact operands at B = 258 and 513; their walks are strided, not contiguous
(csrc/slk_server.hip, csrc/slk_wino.hip). The direct forward and dgrad and the Winograd dgrad walk whole samples b,
b + 256, b + 512 through two buffers: B = 258 gives workgroups 0 and 1 a second sample, B = 513 gives workgroup 0
its first third one (the first read of a refilled buffer). The Winograd forward walks super-units su, su + 256, ...
of the ceil(3 B / 2) pairs of bands (band 2 su + pr = a third of a sample): B = 258 gives 131 workgroups two
super-units and no more, B = 513 gives every workgroup three and workgroups 0 and 1 four. Their weight gradients
stay at B <= 130 (the 2^20 Winograd bound does not fit more).

Inputs that keep the bounds (chosen, not tolerances). The weight gradient and the client backward sum over the
batch, so the product of their two densities is scaled by 130 / B from the values test_x3_lo_exact_gpu uses at
B = 130: dpooled 0.05 x 130 / B (14-bit dpooled 0.02 x 130 / B; act stays 0.05), ReLU bits min(0.25, 8 / (676 B))
in the lo classes (already ~ 1 / B) and 0.25 x 130 / B in the f16 classes (x stays 0.25). The f16-exact wide ranges
need no thinning for the weight gradient (about 6.7 k per sample and element: 2.3 M at B = 342). So that a thinned
case cannot pass by being empty, at least 0.9 of the expected dW2 elements must be nonzero (asserted).

K5 weight gradients (csrc/slk_wide.hip, wide_wgrad_kernel): share ks walks tile slots ks, ks + KSPLIT, ... while
valid; the tile buffer is double-buffered, and conv2 (SPLIT) also double-buffers the raw pooled dC and requests it
TWO tiles ahead (`valid(t + 2 * KSPLIT)`), which first runs when a share owns three tiles.
  conv2  WgCfg<64,128,32,4>:  64 slots per 8 images, KSPLIT 256. B = 65: shares 0, 8, ..., 56 own a third tile
         (image 64's 8 row blocks), 248 own two. B = 131: 4 tiles (232 shares) or 5 (24). B = 261: 8 (216) or 9 (40).
  conv3  WgCfg<128,256,16,8>: 16 slots per 8 images, KSPLIT 64. B = 131: 4 (58) or 5 (6). B = 261: 8 (54) or 9 (10).
Each runs on eight code patterns in five families aimed at sp_expand's index byte `ib`, its row-parity mask `rowp`
and the d = 0 / 1 record halves: uniform 0..4; every window at one position (0, 1, 2, 3); all blocked (every slab
element and db must be +0); the position cycling 0, 1, 2, 3 along the pooled columns (the four windows of one staging
item all differ); the position cycling along the channels of a C8 chunk.

Guards. Where a grid is queryable it is asserted to be what this derivation assumes (a changed grid fails here and
forces the batches to be re-derived). In every case the reference side asserts that, inside every workgroup's range,
what the unit at position k produces (forward: pooled and codes; dgrad: the cut gradient of the pair) or consumes
(weight gradients: the unit's act rows and routed dY, K5: the tile's input and pooled gradient) differs from that of
the units at k - 2 and k - 3 (the strided presets: from the samples 256 and 512, or the bands 512 and 1024, before
it): a stale buffer or ring slot cannot reproduce the right answer. The dgrad's two special
samples (1: all blocked, 2: one routed window) are exempt among themselves: their gradients are zero by design. The
lo classes' ReLU bits are sparse by their bound (8 set bits per channel in the whole batch), so the fused client
backward's steady state rests on the f16 classes, where the per-pair contributions to [dW1 | db1] are asserted to
differ too.
"""
import pytest
import torch
import torch.nn.functional as F

import unit_partition as P
import wide_ref64 as R
from ref64 import conv_relu64, dgrad64, route64, routing64, wgrad64
from test_wide_conv_gpu import _ref_wgrad, _run_wgrad
from test_x3_exact_gpu import WINO_LIMIT, _assert_bound, _c1_ref64, _exact_case, encode_relu_bits
from test_x3_lo_exact_gpu import (_amax_forms, _assert_fwd, _check_images, _img, _nan, dgrad_case, fwd_case,
                                  wgrad_case, wgrad_densities)
from x3_split_ref import x3_exp

pytestmark = pytest.mark.gpu

CHUNK = 128                       # float64 conv chunk (samples)
F16 = ("wide", "narrow")
PART_PIX = (0, 240, 464, 676)     # dgrad part pt = cut pixels [16 x3d_t0(pt), 16 x3d_t0(pt + 1)) (43 M tiles of 16)


def _chunked(f, batched, *rest):
    """f over the batch in chunks; `batched` is a tuple of per-sample operands."""
    B = batched[0].shape[0]
    return torch.cat([f(*(t[s:s + CHUNK] for t in batched), *rest) for s in range(0, B, CHUNK)])


def _conv_relu(act, W2, b2):
    return _chunked(conv_relu64, (act,), W2, b2)


def _dgrad(dc, W2):
    return _chunked(dgrad64, (dc,), W2)


def _differ(units, ranges, exempt=None, what=""):
    """units [n, ...]: unit u differs from units u - 2 and u - 3 wherever both lie in one range."""
    a, b = P.lag_pairs(ranges)
    if exempt is not None:
        keep = [i for i, (x, y) in enumerate(zip(a, b)) if not (exempt(x) and exempt(y))]
        a, b = [a[i] for i in keep], [b[i] for i in keep]
    assert len(a) > 0, f"{what}: no range is three units long"
    u = units.reshape(units.shape[0], -1)
    a, b = (torch.tensor(t, device=u.device) for t in (a, b))
    same = (u[a] == u[b]).all(dim=1)
    assert not same.any(), f"{what}: {int(same.sum())} units equal a unit 2 or 3 positions before them"


def _bands(t, rows, step):
    """[B, C, H, W] -> the three units' row bands [3 B, C * rows * W]: unit i of a sample is rows i * step .. + rows."""
    return torch.stack([t[:, :, i * step:i * step + rows] for i in range(3)], dim=1).reshape(3 * t.shape[0], -1)


# ----------------------------------------------------------------------------- K2 forward
def _fwd_operands(cls, B, dev):
    if cls in F16:
        c = _exact_case(dev, B, seed=11000 + B, narrow=cls == "narrow")
        act, W2, b2 = c["act"], c["W2"], c["b2"]
        _assert_bound(_conv_relu(act.abs(), W2.abs(), b2.abs()))
        want_c, win = routing64(_conv_relu(act, W2, b2))
        return act, W2, b2, win.max(-1).values, want_c
    return fwd_case(cls, B, 21000 + B, dev)


def fwd_guards(B, want_p, want_c):
    """Reference side: every unit's pooled rows and codes differ from those 2 and 3 positions before it, in the
    ranges of the unit-partitioned forward and of the whole-sample amax forward."""
    units = torch.cat([_bands(want_p, 4, 4), _bands(want_c.double(), 4, 4)], dim=1)
    _differ(units, P.x3_fwd(B)[1], what="forward")
    _differ(units, P.x3_fwd_amax(B)[1], what="amax forward")


@pytest.mark.parametrize("B", [171, 258, 342, 512])
@pytest.mark.parametrize("cls", ["wide", "narrow", "act14", "act18", "w14", "both"])
def test_x3_fwd_steady(gpu, cls, B):
    """impl="x3" in its five forms - f32 cut (x3), writing images (x3s), reading them (x3i), code-less (x3p), amax
    in the kernel (x3sa): pooled and codes == float64 in every window; the images of x3s / x3sa == the numpy split,
    every byte."""
    from splitcnn import ops
    act, W2, b2, want_p, want_c = _fwd_operands(cls, B, gpu)
    fwd_guards(B, want_p, want_c)
    shp = (B, 64, 12, 12)

    def outs():
        return dict(pooled=_nan(shp, gpu), code=torch.full(shp, 0xEE, dtype=torch.uint8, device=gpu))

    for name, am in _amax_forms(act):
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, **outs()), want_p, want_c, f"x3 {name}")
        a16 = _img(B, gpu)
        _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act_amax=am, act16=a16, **outs()), want_p, want_c,
                    f"x3s {name}")
        _check_images(a16, B, act, am, f"x3s {name}")
        _assert_fwd(*ops.conv2_fwd_pool_x3i(a16, am, W2, b2, **outs()), want_p, want_c, f"x3i {name}")
        _assert_fwd(ops.conv2_fwd_pool_x3p(a16, am, W2, b2, pooled=_nan(shp, gpu)), None, want_p, want_c, f"x3p {name}")
    a16 = _img(B, gpu)
    am1 = torch.full((B,), -1.0, device=gpu)
    _assert_fwd(*ops.conv2_fwd_pool(act, W2, b2, impl="x3", act16=a16, act_amax_out=am1, **outs()), want_p, want_c,
                "x3sa")
    assert torch.equal(am1, ops.row_amax(act))
    _check_images(a16, B, act, am1, "x3sa")


# ----------------------------------------------------------------------------- K2 input gradient
def _special_codes(code):
    code[1:3] = 4                 # sample 1 blocked everywhere, sample 2 one routed window
    code[2, 17, 5, 7] = 2
    return code


def f16_relu_density(B):
    return 0.25 * 130 / B


def _c1_pairs(x, gm):
    """The fused client backward's contribution of every pair (sample, part): [3 B, 320] float64."""
    B = x.shape[0]
    win = F.unfold(x.double(), 3)                                    # B, 9, 676
    g = gm.reshape(B, 32, 676)
    out = []
    for pt in range(3):
        s = slice(PART_PIX[pt], PART_PIX[pt + 1])
        dW = torch.einsum("bcp,bkp->bck", g[:, :, s], win[:, :, s]).reshape(B, 288)
        out.append(torch.cat([dW, g[:, :, s].sum(-1)], dim=1))
    return torch.stack(out, dim=1).reshape(3 * B, 320)


def dgrad_operands(cls, B, dev):
    """(dp, W2, code, x, relu, g64, c1) with the bounds asserted."""
    if cls not in F16:
        dp, W2, code, x, relu, _, g64, c1 = dgrad_case(cls, B, 22000 + B, dev, special=True)
        return dp, W2, code, x, relu, g64, c1
    c = _exact_case(dev, B, seed=12000 + B, narrow=cls == "narrow", relu_p=f16_relu_density(B))
    W2, dp, x, relu = c["W2"], c["dp"], c["x"], c["relu"]
    code = _special_codes(c["code"])
    dc = route64(dp, code)
    _assert_bound(_dgrad(dc.abs(), W2.abs()))
    g64 = _dgrad(dc, W2)
    gm = torch.where(relu, g64, torch.zeros_like(g64))
    _assert_bound(_c1_ref64(x.abs(), gm.abs()))
    return dp, W2, code, x, relu, g64, _c1_ref64(x, gm)


def dgrad_guards(cls, B, code, x, relu, g64):
    ranges = P.x3_dgrad(B)[1]
    g = g64.reshape(B, 32, 676)
    units = torch.stack([g[:, :, PART_PIX[pt]:PART_PIX[pt] + 212] for pt in range(3)], dim=1).reshape(3 * B, -1)
    special = lambda p: p // 3 in (1, 2)                           # noqa: E731
    assert float(g64[1].abs().max()) == 0.0 and int((g64[2] != 0).sum()) <= 32 * 9
    assert int((code[2] < 4).sum()) == 1
    _differ(units, ranges, exempt=special, what="dgrad")
    # c1w's buffered operands: a pair's x differs from the x of the pairs 2 and 3 before it in another sample
    xs = x.reshape(B, -1).repeat_interleave(3, dim=0)
    a, b = P.lag_pairs(ranges)
    ab = [(p, q) for p, q in zip(a, b) if p // 3 != q // 3]
    assert len(ab) > 0 or B == 171                                   # B = 171: a range is one sample
    if ab:
        a, b = (torch.tensor(t, device=x.device) for t in zip(*ab))
        assert not (xs[a] == xs[b]).all(dim=1).any()
    if cls in F16:
        gm = torch.where(relu, g64, torch.zeros_like(g64))
        _differ(_c1_pairs(x, gm), ranges, exempt=special, what="client backward")


@pytest.mark.parametrize("B", [171, 258, 342, 512])
@pytest.mark.parametrize("cls", ["wide", "narrow", "dp14", "dp18", "w14", "both"])
def test_x3_dgrad_steady(gpu, cls, B):
    """slk_conv2_dgrad_x3 and slk_conv2_dgrad_x3_c1w on uniform codes with one sample all blocked and one with a
    single routed window: the cut gradient, and the float64 sum and slk_reduce_slabs of the client slabs."""
    from splitcnn import ops
    assert ops.conv2_dgrad_c1w_nslab(B) == min(3 * B, 256)
    dp, W2, code, x, relu, g64, c1 = dgrad_operands(cls, B, gpu)
    dgrad_guards(cls, B, code, x, relu, g64)
    bits = encode_relu_bits(relu)
    for name, dpa in _amax_forms(dp):
        gx = ops.conv2_dgrad(dp, code, W2, impl="x3", dp_amax=dpa, out=_nan((B, 32, 26, 26), gpu))
        bad = gx.double() != g64
        assert not bad.any(), f"x3 dgrad ({name}): {int(bad.sum())} of {bad.numel()} differ"
        assert float(gx[1].abs().max()) == 0.0
        slabs = ops.conv2_dgrad_client_slabs(dp, code, W2, x, bits, dp_amax=dpa,
                                             slabs=_nan((ops.conv2_dgrad_c1w_nslab(B), 320), gpu))
        bad = slabs.double().sum(0) != c1
        assert not bad.any(), f"fused client backward ({name}): {int(bad.sum())} of 320 slab sums differ"
        assert torch.equal(ops.reduce_slabs(slabs).double(), c1), f"reduce_slabs of the client slabs ({name})"


# ----------------------------------------------------------------------------- K2 weight gradient
WGRAD_B = [171, 258, 342]
MIN_NONZERO = 0.9


def steady_densities(cls, B):
    """test_x3_lo_exact_gpu's densities at B = 130 with the dpooled one scaled by 130 / B."""
    pa, pd = wgrad_densities(cls, 130)
    return pa, pd * 130 / B


def wgrad_operands(cls, B, dev):
    """(act, dp, code, want [dW2 | db2]) with the bound and the non-emptiness asserted."""
    if cls in F16:
        c = _exact_case(dev, B, seed=13000 + B, narrow=cls == "narrow")
        act, dp, code = c["act"], c["dp"], c["code"]
        dc = route64(dp, code)
        dWa, dba = wgrad64(act.abs(), dc.abs(), chunk=CHUNK)
        _assert_bound(torch.cat([dWa.reshape(-1), dba]))
        dW, db = wgrad64(act, dc, chunk=CHUNK)
        want = torch.cat([dW.reshape(-1), db])
    else:
        act, dp, code, want = wgrad_case(cls, B, 23000 + B, dev, densities=steady_densities(cls, B))
    nz = float((want[:18432] != 0).double().mean())
    assert nz >= MIN_NONZERO, f"only {nz:.3f} of the expected dW2 elements are nonzero"
    return act, dp, code, want


def wgrad_guards(cls, B, act, dp, code):
    f32, img = P.x3_wgrad_f32(B)[1], P.x3_wgrad_images(B)[1]
    dc = route64(dp, code)
    dyu = _bands(dc, 8, 8)                                                   # a unit: 8 dY rows, 10 act rows
    units = torch.cat([_bands(act.double(), 10, 8), dyu], dim=1)
    for ranges, what in ((f32, "f32-act wgrad"), (img, "images wgrad")):
        _differ(units, ranges, what=what)
        _differ(dyu, ranges, what=what + " dY")
    if cls.startswith("mixed"):
        # three consecutive samples in one share = three distinct values of each scale exponent (ka, kd by b mod 3)
        assert P.sample_span(f32) >= 3
        assert (P.sample_span(img) >= 3) == (B == 342)
        for t in (act, dp):
            e = x3_exp(t.flatten(1).abs().max(1).values.cpu().numpy())
            u0, u1 = next((u0, u1) for u0, u1 in (img if B == 342 else f32) if (u1 - 1) // 3 - u0 // 3 >= 2)
            assert len(set(e[u0 // 3:(u1 - 1) // 3 + 1].tolist())) >= 3


WGRAD_CASES = [(c, B) for c in ("wide", "narrow", "act14", "dp14", "both", "mixed_act", "mixed_dp") for B in WGRAD_B]


@pytest.mark.parametrize("cls,B", WGRAD_CASES)
def test_x3_wgrad_steady(gpu, cls, B):
    """slk_conv2_wgrad_x3 (f32 act) and slk_conv2_wgrad_x3s (images, 2:4 sparse): the float64 slab sum and
    ops.reduce_slabs == [dW2 | db2] at every pairing of tight and loose scale bounds."""
    from splitcnn import ops
    nslab = ops.conv2_wgrad_nslab(B, impl="x3")
    assert nslab == min(6 * B, 256)
    act, dp, code, want = wgrad_operands(cls, B, gpu)
    wgrad_guards(cls, B, act, dp, code)
    W2 = torch.zeros(64, 32, 3, 3, device=gpu)
    W2[:, 0, 1, 1] = 1.0
    b2 = torch.zeros(64, device=gpu)
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


# ----------------------------------------------------------------------------- direct and Winograd presets
F32_B = [258, 513]


def _strided_differ(units, stride, what):
    """units [n, ...] walked u, u + stride, u + 2 stride, ... by one workgroup through two buffers: every unit
    differs from the one and the two positions before it."""
    u = units.reshape(units.shape[0], -1)
    for lag in (stride, 2 * stride):
        if u.shape[0] > lag:
            same = (u[lag:] == u[:-lag]).all(dim=1)
            assert not same.any(), f"{what}: {int(same.sum())} units equal the unit {lag} before them"


@pytest.mark.parametrize("B", F32_B)
@pytest.mark.parametrize("impl", ["direct", "wino"])
@pytest.mark.parametrize("narrow", [False, True], ids=["wide", "narrow"])
def test_f32_fwd_steady(gpu, impl, B, narrow):
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=14000 + B, narrow=narrow)
    act, W2, b2 = c["act"], c["W2"], c["b2"]
    _assert_bound(_conv_relu(act.abs(), W2.abs(), b2.abs()))
    if impl == "wino":
        bound = 9 * 32 * (4 * float(act.abs().max())) * (2.25 * float(W2.abs().max())) + float(b2.abs().max())
        assert bound < WINO_LIMIT, bound
    want_c, win = routing64(_conv_relu(act, W2, b2))
    want_p = win.max(-1).values
    assert P.length_counts(P.strided(B, 256)) == {258: {2: 2, 1: 254}, 513: {3: 1, 2: 255}}[B]
    assert P.length_counts(P.wino_fwd(B)) == {258: {2: 131, 1: 125}, 513: {4: 2, 3: 254}}[B]
    if impl == "wino":     # bands 2 su + pr, super-units 256 apart: bands 512 and 1024 apart share a workgroup
        units = torch.cat([_bands(want_p, 4, 4), _bands(want_c.double(), 4, 4)], dim=1)
        _strided_differ(units, 512, "Winograd forward bands")
    else:                  # whole samples 256 apart
        _strided_differ(torch.cat([want_p.flatten(1), want_c.double().flatten(1)], dim=1), 256, "direct forward")
    shp = (B, 64, 12, 12)
    got = ops.conv2_fwd_pool(act, W2, b2, impl=impl, pooled=_nan(shp, gpu),
                             code=torch.full(shp, 0xEE, dtype=torch.uint8, device=gpu))
    _assert_fwd(*got, want_p, want_c, impl)


@pytest.mark.parametrize("B", F32_B)
@pytest.mark.parametrize("impl", ["direct", "wino"])
def test_f32_dgrad_steady(gpu, impl, B):
    from splitcnn import ops
    c = _exact_case(gpu, B, seed=15000 + B)
    W2, dp = c["W2"], c["dp"]
    code = _special_codes(c["code"])
    dc = route64(dp, code)
    _assert_bound(_dgrad(dc.abs(), W2.abs()))
    if impl == "wino":
        bound = 9 * 64 * (4 * float(dp.abs().max())) * (2.25 * float(W2.abs().max()))
        assert bound < WINO_LIMIT, bound
    g64 = _dgrad(dc, W2)
    # both presets: whole samples strided by the 256 workgroups, sample b, b + 256, b + 512 through two buffers.
    # (Samples 1 and 2, zero by design, meet only nonzero ones: 257 / 258 and 513 / 514 are ordinary or absent.)
    assert P.length_counts(P.strided(B, 256)) == {258: {2: 2, 1: 254}, 513: {3: 1, 2: 255}}[B]
    _strided_differ(g64, 256, f"{impl} dgrad")
    _strided_differ(dc, 256, f"{impl} dgrad dY")
    g = ops.conv2_dgrad(dp, code, W2, impl=impl, out=_nan((B, 32, 26, 26), gpu))
    bad = g.double() != g64
    assert not bad.any(), f"{impl} dgrad: {int(bad.sum())} of {bad.numel()} differ"
    assert float(g[1].abs().max()) == 0.0 and int((g[2] != 0).sum()) <= 32 * 9


# ----------------------------------------------------------------------------- K5 weight gradients
K5_CFG = {2: P.WG2, 3: P.WG3}
K5_BATCHES = [(2, 65), (2, 131), (2, 261), (3, 131), (3, 261)]
K5_FAMILIES = ["uniform", "pos0", "pos1", "pos2", "pos3", "blocked", "columns", "channels"]


def k5_codes(fam, code):
    """The code pattern of a family, in the shape of the uniform draw `code` [B, CO, h, w] (int64)."""
    if fam == "uniform":
        return code
    if fam.startswith("pos"):
        return torch.full_like(code, int(fam[3]))
    if fam == "blocked":
        return torch.full_like(code, R.CODE_NONE)
    n = code.shape[3] if fam == "columns" else code.shape[1]
    idx = torch.arange(n, device=code.device) & 3
    idx = idx[None, None, None, :] if fam == "columns" else idx[None, :, None, None]
    return idx.expand_as(code).contiguous()


def _k5_operands(layer, B, dev):
    """The operands of one (layer, batch): the operand and bound preconditions, and the tile guard, are asserted
    here. The bound is taken with |d| routed to ALL four positions of every window at once, which dominates the
    absolute-value sum of every code pattern."""
    inp, d, code = R.wgrad_case(layer, B, "exact", seed=16000 * layer + B, device=dev)
    R.assert_exact_operands(inp, d)
    every = d.abs().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    dW, db = R.conv_wgrad(inp.abs(), every)
    R.assert_abs_bound(torch.cat([dW.reshape(-1), db]))
    cfg = K5_CFG[layer]
    RB, K = P.wg_rb(cfg), P.wg_ksplit(cfg)
    # tile (n, rb) consumes TR input rows (+ halo) and TR / 2 pooled rows: those of tile k differ from k - 2, k - 3
    ti = inp.reshape(B, cfg.CI, RB, cfg.TR * cfg.HW).permute(0, 2, 1, 3).reshape(B * RB, -1)
    td = d.reshape(B, cfg.CO, RB, (cfg.TR // 2) * (cfg.HW // 2)).permute(0, 2, 1, 3).reshape(B * RB, -1)
    a, b = [], []
    for ks in range(K):
        ids = [n * RB + rb for n, rb in (P.tile_of(cfg, t) for t in P.share_tiles(cfg, ks, B))]
        for k in range(len(ids)):
            for lag in (2, 3):
                if k - lag >= 0:
                    a.append(ids[k])
                    b.append(ids[k - lag])
    assert len(a) > 0, "no share owns a third tile"
    a, b = (torch.tensor(t, device=inp.device) for t in (a, b))
    assert not (ti[a] == ti[b]).all(dim=1).any() and not (td[a] == td[b]).all(dim=1).any()
    return inp, d, code


@pytest.fixture(scope="module", params=K5_BATCHES, ids=lambda p: f"conv{p[0]}-{p[1]}")
def k5_case(request, gpu):
    """One (layer, batch)'s operands, shared by its code families, never modified, freed after the last of them."""
    layer, B = request.param
    return (layer, B) + _k5_operands(layer, B, gpu)


@pytest.mark.parametrize("fam", K5_FAMILIES)
def test_k5_wgrad_steady(gpu, k5_case, fam):
    """slk_wide_conv2_wgrad / slk_wide_conv3_wgrad where a share owns 3 to 9 tiles: the float64 sum of the slabs and
    slk_reduce_slabs == the reference exactly, on every code family."""
    from splitcnn import _lib
    layer, B, inp, d, code = k5_case
    assert _lib.query(f"slk_wide_conv{layer}_wgrad_nslab", B) == P.wg_ksplit(K5_CFG[layer]) == {2: 256, 3: 64}[layer]
    code = k5_codes(fam, code)
    want = _ref_wgrad(layer, inp, d, code)
    slabs, red = _run_wgrad(gpu, layer, inp, d, code)
    bad = slabs.double().sum(0) != want
    assert not bad.any(), f"conv{layer} wgrad {fam} B={B}: {int(bad.sum())} of {bad.numel()} slab sums differ"
    assert torch.equal(red.double(), want), f"slk_reduce_slabs, conv{layer} {fam} B={B}"
    if fam == "blocked":
        assert float(want.abs().max()) == 0.0
        assert (slabs.view(torch.int32) == 0).all() and (red.view(torch.int32) == 0).all(), "a blocked batch is not +0"
    else:
        assert float((want != 0).double().mean()) >= MIN_NONZERO
