"""Every K5 conv kernel (csrc/slk_wide.hip, csrc/slk_wide_head.hip's shadows) called ALONE through its entry point,
against the float64 reference of tests/wide_ref64.py on the same operands: exactly where that is possible, at the
project's bf16 bars otherwise.

Each launch gets fresh operands in the C8 layouts, shadows from wide.build_shadows, and output buffers pre-filled with
NaN (values) / 0xFF (codes): every test asserts that nothing was left unwritten. Nothing flows from one kernel into the
next, so a failure names its kernel.

Exact regime (wide_ref64's docstring): integer operands, absolute-value sums below 2^24, so the f32 accumulation is
exact in any order and the stored bf16 / code / f32 slab must EQUAL the reference bit for bit, with no element excused
and no tie waived. Both preconditions are asserted on the reference side in every exact test. The wide variant makes
the bf16 store round (14 % / 22 % of the outputs are exact halfway cases); the narrow variant makes window ties
(3-4 % of the windows), maxima of exactly 0 (1.5-2.4 %) and every first-max position (24-26 % each) —
tests/test_wide_ref64_cpu.py asserts those shares.

Batch sizes = the smallest that reach each path of the persistent kernels. Re-derived from the code: tile_state<C>
maps tile index t to XCD t & 7 and j = t >> 3, image n = (j / (RB * NCB)) * 8 + (t & 7), so every group of 8 images
takes 8 * RB * NCB tile indices and a ragged last group leaves invalid slots; launch_conv's grid is
min(512 (4 waves) or 256 (8 waves), 8 * ceil(B / 8) * RB * NCB) and a workgroup walks t, t + grid, ...
  conv2 forward  Conv32Cfg<64,128,32>:                   NPX 256, TR 8,  RB 4, NCB 1 -> 4 tiles/image, grid 512
  conv3 forward  ConvCfg<128,256,16,128,FWD,4,4>:         NPX 128, TR 8,  RB 2, NCB 2 -> 4 tiles/image, grid 512
  conv2 dgrad    ConvCfg<128,64,32,64,MASK,4,4,EXP>:      NPX 256, TR 8,  RB 4, NCB 1 -> 4 tiles/image, grid 512
  conv3 dgrad    ConvCfg<256,128,16,128,PLAIN,4,8,EXP>:   NPX 256, TR 16, RB 1, NCB 1 -> 1 tile/image,  grid 256
  B = 1    the smallest launch (grid 32 / 8: 7 of every 8 slots invalid);
  B = 9    one image past the 8-XCD group: the second group has 7 invalid slots of every 8;
  B = 37   ragged (5 groups, the last with 5 of 8 images); every workgroup still owns at most one tile;
  B = 131  the three 4-tiles-per-image kernels: 128 images fill the 512 workgroups' first round, tiles 512..543 are
           images 128..135 of which 3 exist: 12 workgroups run a second tile, 20 meet an invalid `nxt` after a
           valid tile (conv3 dgrad: still one round, span 136);
  B = 261  conv3 dgrad: 256 images fill its 256 workgroups, tiles 256..263 hold 5 valid and 3 invalid slots (its
           first second round); the other three run a third round (span 1056 = 2 x 512 + 32, 20 of 32 valid).
Weight gradients: conv2 / conv3 (256 workgroups = NBLK blocks x KSPLIT K shares, share ks walks tile slots ks,
ks + KSPLIT, ... of the same XCD-grouped slot order; WgCfg<64,128,32,4>: NBLK 1, KSPLIT 256, 8 tiles/image;
WgCfg<128,256,16,8>: NBLK 4, KSPLIT 64, 2 tiles/image) at B = 9 (128 / 32 slots: half the shares get none, the others
one slot, 7 of 8 of the second group's invalid) and B = 37 (320 / 80 slots: 64 / 16 shares get two, the rest one);
conv1 (grid 512, images strided by 512) also at B = 515, where workgroups
0..2 take two images and the rest one; at B = 37 the 475 idle workgroups must write zero slabs.
conv1 forward (grid min(B, 2048), images strided): B = 2053 gives 5 workgroups a second image.
"""
import pytest
import torch

import wide_ref64 as R

pytestmark = pytest.mark.gpu

BATCHES = [1, 9, 37, 131, 261]
NAN = float("nan")


# ----------------------------------------------------------------------------- plumbing
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _shadows(dev, W1=None, W2=None, W3=None):
    from splitcnn import wide
    sh = wide.new_shadows(dev)
    for v in sh.values():
        v.view(torch.int16).fill_(-64)   # 0xFFC0: a NaN pattern
    Ws = [torch.zeros(shape, device=dev) if w is None else w.to(torch.float32).contiguous()
          for w, shape in ((W1, (64, 3, 3, 3)), (W2, (128, 64, 3, 3)), (W3, (256, 128, 3, 3)))]
    wide.build_shadows(*Ws, sh, _stream())
    torch.cuda.synchronize()
    return sh


def _c8(t, dtype):
    from splitcnn.wide import nchw_to_c8
    return nchw_to_c8(t.to(dtype))


def _nchw(t):
    from splitcnn.wide import c8_to_nchw
    return c8_to_nchw(t).contiguous()


def _assert_written(values=None, codes=None):
    if values is not None:
        assert not torch.isnan(values.float()).any(), "an output value was left unwritten"
    if codes is not None:
        assert int(codes.max()) <= 4, "a routing code was left unwritten (or is out of range)"


def _assert_bits(got_bf16, want_f64, what):
    """got == bf16(want) bit for bit (so +0 and -0 differ); want's zeros are +0 (R.pos_zero)."""
    want = R.bf16(R.pos_zero(want_f64))
    bad = got_bf16.view(torch.int16) != want.view(torch.int16)
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} of {bad.numel()} stored values differ from bf16(float64); first at {i}: "
                             f"got {got_bf16[tuple(i)].item()!r}, want {want[tuple(i)].item()!r} "
                             f"(float64 {want_f64[tuple(i)].item()!r})")


def _assert_codes(got, want, what):
    bad = got.long() != want
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} of {bad.numel()} routing codes differ; first at {i}: got "
                             f"{int(got[tuple(i)])}, want {int(want[tuple(i)])}")


def _np(t):
    return t.double().cpu().numpy()


# ----------------------------------------------------------------------------- conv2 / conv3 forward
def _run_fwd(dev, layer, inp, W, b):
    from splitcnn import _lib
    B = inp.shape[0]
    CI, CO, HW = R.LAYERS[layer]
    sh = _shadows(dev, **{f"W{layer}": W})
    a = _c8(inp, torch.bfloat16)
    bias = b.to(torch.float32).contiguous()
    out = torch.full((B, CO // 8, HW // 2, HW // 2, 8), NAN, dtype=torch.bfloat16, device=dev)
    code = torch.full((B, CO // 8, HW // 2, HW // 2, 8), 0xFF, dtype=torch.uint8, device=dev)
    _lib.call(f"slk_wide_conv{layer}_fwd", a.data_ptr(), sh[f"w{layer}f"].data_ptr(), bias.data_ptr(), out.data_ptr(),
              code.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    out, code = _nchw(out), _nchw(code)
    _assert_written(out, code)
    return out, code


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("regime", ["wide", "narrow"])
@pytest.mark.parametrize("layer", [2, 3])
def test_conv_fwd_exact(gpu, layer, regime, B):
    """pooled bf16 and routing code of slk_wide_conv<layer>_fwd == the float64 reference, bit for bit, every window."""
    inp, W, b = R.fwd_case(layer, B, regime, seed=1000 * layer + B, device=gpu)
    R.assert_exact_operands(inp, W, b)
    R.assert_abs_bound(R.conv_fwd(inp.abs(), W.abs(), b.abs()))
    pooled, code = R.relu_pool_code(R.conv_fwd(inp, W, b))
    got_p, got_c = _run_fwd(gpu, layer, inp, W, b)
    _assert_codes(got_c, code, f"conv{layer} fwd {regime} B={B}")
    _assert_bits(got_p, pooled, f"conv{layer} fwd {regime} B={B}")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layer", [2, 3])
def test_conv_fwd_real(gpu, layer, B):
    """Real-valued operands, layer-isolated as tests/test_wide_gpu.py: codes equal float64's except numerical ties
    (codes_close), the pooled value within bf16_close of float64's value at the kernel's own code."""
    inp, W, b = R.fwd_case(layer, B, "real", seed=2000 * layer + B, device=gpu)
    c = R.conv_fwd(inp, R.bf16_f64(W), b)
    _, code = R.relu_pool_code(c)
    got_p, got_c = _run_fwd(gpu, layer, inp, W, b)
    R.codes_close(c.cpu().numpy(), got_c.long().cpu().numpy(), code.cpu().numpy())
    R.bf16_close(_np(got_p), _np(R.bf16_f64(R.pooled_at(c, got_c))))


# ----------------------------------------------------------------------------- conv3 / conv2 dgrad
def relu_words(relu):
    """[B,64,H,W] bool -> the ReLU words [B, H*W] int64, bit c = relu[c] (include/slk.h, slk_wide_conv1_fwd)."""
    B, C, H, Wd = relu.shape
    w = torch.zeros(B, H, Wd, dtype=torch.int64, device=relu.device)
    for c in range(C):
        w |= relu[:, c].long() << c
    return w.reshape(B, H * Wd).contiguous()


def _run_dgrad(dev, layer, dp, code, W, relu):
    from splitcnn import _lib
    B = dp.shape[0]
    CI, CO, HW = R.LAYERS[layer]
    sh = _shadows(dev, **{f"W{layer}": W})
    d8, c8 = _c8(dp, torch.bfloat16), _c8(code, torch.uint8)
    out = torch.full((B, CI // 8, HW, HW, 8), NAN, dtype=torch.bfloat16, device=dev)
    if layer == 3:
        _lib.call("slk_wide_conv3_dgrad", d8.data_ptr(), c8.data_ptr(), sh["w3d"].data_ptr(), out.data_ptr(), B, _stream())
    else:
        words = relu_words(relu)
        _lib.call("slk_wide_conv2_dgrad", d8.data_ptr(), c8.data_ptr(), sh["w2d"].data_ptr(), words.data_ptr(),
                  out.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    out = _nchw(out)
    _assert_written(out)
    return out


def _ref_dgrad(dp, code, Wb, relu):
    d = R.conv_dgrad(R.unpool(dp, code), Wb)
    return d if relu is None else torch.where(relu, d, torch.zeros_like(d))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layer", [3, 2])
def test_conv_dgrad_exact(gpu, layer, B):
    """slk_wide_conv3_dgrad / slk_wide_conv2_dgrad on arbitrary codes == bf16(float64) bit for bit; conv2's is exactly
    +0 wherever the ReLU bit is clear (random words, sample 0 all ones, sample 1 all zeros)."""
    dp, code, W, relu = R.dgrad_case(layer, B, "wide", seed=3000 * layer + B, device=gpu)
    R.assert_exact_operands(dp, W)
    R.assert_abs_bound(R.conv_dgrad(R.unpool(dp.abs(), code), W.abs()))
    want = _ref_dgrad(dp, code, W, relu)
    got = _run_dgrad(gpu, layer, dp, code, W, relu)
    _assert_bits(got, want, f"conv{layer} dgrad B={B}")
    if relu is not None:
        assert (got.view(torch.int16)[~relu] == 0).all(), "a ReLU-masked gradient is not +0"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layer", [3, 2])
def test_conv_dgrad_real(gpu, layer, B):
    dp, code, W, relu = R.dgrad_case(layer, B, "real", seed=4000 * layer + B, device=gpu)
    want = _ref_dgrad(dp, code, R.bf16_f64(W), relu)
    got = _run_dgrad(gpu, layer, dp, code, W, relu)
    R.bf16_close(_np(got), _np(R.bf16_f64(want)))
    if relu is not None:
        assert (got.view(torch.int16)[~relu] == 0).all(), "a ReLU-masked gradient is not +0"


# ----------------------------------------------------------------------------- conv1 forward, ReLU words
def _run_conv1(dev, x, W1, b1):
    from splitcnn import _lib
    B = x.shape[0]
    sh = _shadows(dev, W1=W1)
    xf, bias = x.to(torch.float32).contiguous(), b1.to(torch.float32).contiguous()
    a1 = torch.full((B, 8, 32, 32, 8), NAN, dtype=torch.bfloat16, device=dev)
    bits = torch.full((B, 1024), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    _lib.call("slk_wide_conv1_fwd", xf.data_ptr(), sh["w1b"].data_ptr(), bias.data_ptr(), a1.data_ptr(), bits.data_ptr(),
              B, _stream())
    bits2 = torch.full((B, 1024), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    _lib.call("slk_wide_relu_bits", a1.data_ptr(), bits2.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    _assert_written(a1)
    return _nchw(a1), bits, bits2


@pytest.mark.parametrize("B", [1, 9, 37, 2053])
@pytest.mark.parametrize("regime", ["wide", "narrow"])
def test_conv1_fwd_exact(gpu, regime, B):
    """a1 == bf16(relu(conv1(x) + b1)) bit for bit on integer operands; a1bits == (a1 > 0) packed bit c = channel c,
    one u64 per pixel; and == slk_wide_relu_bits of the stored a1."""
    x, W1, b1 = R.fwd_case(1, B, regime, seed=500 + B, device=gpu)
    R.assert_exact_operands(x, W1, b1)
    R.assert_abs_bound(R.conv_fwd(x.abs(), W1.abs(), b1.abs()))
    want = R.conv_fwd(x, W1, b1).clamp_min(0.0)
    a1, bits, bits2 = _run_conv1(gpu, x, W1, b1)
    _assert_bits(a1, want, f"conv1 fwd {regime} B={B}")
    words = relu_words(want > 0)
    assert torch.equal(bits, words), "a1bits != (a1 > 0)"
    assert torch.equal(bits2, words), "slk_wide_relu_bits(a1) != (a1 > 0)"


def _halfway_f32(shape, seed, dev):
    """Finite f32 values (both signs, biased exponents 110..140: no subnormal, no overflow) whose low 16 bits are exact
    bf16 halfway values, their two neighbours, and the two ends of a bf16 interval, with odd and even upper halves."""
    g = torch.Generator().manual_seed(seed)
    low = torch.tensor([0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF])[torch.randint(0, 6, shape, generator=g)]
    mant = torch.randint(0, 128, shape, generator=g)
    expo = torch.randint(110, 141, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g)
    bits = (sign << 31) | (expo << 23) | (mant << 16) | low
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32).to(dev)


def test_conv1_rounds_x_to_nearest_even(gpu):
    """Delta filters (one tap = +1 for channels 0..26, one tap = -1 for channels 27..53, bias 0) on an x of exact bf16
    halfway values and their neighbours: channel k returns relu(+-bf16(x)) at tap k's offset, round-to-nearest-even."""
    B = 3
    x = _halfway_f32((B, 3, 32, 32), 77, gpu)
    W1 = torch.zeros(64, 27, dtype=torch.float64, device=gpu)
    for k in range(27):
        W1[k, k], W1[27 + k, k] = 1.0, -1.0
    W1 = W1.reshape(64, 3, 3, 3)
    b1 = torch.zeros(64, dtype=torch.float64, device=gpu)
    xb = R.bf16_f64(x)
    assert R.halfway_share(x) >= 0.1 and float((xb != x.double()).double().mean()) >= 0.5
    a1, bits, bits2 = _run_conv1(gpu, x, W1, b1)
    want = R.conv_fwd(xb, W1, b1).clamp_min(0.0)      # one nonzero term per output: exact
    _assert_bits(a1, want, "conv1 delta filter")
    # centre taps, written out: channel 4 = relu(bf16(x[:, 0])), channel 27 + 13 = relu(-bf16(x[:, 1]))
    assert torch.equal(a1[:, 4].double(), xb[:, 0].clamp_min(0.0))
    assert torch.equal(a1[:, 40].double(), (-xb[:, 1]).clamp_min(0.0))
    assert torch.equal(bits, relu_words(want > 0)) and torch.equal(bits2, bits)


def test_relu_bits_edge_values(gpu):
    """slk_wide_relu_bits on +0, -0, the smallest bf16 subnormals, +-1, the largest finite values and the infinities,
    every pattern in every channel: bit c == (a1[c] > 0) exactly."""
    from splitcnn import _lib
    pats = torch.tensor([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x0080, 0x8080])
    g = torch.Generator().manual_seed(8)
    B = 2
    p = pats[torch.randint(0, len(pats), (B, 64, 32, 32), generator=g)]
    for c in range(64):                      # pixel c of sample 0: only channel c positive; sample 1 pixel c: all but c
        p[0, :, c // 32, c % 32], p[0, c, c // 32, c % 32] = 0x8000, 0x0001
        p[1, :, c // 32, c % 32], p[1, c, c // 32, c % 32] = 0x0001, 0x0000
    i16 = torch.where(p >= 0x8000, p - 0x10000, p).to(torch.int16)
    a1 = i16.view(torch.bfloat16)
    want = i16 > 0                           # sign clear and not +0
    assert torch.equal(want, a1.float() > 0)
    a1d = _c8(a1.to(gpu), torch.bfloat16)
    assert torch.equal(_nchw(a1d).view(torch.int16).cpu(), i16)      # the layout change kept every bit
    bits = torch.full((B, 1024), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=gpu)
    _lib.call("slk_wide_relu_bits", a1d.data_ptr(), bits.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    assert torch.equal(bits, relu_words(want.to(gpu)))
    assert bits[0, 5].item() == 1 << 5 and bits[1, 63].item() == (1 << 63) - 1


# ----------------------------------------------------------------------------- weight gradients
def _run_wgrad(dev, layer, inp, d, code):
    """Returns (slabs [nslab, n] f32, slk_reduce_slabs of them [n] f32)."""
    from splitcnn import _lib
    B = inp.shape[0]
    CI, CO, HW = R.LAYERS[layer]
    n = CO * CI * 9 + CO
    nslab = _lib.query(f"slk_wide_conv{layer}_wgrad_nslab", B)
    slabs = torch.full((nslab, n), NAN, device=dev)
    d8 = _c8(d, torch.bfloat16)
    if layer == 1:
        xf = inp.to(torch.float32).contiguous()
        _lib.call("slk_wide_conv1_wgrad", xf.data_ptr(), d8.data_ptr(), slabs.data_ptr(), B, _stream())
    else:
        c8, i8 = _c8(code, torch.uint8), _c8(inp, torch.bfloat16)
        _lib.call(f"slk_wide_conv{layer}_wgrad", d8.data_ptr(), c8.data_ptr(), i8.data_ptr(), slabs.data_ptr(), B, _stream())
    red = torch.full((n,), NAN, device=dev)
    _lib.call("slk_reduce_slabs", slabs.data_ptr(), nslab, n, red.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    assert torch.isfinite(slabs).all(), "a slab was left unwritten"
    return slabs, red


def _ref_wgrad(layer, inp, d, code):
    dy = d if layer == 1 else R.unpool(d, code)
    dW, db = R.conv_wgrad(inp, dy)
    return torch.cat([dW.reshape(-1), db])


@pytest.mark.parametrize("layer,B", [(1, 9), (1, 37), (1, 515), (2, 9), (2, 37), (3, 9), (3, 37)])
def test_wgrad_exact(gpu, layer, B):
    """Operand magnitudes <= 3: the float64 sum of the slabs == the reference exactly, and so does slk_reduce_slabs
    (as f32: every value is an integer below 2^24)."""
    inp, d, code = R.wgrad_case(layer, B, "exact", seed=6000 * layer + B, device=gpu)
    R.assert_exact_operands(inp, d)
    R.assert_abs_bound(_ref_wgrad(layer, inp.abs(), d.abs(), code))
    want = _ref_wgrad(layer, inp, d, code)
    slabs, red = _run_wgrad(gpu, layer, inp, d, code)
    assert torch.equal(slabs.double().sum(0), want)
    assert torch.equal(red.double(), want)
    if layer == 1 and B < 512:
        assert (slabs[B:] == 0).all(), "an idle workgroup's slab is not zero"


@pytest.mark.parametrize("B", [9, 37, 515])
def test_conv1_wgrad_real(gpu, B):
    """slk_wide_conv1_wgrad (bf16(x) operand) vs float64 at the f32 accumulation bar, 1e-5 of the gradient's max."""
    x, d, _ = R.wgrad_case(1, B, "real", seed=7000 + B, device=gpu)
    want = _ref_wgrad(1, R.bf16_f64(x), d, None)
    slabs, red = _run_wgrad(gpu, 1, x, d, None)
    for got in (slabs.double().sum(0), red):
        R.grad_close(_np(got[:1728]), _np(want[:1728]))
        R.grad_close(_np(got[1728:]), _np(want[1728:]))


# ----------------------------------------------------------------------------- shadows
def test_shadows_bit_exact(gpu):
    """slk_wide_shadows / slk_wide_fc_shadow against include/slk.h's index formulas as torch permutations of bf16(W):
    w2f [tap][ci/8][co][8], w2d [8 - tap][co/8][ci][8], w3f [co/128][tap][ci/8][co % 128][8], w3d [8 - tap][co/8][ci][8],
    w1b [64][32] = W1 rows | zeros, wf8[j][(plane * 64 + pix) * 8 + k] = Wf[j][(plane * 8 + k) * 64 + pix]. The weights
    hold exact bf16 halfway values and their neighbours."""
    from splitcnn import _lib
    W1, W2, W3 = (_halfway_f32(s, 90 + i, gpu) for i, s in enumerate(((64, 3, 3, 3), (128, 64, 3, 3), (256, 128, 3, 3))))
    assert R.halfway_share(W3) >= 0.1
    sh = _shadows(gpu, W1, W2, W3)
    b = lambda w: R.bf16(w).view(torch.int16)  # noqa: E731
    w1b = torch.zeros(64, 32, dtype=torch.int16, device=gpu)
    w1b[:, :27] = b(W1).reshape(64, 27)
    assert (sh["w1b"].view(torch.int16).reshape(64, 32)[:, 27:] == 0).all()
    assert torch.equal(sh["w1b"].view(torch.int16).reshape(64, 32), w1b)
    W2b, W3b = b(W2).reshape(128, 64, 9), b(W3).reshape(256, 128, 9)
    want = {
        "w2f": W2b.reshape(128, 8, 8, 9).permute(3, 1, 0, 2),                       # [tap][ci/8][co][ci%8]
        "w2d": W2b.flip(-1).reshape(16, 8, 64, 9).permute(3, 0, 2, 1),              # [8-tap][co/8][ci][co%8]
        "w3f": W3b.reshape(2, 128, 16, 8, 9).permute(0, 4, 2, 1, 3),                # [co/128][tap][ci/8][co%128][ci%8]
        "w3d": W3b.flip(-1).reshape(32, 8, 128, 9).permute(3, 0, 2, 1),
    }
    for k, w in want.items():
        assert torch.equal(sh[k].view(torch.int16), w.reshape(-1)), k
    Wf = _halfway_f32((10, 16384), 99, gpu)
    wf8 = torch.full((10, 16384), NAN, device=gpu)
    _lib.call("slk_wide_fc_shadow", Wf.data_ptr(), wf8.data_ptr(), _stream())
    torch.cuda.synchronize()
    wantf = Wf.reshape(10, 32, 8, 64).permute(0, 1, 3, 2).reshape(10, 16384)
    assert torch.equal(wf8.view(torch.int32), wantf.contiguous().view(torch.int32))
