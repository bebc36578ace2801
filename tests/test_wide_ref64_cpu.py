"""CPU pins of tests/wide_ref64.py (the float64 reference and operand generators of tests/test_wide_conv_gpu.py).

1. Every reference function equals oracle/wide_step.py's (which tests/test_wide_oracle.py pins to torch autograd) on
   CPU tensors at B = 2: exactly on integer inputs, to 1e-12 relative on real-valued ones.
2. The exact-regime generators meet their preconditions and DISCRIMINATE: exact ties, zero maxima, every first-max
   position and bf16 halfway cases each make up at least 1 % of what the exact GPU tests compare, so a kernel that
   resolved ties to the last maximum, blocked at `m >= 0` / `m < 0`, or truncated instead of rounding to nearest even
   would fail them. The floors are 1 %; the shares measured with these generators are printed and stated below.
3. The real-valued generators leave the project's bf16 bar its margin: an independent f32 reference (torch f32 conv
   on the same operands) against float64 flips the bf16 rounding of at most 3e-4 of the elements (a third of
   bf16_close's 1e-3 cap; measured 1e-5 to 8.4e-5).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wide_ref64 as R
from oracle import wide_step as W


def _same(got, want, exact):
    got, want = got.double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if exact:
        assert np.array_equal(got, want)
    else:
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("regime", ["wide", "narrow", "real"])
def test_conv_functions_equal_the_oracle(layer, regime):
    exact = regime != "real"
    x, Wt, b = R.fwd_case(layer, 2, regime, seed=100 + layer)
    _same(R.conv_fwd(x, Wt, b, chunk=1), W.conv3x3p1(x.numpy(), Wt.numpy(), b.numpy()), exact)
    _same(R.conv_fwd(x, Wt), W.conv3x3p1(x.numpy(), Wt.numpy()), exact)
    CI, CO, HW = R.LAYERS[layer]
    g = torch.Generator().manual_seed(7 + layer)
    dy = torch.randint(-15, 16, (2, CO, HW, HW), generator=g).double() if exact else \
        torch.randn(2, CO, HW, HW, generator=g).double()
    _same(R.conv_dgrad(dy, Wt, chunk=1), W.conv3x3p1_dgrad(dy.numpy(), Wt.numpy()), exact)
    dW, db = R.conv_wgrad(x, dy, chunk=1)
    dWo, dbo = W.conv3x3p1_wgrad(x.numpy(), dy.numpy())
    _same(dW, dWo, exact)
    _same(db, dbo, exact)


@pytest.mark.parametrize("regime", ["wide", "narrow", "real"])
def test_pool_unpool_bf16_equal_the_oracle(regime):
    x, Wt, b = R.fwd_case(2, 2, regime, seed=5)
    c = R.conv_fwd(x, Wt, b)
    pooled, code = R.relu_pool_code(c)
    po, co = W.relu_pool_code(c.numpy())
    assert np.array_equal(pooled.numpy(), po) and np.array_equal(code.numpy(), co)
    assert not torch.signbit(pooled).any()                      # +0 where blocked
    assert torch.equal(R.pooled_at(c, code), pooled)
    g = torch.Generator().manual_seed(1)
    rc = R.codes(g, tuple(code.shape))
    dp = torch.randn(tuple(code.shape), generator=g).double()
    assert np.array_equal(R.unpool(dp, rc).numpy(), W.unpool(dp.numpy(), rc.numpy()))
    assert np.array_equal(R.bf16_f64(c).numpy(), W.bf16(c.numpy()).astype(np.float64))
    # ties to even at exact halfway values, both neighbours: 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6
    h = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 257.0, 259.0], dtype=torch.float64)
    assert R.bf16_f64(h).tolist() == [1.0, 1 + 2.0 ** -6, -1.0, 256.0, 260.0]
    assert np.array_equal(R.bf16_f64(h).numpy(), W.bf16(h.numpy()).astype(np.float64))


def test_pos_zero_and_halfway_share():
    z = torch.tensor([-0.0, 0.0, -1.0])
    assert not torch.signbit(R.pos_zero(z)[:2]).any() and R.pos_zero(z)[2] == -1
    assert R.halfway_share(torch.tensor([257.0, 256.0, 258.0, 259.0])) == 0.5


@pytest.mark.parametrize("layer", [2, 3])
def test_narrow_generator_produces_ties_zero_maxima_and_every_position(layer, capsys):
    """Shares among the pooling windows of conv<layer> at B = 2 (floor 1 % each). Measured: positive maxima attained
    more than once 3.7 % / 2.9 % (conv2 / conv3), maxima of exactly 0 2.4 % / 1.5 %, first-max positions 24-26 % each."""
    x, Wt, b = R.fwd_case(layer, 2, "narrow", seed=31 + layer)
    R.assert_exact_operands(x, Wt, b)
    R.assert_abs_bound(R.conv_fwd(x.abs(), Wt.abs(), b.abs()))
    c = R.conv_fwd(x, Wt, b)
    win = R.windows(c)
    m = win.max(-1).values
    pooled, code = R.relu_pool_code(c)
    tie = ((win == m[..., None]).sum(-1) > 1) & (m > 0)
    zero = m == 0
    shares = {"tie": float(tie.double().mean()), "zero max": float(zero.double().mean())}
    npos = float((m > 0).sum())
    for q in range(4):
        shares[f"first max at {q}"] = float((code == q).sum()) / npos
    with capsys.disabled():
        print(f"\nconv{layer} narrow: " + ", ".join(f"{k} {v:.3%}" for k, v in shares.items()))
    for k, v in shares.items():
        assert v >= 0.01, (k, v)
    # where a tie occurs, first-max and last-max routing differ (what the exact GPU test then tells apart)
    last = 3 - (win.flip(-1) == m[..., None]).long().argmax(-1)
    assert float(((last != code) & (m > 0)).double().mean()) >= 0.01


def test_wide_generator_produces_bf16_halfway_cases(capsys):
    """Exact halfway cases of the bf16 store (low 16 bits of the f32 value 0x8000) at B = 2, floor 1 %. Measured:
    pooled conv2 forward 14.8 %, conv3 dgrad 21.9 %. Round-to-nearest-even and truncation differ on all of those that
    round up, and round-half-away differs on those that round down."""
    x, Wt, b = R.fwd_case(2, 2, "wide", seed=41)
    R.assert_exact_operands(x, Wt, b)
    R.assert_abs_bound(R.conv_fwd(x.abs(), Wt.abs(), b.abs()))
    pooled, _ = R.relu_pool_code(R.conv_fwd(x, Wt, b))
    dp, code, W3, _ = R.dgrad_case(3, 2, "wide", seed=42)
    R.assert_exact_operands(dp, W3)
    R.assert_abs_bound(R.conv_dgrad(R.unpool(dp, code).abs(), W3.abs()))
    d = R.conv_dgrad(R.unpool(dp, code), W3)
    s2, s3 = R.halfway_share(pooled), R.halfway_share(d)
    with capsys.disabled():
        print(f"\nwide: bf16 halfway cases, pooled conv2 forward {s2:.3%}, conv3 dgrad {s3:.3%}")
    assert s2 >= 0.01 and s3 >= 0.01
    for v in (pooled, d):   # and nearest-even differs from truncation on at least 1 % of the stored values
        trunc = (v.float().view(torch.int32) & ~0xFFFF).view(torch.float32).double()
        assert float((trunc != R.bf16_f64(v)).double().mean()) >= 0.01


def test_wgrad_generator_stays_exact_at_the_largest_batch():
    """The weight-gradient operands have magnitudes <= 3: the absolute-value sum over a whole batch of 515 is at most
    515 x 1024 x 9 = 4.7 M < 2^24 whatever the draw (the GPU tests assert the bound on their own operands)."""
    for layer in (1, 2, 3):
        inp, d, code = R.wgrad_case(layer, 2, "exact", seed=3)
        R.assert_exact_operands(inp, d)
        assert inp.abs().max() <= 3 and d.abs().max() <= 3
    assert 515 * 1024 * 9 < 2 ** 24


@pytest.mark.parametrize("layer", [1, 2, 3])
def test_real_generator_leaves_the_bf16_bar_its_margin(layer, capsys):
    """bf16_close lets 1e-3 of the elements differ by one bf16 ulp. An independent f32 evaluation of the same math
    (torch's f32 conv on the CPU, B = 8) against float64 flips far fewer bf16 roundings with these distributions
    (measured 3.2e-5 to 8.4e-5 over conv2 / conv3 forward and dgrad, 1e-5 for conv1); the ceiling is 3e-4, a third of
    the cap. If a changed generator moves an f32 reference alone towards the bar, this says so."""
    B = 8
    x, Wt, b = R.fwd_case(layer, B, "real", seed=51 + layer)
    xb, Wb = R.bf16_f64(x), R.bf16_f64(Wt)
    c64 = R.conv_fwd(xb, Wb, b)
    c32 = F.conv2d(xb.float(), Wb.float(), b.float(), padding=1)
    cases = {"forward": (torch.relu(c64), torch.relu(c32))}
    if layer > 1:   # the dgrad of this layer: routed pooled gradient x the same weights
        dp, code, Wd, _ = R.dgrad_case(layer, B, "real", seed=61 + layer)
        dc = R.unpool(dp, code)
        Wdb = R.bf16_f64(Wd)
        d32 = F.conv_transpose2d(dc.float(), Wdb.float(), padding=1)
        cases["dgrad"] = (R.conv_dgrad(dc, Wdb), d32)
    for name, (v64, v32) in cases.items():
        flips = float((R.bf16(v64) != R.bf16(v32)).double().mean())
        with capsys.disabled():
            print(f"\nconv{layer} {name}: f32 vs float64 flips {flips:.2e} of the bf16 roundings")
        assert flips <= 3e-4, (name, flips)
        R.bf16_close(R.bf16_f64(v32).numpy(), R.bf16_f64(v64).numpy())
