"""The K2 client kernels (csrc/slk_client.hip) and the K2 fc kernels (csrc/slk_server.hip: fc_head16_kernel's logits
and dgrad stages, fc_wgrad_kernel) called ALONE through their entry points against the float64 references of
tests/head_ref64.py, bit for bit on integer operands (every partial sum below 2^24: head_ref64's generators state the
bounds, each test asserts them on the reference side).

Every output is pre-filled with NaN and allocated with one extra sample (or slab) of sentinel after its last row: a
skipped element fails the bitwise comparison, a write past a ragged batch fails assert_sentinel.

Batch sizes, from the code:
  conv1 forward   one workgroup per sample, 169 of 192 threads own 4 consecutive pixels (a group may straddle two
                  rows): B = 1, 5, 2053.
  conv1 wgrad     grid min(B, 128) sample ranges [grp * B / G, (grp + 1) * B / G) x 8 channel groups; items = sample x
                  338 pixel pairs over 256 threads: B = 1 (338 items: a ragged second round), 5, 127, 128 (one sample
                  per range), 129 and 300 (ranges of unequal length: 1-2 and 2-3 samples).
  fc fwd / dgrad  16 samples per workgroup, wave w owns features 1152 w .. in 64-feature chunks: B = 1, 15, 16, 17, 33.
  fc wgrad        slices of per = ceil(B / min(64, ceil(B / 64))) samples, 8 unrolled + a tail: B = 1, 7, 8, 9, 64,
                  65 (33 + 32), 130 (44 + 44 + 42).
Each exact test ends by mutating the REFERENCE (`>=` mask, dropped last pixel pair, one tap shifted, last sample of a
range dropped, class index transposed) and asserting that the kernel's result differs from it: the test would notice
that bug in the kernel.
"""
import pytest
import torch

import head_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
FC_BATCHES = [1, 15, 16, 17, 33]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t):
    return t.to(torch.float32).contiguous()


def _nan(shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


# ----------------------------------------------------------------------------- conv1 forward
def _run_conv1(dev, x, W1, b1, amax):
    from splitcnn import _lib
    B = x.shape[0]
    xf, wf, bf = _f32(x), _f32(W1), _f32(b1)
    act = _nan((B + 1, 32, 26, 26), dev)
    am = _nan((B + 1,), dev)
    if amax:
        _lib.call("slk_conv1_fwd_amax", xf.data_ptr(), wf.data_ptr(), bf.data_ptr(), act.data_ptr(), am.data_ptr(), B,
                  _stream())
    else:
        _lib.call("slk_conv1_fwd", xf.data_ptr(), wf.data_ptr(), bf.data_ptr(), act.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(act, B * 32 * 676, "conv1 act")
    R.assert_sentinel(am, B if amax else 0, "conv1 act_amax")
    return act[:B], am[:B]


@pytest.mark.parametrize("B", [1, 5, 2053])
def test_conv1_fwd_exact(gpu, B):
    """act == relu(conv1(x)) of float64 bit for bit (+0.0, never -0.0, at every blocked pixel; 2.6 % of the
    pre-activations are exactly 0), from both entry points; act_amax == include/slk.h's expression in f32."""
    x, W1, b1 = R.conv1_int_case(B, 100 + B, gpu)
    assert float(R.conv1_abs_bound(x, W1, b1).max()) < 2 ** 24
    pre = R.conv1_pre(x, W1, b1)
    assert float((pre == 0).double().mean()) >= 0.01
    want = torch.where(pre > 0, pre, torch.zeros_like(pre))
    act, _ = _run_conv1(gpu, x, W1, b1, amax=False)
    R.assert_bits_f32(act, want, f"slk_conv1_fwd B={B}")
    act2, am = _run_conv1(gpu, x, W1, b1, amax=True)
    R.assert_bits_f32(act2, want, f"slk_conv1_fwd_amax B={B}")
    assert torch.equal(R.f32_bits(am), R.f32_bits(R.conv1_cut_bound_f32(x, W1, b1))), "act_amax"
    assert (am.double() >= want.reshape(B, -1).max(dim=1).values).all()
    # mutated references: a `>=`-style ReLU cannot show in the forward (relu(0) = 0 either way), a shifted tap does
    Wm = W1.clone().reshape(32, 9)
    Wm[:, [4, 5]] = Wm[:, [5, 4]]
    assert not torch.equal(act.double(), R.conv1_relu(x, Wm.reshape(32, 1, 3, 3), b1)), "tap 4 <-> 5 not noticed"


@pytest.mark.parametrize("B", [1, 5])
def test_conv1_fwd_real(gpu, B):
    """Real-valued operands against float64, elementwise: the kernel's stated order is a 9-step fma chain from 0 and
    one add of the bias, ten roundings of partial sums bounded by S = sum_k |x_k W_k| + |b|, so
    |act - act64| <= 10 * 2^-24 * S (relu is 1-Lipschitz)."""
    x, W1, b1 = R.conv1_real_case(B, 200 + B, gpu)
    want = R.conv1_relu(x, W1, b1)
    bound = 10 * 2.0 ** -24 * R.conv1_abs_bound(x, W1, b1)
    act, _ = _run_conv1(gpu, x, W1, b1, amax=False)
    assert not torch.isnan(act).any()
    ratio = ((act.double() - want).abs() / bound).max().item()
    print(f"conv1 real B={B}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ----------------------------------------------------------------------------- conv1 weight gradient
def _run_c1w(dev, x, act, W1, b1, g, remask):
    from splitcnn import _lib
    B = x.shape[0]
    nslab = _lib.query("slk_conv1_wgrad_nslab", B)
    assert nslab == min(B, 128)
    xf, gf = _f32(x), _f32(g)
    slabs = _nan((nslab + 1, 320), dev)
    if remask:
        wf, bf = _f32(W1), _f32(b1)
        _lib.call("slk_conv1_wgrad_remask", xf.data_ptr(), wf.data_ptr(), bf.data_ptr(), gf.data_ptr(), slabs.data_ptr(), B,
                  _stream())
    else:
        af = _f32(act)
        _lib.call("slk_conv1_wgrad", xf.data_ptr(), af.data_ptr(), gf.data_ptr(), slabs.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(slabs, nslab * 320, "conv1 wgrad slabs")
    return slabs[:nslab]


@pytest.mark.parametrize("B", [1, 5, 127, 128, 129, 300])
def test_conv1_wgrad_exact(gpu, B):
    """Every slab of slk_conv1_wgrad and slk_conv1_wgrad_remask == the float64 sum over its own sample range, bit for
    bit, with act from the integer forward (exact zeros in the mask); the slabs' sum == the full gradient; the two
    entry points write identical slabs; and a cut gradient that is nonzero exactly where the pre-activation is 0 gives
    an exactly zero gradient."""
    x, W1, b1 = R.conv1_int_case(B, 300 + B, gpu)
    g = R.cut_grad_int(B, 400 + B, gpu)
    pre = R.conv1_pre(x, W1, b1)
    act = torch.where(pre > 0, pre, torch.zeros_like(pre))
    assert float((pre == 0).double().mean()) >= 0.01
    worst = R.conv1_wgrad_slabs(x.abs(), torch.ones_like(act), g.abs())
    assert float(worst.max()) < 2 ** 24
    want = R.conv1_wgrad_slabs(x, act, g)
    got = {rm: _run_c1w(gpu, x, act, W1, b1, g, rm) for rm in (False, True)}
    for rm, s in got.items():
        what = f"slk_conv1_wgrad{'_remask' if rm else ''} B={B}"
        R.assert_bits_f32(s, want, what)
        assert torch.equal(s.double().sum(0), R.conv1_wgrad_per_sample(x, act, g).sum(0)), what
    assert torch.equal(R.f32_bits(got[False]), R.f32_bits(got[True]))
    # gradient only on the ReLU boundary: nothing may pass
    gen = torch.Generator().manual_seed(B)
    gz = torch.where(pre == 0, (torch.randint(1, 5, pre.shape, generator=gen) * 2.0 - 5.0).to(gpu).double(),
                     torch.zeros_like(pre))
    assert (gz != 0).any()
    for rm in (False, True):
        assert (R.f32_bits(_run_c1w(gpu, x, act, W1, b1, gz, rm)) == 0).all(), "a gradient passed the mask at act == 0"
    # mutated references must NOT match the kernel
    muts = ["ge", "drop_last_pair", "shift_tap"] + (["drop_last_sample"] if B > 128 else [])
    for m in muts:
        assert not torch.equal(got[False].double(), R.conv1_wgrad_slabs(x, act, g, mutate=m)), f"mutation {m} not noticed"
    assert not torch.equal(_run_c1w(gpu, x, act, W1, b1, gz, True).double(), R.conv1_wgrad_slabs(x, act, gz, mutate="ge"))


# ----------------------------------------------------------------------------- fc forward
def _run_fc_fwd(dev, pooled, W3, b3):
    from splitcnn import _lib
    B = pooled.shape[0]
    pf, wf, bf = _f32(pooled), _f32(W3), _f32(b3)
    logits = _nan((B + 1, 10), dev)
    _lib.call("slk_fc_fwd", pf.data_ptr(), wf.data_ptr(), bf.data_ptr(), logits.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(logits, B * 10, "fc logits")
    return logits[:B]


@pytest.mark.parametrize("B", FC_BATCHES)
def test_fc_fwd_exact(gpu, B):
    pooled, W3, b3 = R.fc_int_case(B, 500 + B, gpu)
    assert float(R.fc_fwd(pooled, W3.abs(), b3.abs()).max()) < 2 ** 24
    R.assert_bits_f32(_run_fc_fwd(gpu, pooled, W3, b3), R.fc_fwd(pooled, W3, b3), f"slk_fc_fwd B={B}")


@pytest.mark.parametrize("B", FC_BATCHES)
def test_fc_fwd_onehot(gpu, B):
    """pooled[s] = a single 1.0 at feature k_s (first / last feature of several waves and chunks, features 0 and 9215),
    b3 = 0: logits[s] == W3[:, k_s] bit for bit for arbitrary finite W3 (every other product is 0 * finite = +-0)."""
    gen = torch.Generator().manual_seed(600 + B)
    W3 = (torch.randn((10, R.P_SAMPLE), generator=gen) * 10.0 ** (torch.rand((10, R.P_SAMPLE), generator=gen) * 12 - 6))
    W3 = W3.float().to(gpu)
    ks = R.onehot_features(B)
    pooled = R.onehot_rows(B, R.P_SAMPLE, ks, gpu)
    logits = _run_fc_fwd(gpu, pooled, W3, torch.zeros(10, device=gpu))
    want = W3[:, torch.tensor(ks, device=gpu)].T.contiguous()
    assert torch.equal(R.f32_bits(logits), R.f32_bits(want))


# ----------------------------------------------------------------------------- fc dgrad
@pytest.mark.parametrize("B", FC_BATCHES)
def test_fc_dgrad_exact(gpu, B):
    from splitcnn import _lib
    _, W3, _ = R.fc_int_case(1, 700 + B, gpu)
    dl = R.dlogits_int(B, 710 + B, gpu)
    want = R.fc_dgrad(dl, W3)
    assert float(R.fc_dgrad(dl.abs(), W3.abs()).max()) < 2 ** 24
    dlf, wf = _f32(dl), _f32(W3)
    for amax in (False, True):
        dp = _nan((B + 1, R.P_SAMPLE), gpu)
        am = _nan((B + 1,), gpu)
        if amax:
            _lib.call("slk_fc_dgrad_amax", dlf.data_ptr(), wf.data_ptr(), dp.data_ptr(), am.data_ptr(), B, _stream())
        else:
            _lib.call("slk_fc_dgrad", dlf.data_ptr(), wf.data_ptr(), dp.data_ptr(), B, _stream())
        torch.cuda.synchronize()
        R.assert_sentinel(dp, B * R.P_SAMPLE, "dpooled")
        R.assert_sentinel(am, B if amax else 0, "dp_amax")
        R.assert_bits_f32(dp[:B], want, f"slk_fc_dgrad{'_amax' if amax else ''} B={B}")
        if amax:
            assert torch.equal(am[:B].double(), want.abs().max(dim=1).values)
    # a transposed class index in the reference is noticed
    assert not torch.equal(dp[:B].double(), R.fc_dgrad(dl.roll(1, dims=1), W3))


# ----------------------------------------------------------------------------- fc weight gradient
@pytest.mark.parametrize("B", [1, 7, 8, 9, 64, 65, 130])
def test_fc_wgrad_exact(gpu, B):
    """Each slab == float64's sum over its slice of fc_wgrad_per(B) samples bit for bit, db3 included;
    slk_fc_wgrad_nslab matches the formula."""
    from splitcnn import _lib
    pooled, _, _ = R.fc_int_case(B, 800 + B, gpu)
    dl = R.dlogits_int(B, 810 + B, gpu)
    nslab = _lib.query("slk_fc_wgrad_nslab", B)
    assert nslab == R.fc_wgrad_nslab(B)
    assert float(R.fc_wgrad_slabs(dl.abs(), pooled).max()) < 2 ** 24
    slabs = _nan((nslab + 1, 92170), gpu)
    dlf, pf = _f32(dl), _f32(pooled)
    _lib.call("slk_fc_wgrad", dlf.data_ptr(), pf.data_ptr(), slabs.data_ptr(), B, _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(slabs, nslab * 92170, "fc wgrad slabs")
    want = R.fc_wgrad_slabs(dl, pooled)
    R.assert_bits_f32(slabs[:nslab], want, f"slk_fc_wgrad B={B}")
    assert torch.equal(slabs[:nslab, 92160:].double().sum(0), dl.sum(0))
    for m in ["transpose_class"] + (["drop_last_sample"] if B > 1 else []):
        assert not torch.equal(slabs[:nslab].double(), R.fc_wgrad_slabs(dl, pooled, mutate=m)), f"mutation {m} not noticed"


@pytest.mark.parametrize("B,n", [(1, 1), (64, 1), (65, 2), (130, 3), (4096, 64), (4097, 64), (100000, 64)])
def test_fc_wgrad_nslab_formula(gpu, B, n):
    from splitcnn import _lib
    assert _lib.query("slk_fc_wgrad_nslab", B) == n == R.fc_wgrad_nslab(B)
