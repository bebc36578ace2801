"""Every copy of the cross-entropy on extreme logits. The copies: fc_head16_kernel MODE 2 (slk_xent_fwd_bwd and the
fused slk_fc_logits_xent / slk_fc_xent / slk_fc_xent_amax), slk_eval_row (slk_fc_eval, slk_eval_logits) and
wide_head16_kernel<true> (slk_wide_head). All compute m + logf(se) after a max-subtraction; a copy without the
subtraction, or one that takes the wrong z[y], fails here (tests/test_head_ref64_cpu.py shows that on the CPU).

Rows (head_ref64.xent_rows), each with the label at its maximum, its minimum and in between: all equal (0 and 1e4),
100 .. 91 and -100 .. -109 (exp overflow / underflow without the subtraction), one logit 30 and one 200 above the rest,
magnitude 1e4 with unit gaps, +-1e30 mixed (label on the positive and on a negative class) and, for the two entry
points that take logits, rows with -inf off the label.

The fused heads see exactly these logits by a one-hot construction: sample s holds a single 1.0 at its own feature,
the row sits in that column of the weight and the bias is 0 (asserted: the stored logits equal the rows bit for bit).
B = 17 and 33 put rows into the first and last slot of a 16-sample workgroup and into a ragged last workgroup.

Bounds against float64 (head_ref64.loss_bound / grad_bound, grad_scale = 1):
  |loss - loss64| <= 2^-23 (max|z| + ln 10) + (2e-6 |loss64| + 1e-6)
  |dlogits - d64| <= p64 2^-22 (max|z| + ln 10) + 2e-7
  every output finite on every finite row
  |sum_j dlogits_j| <= 2^-22 (max|z| + ln 10) + 10 * 2^-23          (head_ref64.gradsum_bound)
The last bound carries a term that a flat 10 * 2^-23 lacks. Derivation: all ten p_j = exp(z_j - lse) of a row share
the rounding of lse = fl(m + log se), an absolute error of the exponent up to 2^-24 (max|z| + ln 10); it scales the
whole row by exp(error), so the row's sum misses 1 by that much — the per-element bound's relative term summed over
the row (sum_j p64_j = 1). At max|z| = 1e4 (ulp(lse) = 2^-10) the kernels' rows sum to 1 +- 3e-4, inside the
per-element bound and inside this one, far outside 10 * 2^-23 = 1.2e-6; torch's log_softmax keeps (z - m) - log(se)
and does not lose those bits, so the kernels' expression is the less accurate one at such logits.
The largest observed ratio to each bound is printed per entry point.
"""
import numpy as np
import pytest
import torch

import head_ref64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = [(17, 0), (17, 11), (33, 0), (33, 11)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _batch(B, shift, dev, finite_only=True):
    names, z, y = R.xent_batch(B, shift, finite_only)
    return names, z, y, torch.from_numpy(z).float().to(dev).contiguous(), torch.from_numpy(y).to(dev)


def _check(what, names, z, y, loss, dlogits):
    """loss [B], dlogits [B,10] (numpy float32) against float64 at the module docstring's bounds."""
    loss64, d64, p64 = R.xent64(z, y)
    loss, dl = loss.astype(np.float64), dlogits.astype(np.float64) if dlogits is not None else None
    assert np.isfinite(loss).all(), f"{what}: non-finite loss at {[n for n, v in zip(names, loss) if not np.isfinite(v)]}"
    rl = np.abs(loss - loss64) / R.loss_bound(z, loss64)
    msg = f"{what}: loss {rl.max():.3f} of its bound ({names[int(rl.argmax())]})"
    assert rl.max() <= 1.0, msg
    if dl is not None:
        assert np.isfinite(dl).all(), f"{what}: non-finite dlogits"
        rg = np.abs(dl - d64) / R.grad_bound(z, p64)
        rs = np.abs(dl.sum(axis=1)) / R.gradsum_bound(z)
        msg += (f", dlogits {rg.max():.3f} ({names[int(rg.max(axis=1).argmax())]}), row sum {rs.max():.3f} "
                f"({names[int(rs.argmax())]}); largest |row sum| {np.abs(dl.sum(axis=1)).max():.3e}")
        assert rg.max() <= 1.0, msg
        assert rs.max() <= 1.0, msg
    print(msg)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the entry points that take logits
def _xent_direct(dev, zt, yt):
    from splitcnn import _lib
    B = zt.shape[0]
    loss, dl = _nan((B + 1,), dev), _nan((B + 1, 10), dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("slk_xent_fwd_bwd", zt.data_ptr(), yt.data_ptr(), loss.data_ptr(), dl.data_ptr(), 1.0, err.data_ptr(), B,
              _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(loss, B, "loss_i")
    R.assert_sentinel(dl, B * 10, "dlogits")
    assert int(err) == 0
    return loss[:B], dl[:B]


def _eval_logits(dev, zt, yt):
    from splitcnn import _lib
    B = zt.shape[0]
    loss = _nan((B + 1,), dev)
    pred = torch.full((B + 1,), -1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("slk_eval_logits", zt.data_ptr(), yt.data_ptr(), B, loss.data_ptr(), pred.data_ptr(), err.data_ptr(), _stream())
    torch.cuda.synchronize()
    R.assert_sentinel(loss, B, "eval loss_i")
    R.assert_sentinel(pred, B, "eval pred")
    assert int(err) == 0
    return loss[:B], pred[:B]


@pytest.mark.parametrize("B,shift", CASES)
def test_xent_entry_points_on_crafted_rows(gpu, B, shift):
    """slk_xent_fwd_bwd and slk_eval_logits on every row, the -inf rows included; the evaluation loss equals the
    training loss bit for bit and pred is the first maximum."""
    names, z, y, zt, yt = _batch(B, shift, gpu, finite_only=False)
    loss, dl = _xent_direct(gpu, zt, yt)
    _check(f"slk_xent_fwd_bwd B={B}", names, z, y, loss.cpu().numpy(), dl.cpu().numpy())
    eloss, pred = _eval_logits(gpu, zt, yt)
    _check(f"slk_eval_logits B={B}", names, z, y, eloss.cpu().numpy(), None)
    assert torch.equal(_bits(eloss), _bits(loss))
    assert np.array_equal(pred.cpu().numpy(), z.argmax(axis=1))
    assert (dl.cpu().numpy()[~np.isfinite(z)] == 0).all(), "a -inf class got a gradient"


# ----------------------------------------------------------------------------- the K2 fused heads
def _k2_operands(dev, z, B):
    ks = R.onehot_features(B)
    W3 = torch.zeros((10, R.P_SAMPLE), dtype=torch.float32, device=dev)
    W3[:, torch.tensor(ks, device=dev)] = torch.from_numpy(z).float().to(dev).T
    pooled = R.onehot_rows(B, R.P_SAMPLE, ks, dev).float().contiguous()
    return pooled, W3.contiguous(), torch.zeros(10, dtype=torch.float32, device=dev)


@pytest.mark.parametrize("B,shift", CASES)
def test_k2_fused_heads_on_crafted_rows(gpu, B, shift):
    """slk_fc_logits_xent, slk_fc_xent, slk_fc_xent_amax and slk_fc_eval see exactly the crafted logits; each meets the
    float64 bounds; and, bit for bit, the fused heads == slk_fc_fwd -> slk_xent_fwd_bwd (-> slk_fc_dgrad_amax), and
    slk_fc_eval's and slk_eval_logits' loss_i == the training head's."""
    from splitcnn import _lib
    names, z, y, zt, yt = _batch(B, shift, gpu)
    pooled, W3, b3 = _k2_operands(gpu, z, B)
    s = _stream()

    def outs():
        return dict(logits=_nan((B + 1, 10), gpu), loss=_nan((B + 1,), gpu), dl=_nan((B + 1, 10), gpu),
                    dp=_nan((B + 1, R.P_SAMPLE), gpu), am=_nan((B + 1,), gpu),
                    err=torch.zeros(1, dtype=torch.int32, device=gpu))

    # the separate kernels
    sep = outs()
    _lib.call("slk_fc_fwd", pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), sep["logits"].data_ptr(), B, s)
    torch.cuda.synchronize()
    assert torch.equal(_bits(sep["logits"][:B]), _bits(zt)), "the one-hot construction did not reproduce the rows"
    sep["loss"][:B], sep["dl"][:B] = _xent_direct(gpu, sep["logits"][:B].contiguous(), yt)
    _lib.call("slk_fc_dgrad_amax", sep["dl"].data_ptr(), W3.data_ptr(), sep["dp"].data_ptr(), sep["am"].data_ptr(), B, s)
    torch.cuda.synchronize()

    runs = {}
    o = outs()
    _lib.call("slk_fc_logits_xent", pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), o["logits"].data_ptr(),
              o["loss"].data_ptr(), o["dl"].data_ptr(), 1.0, o["err"].data_ptr(), B, s)
    runs["slk_fc_logits_xent"] = o
    o = outs()
    _lib.call("slk_fc_xent", pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), o["logits"].data_ptr(),
              o["loss"].data_ptr(), o["dl"].data_ptr(), o["dp"].data_ptr(), 1.0, o["err"].data_ptr(), B, s)
    runs["slk_fc_xent"] = o
    o = outs()
    _lib.call("slk_fc_xent_amax", pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), o["logits"].data_ptr(),
              o["loss"].data_ptr(), o["dl"].data_ptr(), o["dp"].data_ptr(), o["am"].data_ptr(), 1.0, o["err"].data_ptr(),
              B, s)
    runs["slk_fc_xent_amax"] = o
    torch.cuda.synchronize()
    for name, o in runs.items():
        assert int(o["err"]) == 0
        for k, used in (("logits", B * 10), ("loss", B), ("dl", B * 10)):
            R.assert_sentinel(o[k], used, f"{name} {k}")
            assert torch.equal(_bits(o[k][:B]), _bits(sep[k][:B])), f"{name}: {k} differs from the separate kernels"
        _check(f"{name} B={B}", names, z, y, o["loss"][:B].cpu().numpy(), o["dl"][:B].cpu().numpy())
        has_dp, has_am = name != "slk_fc_logits_xent", name == "slk_fc_xent_amax"
        R.assert_sentinel(o["dp"], B * R.P_SAMPLE if has_dp else 0, f"{name} dpooled")
        R.assert_sentinel(o["am"], B if has_am else 0, f"{name} dp_amax")
        if has_dp:
            assert torch.isfinite(o["dp"][:B]).all()
            assert torch.equal(_bits(o["dp"][:B]), _bits(sep["dp"][:B])), f"{name}: dpooled differs from slk_fc_dgrad"
        if has_am:
            assert torch.equal(_bits(o["am"][:B]), _bits(sep["am"][:B]))
            assert torch.equal(o["am"][:B], o["dp"][:B].abs().max(dim=1).values)

    # evaluation copies
    e = outs()
    pred = torch.full((B + 1,), -1, dtype=torch.int64, device=gpu)
    _lib.call("slk_fc_eval", pooled.data_ptr(), W3.data_ptr(), b3.data_ptr(), yt.data_ptr(), e["logits"].data_ptr(),
              e["loss"].data_ptr(), pred.data_ptr(), e["err"].data_ptr(), B, s)
    torch.cuda.synchronize()
    R.assert_sentinel(e["logits"], B * 10, "slk_fc_eval logits")
    R.assert_sentinel(e["loss"], B, "slk_fc_eval loss_i")
    R.assert_sentinel(pred, B, "slk_fc_eval pred")
    _check(f"slk_fc_eval B={B}", names, z, y, e["loss"][:B].cpu().numpy(), None)
    assert torch.equal(_bits(e["logits"][:B]), _bits(zt)) and int(e["err"]) == 0
    assert torch.equal(_bits(e["loss"][:B]), _bits(sep["loss"][:B])), "slk_fc_eval loss_i != the training head's"
    assert np.array_equal(pred[:B].cpu().numpy(), z.argmax(axis=1))
    eloss, epred = _eval_logits(gpu, zt, yt)
    assert torch.equal(_bits(eloss), _bits(sep["loss"][:B])), "slk_eval_logits loss_i != the training head's"
    assert torch.equal(epred, pred[:B])


# ----------------------------------------------------------------------------- the K5 head
def _wide_positions(B):
    """Distinct C8 positions (chunk * 8 + k) of the one-hot cut: the first and last feature of the cut and of waves
    1, 3, 7 (wave w owns chunks 256 w ..), then fillers across every wave."""
    ps = [0, R.CUT_F - 1]
    for w in (1, 3, 7):
        ps += [2048 * w, 2048 * w + 2047]
    ps = list(dict.fromkeys(ps))
    ps += [p for p in range(37, R.CUT_F, 487) if p not in ps]
    assert B <= len(ps)
    return ps[:B]


@pytest.mark.parametrize("B,shift", CASES)
def test_wide_head_on_crafted_rows(gpu, B, shift):
    """slk_wide_head with keep_threshold 0, keep_scale 1 (the evaluation path's setting) on a one-hot bf16 cut with the
    rows in columns of Wf: its logits are the rows bit for bit, its loss and dlogits meet the float64 bounds, and every
    output (dcut, the weight-gradient slabs) is finite."""
    from splitcnn import _lib
    names, z, y, zt, yt = _batch(B, shift, gpu)
    s = _stream()
    ps = torch.tensor(_wide_positions(B), device=gpu)
    cut8 = torch.zeros((B, R.CUT_F), dtype=torch.float64, device=gpu)
    cut8[torch.arange(B, device=gpu), ps] = 1.0
    feat = R.flat_of_c8(cut8).argmax(dim=1)                     # the flatten-order feature of each sample's one
    Wf = torch.zeros((10, R.CUT_F), dtype=torch.float32, device=gpu)
    Wf[:, feat] = zt.T
    wf8 = _nan((10, R.CUT_F), gpu)
    _lib.call("slk_wide_fc_shadow", Wf.data_ptr(), wf8.data_ptr(), s)
    cut = cut8.to(torch.bfloat16).contiguous()
    bf = torch.zeros(10, dtype=torch.float32, device=gpu)
    step = torch.full((1,), 3, dtype=torch.int32, device=gpu)
    nslab = _lib.query("slk_wide_head_nslab", B)
    nwork = _lib.query("slk_wide_head_work", B)
    logits, loss, dl = _nan((B + 1, 10), gpu), _nan((B + 1,), gpu), _nan((B + 1, 10), gpu)
    dcut = torch.full((B + 1, R.CUT_F), NAN, dtype=torch.bfloat16, device=gpu)
    slabs = _nan((nslab + 1, 163850), gpu)
    work = _nan((nwork + 512,), gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    _lib.call("slk_wide_head", cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), yt.data_ptr(), step.data_ptr(), 7, 0, 1.0, 1.0,
              logits.data_ptr(), loss.data_ptr(), dl.data_ptr(), dcut.data_ptr(), slabs.data_ptr(), work.data_ptr(),
              err.data_ptr(), 0, B, s)
    torch.cuda.synchronize()
    for t, used, what in ((logits, B * 10, "logits"), (loss, B, "loss_i"), (dl, B * 10, "dlogits"),
                          (dcut, B * R.CUT_F, "dcut"), (slabs, nslab * 163850, "slabs"), (work, nwork, "work")):
        R.assert_sentinel(t, used, f"slk_wide_head {what}")
    assert int(err) == 0
    assert torch.equal(_bits(logits[:B]), _bits(zt)), "the one-hot construction did not reproduce the rows"
    _check(f"slk_wide_head B={B}", names, z, y, loss[:B].cpu().numpy(), dl[:B].cpu().numpy())
    assert torch.isfinite(dcut[:B].float()).all() and torch.isfinite(slabs[:nslab]).all()
    assert (work[:nwork].view(torch.uint8) == 0xFF).all(), "keep_threshold 0 keeps every feature"
    # the same rows through the split entry: bit-identical logits, then the same loss from slk_eval_logits' copy
    lg = _nan((B + 1, 10), gpu)
    _lib.call("slk_wide_head_fwd", cut.data_ptr(), wf8.data_ptr(), bf.data_ptr(), step.data_ptr(), 7, 0, 1.0, lg.data_ptr(),
              0, B, s)
    torch.cuda.synchronize()
    R.assert_sentinel(lg, B * 10, "slk_wide_head_fwd logits")
    assert torch.equal(_bits(lg[:B]), _bits(zt))
