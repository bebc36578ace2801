"""The soft-target reference itself (tests/soft_ref64.py), on the CPU: the float64 closed form against torch's
probability-target cross-entropy and against head_ref64.xent64, the pack / unpack twins, the bounds' reduction to the
hard-label bounds, and the float32 emulation of the documented expression inside the bounds — with three wrong
implementations outside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_ref64 as R
import soft_ref64 as S
from splitcnn import loss as L

EPSS = (0.0, 0.1, 1.0)
WBS = (0.0, 0.25, 1.0)


def _random_case(B=64, seed=0):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((B, 10)) * 6).astype(np.float32).astype(np.float64)
    a, b = rng.integers(0, 10, B), rng.integers(0, 10, B)
    wb = rng.random(B).astype(np.float32)
    wb[:4] = (0.0, 1.0, 0.5, 900 / 1024)
    b[4:8] = a[4:8]
    return z, S.pack_np(a, b, wb)


@pytest.mark.parametrize("eps", (0.0, 0.1, 0.5, 1.0))
def test_closed_form_is_torchs_probability_target_path(eps):
    z, y = _random_case()
    loss, dl, _, t = S.soft_xent64(z, y, eps)
    assert np.abs(t.sum(axis=1) - 1).max() < 1e-15
    zt = torch.from_numpy(z).requires_grad_(True)
    probs = torch.from_numpy(S.targets64(y, 0.0))          # torch applies the smoothing itself
    want = F.cross_entropy(zt, probs, label_smoothing=eps, reduction="none")
    assert np.abs(loss - want.detach().numpy()).max() <= 1e-12
    want.sum().backward()
    assert np.abs(dl - zt.grad.numpy()).max() <= 1e-12
    # loss.soft_targets is the same distribution
    assert np.abs(L.soft_targets(torch.from_numpy(y), eps).numpy() - t).max() < 1e-15


def test_closed_form_equals_xent64_on_plain_labels():
    for shift in (0, 11):
        _, z, y = R.xent_batch(33, shift, finite_only=False)
        loss, dl, p, _ = S.soft_xent64(z, y, 0.0)
        loss0, dl0, p0 = R.xent64(z, y)
        assert np.array_equal(loss, loss0) and np.array_equal(dl, dl0) and np.array_equal(p, p0)


def test_pack_unpack_round_trip():
    denorm = np.float32(1e-45)
    assert denorm.view(np.uint32) == 1
    wb = np.array([0.0, 1.0, denorm, 900 / 1024, 0.25, 0.3], dtype=np.float32)
    a = np.array([0, 9, 3, 7, 5, 2])
    b = np.array([0, 0, 9, 7, 1, 8])
    y = S.pack_np(a, b, wb)
    assert y[0] == 0 and y[1] == 9 | (0x3F800000 << 32) and y[2] == 3 | (9 << 8) | (1 << 32)
    yt = L.pack_mixed(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(wb))
    assert yt.dtype == torch.int64 and np.array_equal(yt.numpy(), y)
    import cutmix_ref
    assert np.array_equal(cutmix_ref.pack(a, b, wb), y)
    for ua, ub, uw in (S.unpack_np(y), tuple(t.numpy() for t in L.unpack_mixed(yt)), cutmix_ref.unpack(y)):
        assert np.array_equal(ua, a) and np.array_equal(ub, b)
        assert np.array_equal(np.asarray(uw, dtype=np.float32).view(np.uint32), wb.view(np.uint32))
    # a plain label is a mixed label; one with wb != 0 is out of a hard-label head's range
    pa, pb, pw = L.unpack_mixed(torch.arange(10))
    assert torch.equal(pa, torch.arange(10)) and not pb.any() and not pw.any()
    assert (y[1:] >= 2 ** 32).all()


def test_constructors_validate():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            L.SoftCrossEntropy(bad)
        with pytest.raises(ValueError):
            L.CutMix(bad)
    with pytest.raises(TypeError):
        L.check_loss(0.1)
    assert L.check_loss(None) is None and L.SoftCrossEntropy().label_smoothing == 0.0 and L.CutMix().prob == 1.0


def test_bounds_reduce_to_the_hard_label_bounds():
    _, z, y = R.xent_batch(33, 5)
    loss64, _, p64 = R.xent64(z, y)
    assert np.array_equal(S.soft_loss_bound(z, y, 0.0, loss64), R.loss_bound(z, loss64))
    assert np.array_equal(S.soft_grad_bound(z, y, 0.0, p64), R.grad_bound(z, p64))
    assert np.array_equal(S.soft_gradsum_bound(z, y, 0.0), R.gradsum_bound(z))
    assert not S.t_terms(y, 0.0).any()
    # ... and grow as soon as anything can round
    yb = S.mixed_cases(y, 0.25)
    assert (S.soft_loss_bound(z, yb, 0.0, loss64) >= R.loss_bound(z, loss64)).all()
    grew = S.soft_grad_bound(z, y, 0.1, p64) - R.grad_bound(z, p64)
    assert (grew >= 0).all() and (grew[np.abs(z).max(axis=1) <= 200] > 0).all()   # (absorbed at 1e30, where ulp > 1)


def _ratios(z, y, eps, variant):
    loss64, d64, p64, _ = S.soft_xent64(z, y, eps)
    loss, dl = S.emulate32(z, y, eps, variant=variant)
    with np.errstate(invalid="ignore"):
        rl = np.abs(loss.astype(np.float64) - loss64) / S.soft_loss_bound(z, y, eps, loss64)
        rg = np.abs(dl.astype(np.float64) - d64) / S.soft_grad_bound(z, y, eps, p64)
        rs = np.abs(dl.astype(np.float64).sum(axis=1)) / S.soft_gradsum_bound(z, y, eps)
    return loss, dl, np.nan_to_num(rl, nan=np.inf), np.nan_to_num(rg, nan=np.inf), np.nan_to_num(rs, nan=np.inf)


def _grid():
    names, z, y = R.xent_batch(27, 0)          # every crafted row x label position once
    for eps in EPSS:
        for wb in WBS:
            for same in (False, True):
                yield names, z, S.mixed_cases(y, wb, same=same), eps, wb, same


def test_emulation_of_the_documented_expression_is_inside_the_bounds():
    worst = [0.0, 0.0, 0.0]
    for names, z, y, eps, wb, same in _grid():
        loss, dl, rl, rg, rs = _ratios(z, y, eps, None)
        assert np.isfinite(loss).all() and np.isfinite(dl).all()
        what = f"eps={eps} wb={wb} same={same}"
        assert rl.max() <= 1.0, f"{what}: loss {rl.max():.3f} of its bound at {names[int(rl.argmax())]}"
        assert rg.max() <= 1.0, f"{what}: dlogits {rg.max():.3f} at {names[int(rg.max(axis=1).argmax())]}"
        assert rs.max() <= 1.0, f"{what}: row sum {rs.max():.3f} at {names[int(rs.argmax())]}"
        worst = [max(w, float(r.max())) for w, r in zip(worst, (rl, rg, rs))]
    print(f"largest share of the bounds: loss {worst[0]:.3f}, dlogits {worst[1]:.3f}, row sum {worst[2]:.3f}")


def test_emulation_is_bitwise_the_hard_expression_on_plain_labels():
    """eps = 0 on plain labels: t is exactly one-hot and S = z_a, so loss = fl(lse - z_a) and g = fl(fl(p - onehot) gs)."""
    _, z, y = R.xent_batch(27, 0, finite_only=False)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        loss, dl = S.emulate32(z, y, 0.0)
        z32 = z.astype(np.float32)
        m = z32.max(axis=1)
        se = np.zeros(27, dtype=np.float32)
        for j in range(10):
            se = (se + np.exp(z32[:, j] - m)).astype(np.float32)
        lse = (m + np.log(se)).astype(np.float32)
        want = (lse - z32[np.arange(27), y]).astype(np.float32)
        p = np.exp((z32 - lse[:, None]).astype(np.float32)).astype(np.float32)
    onehot = np.zeros((27, 10), dtype=np.float32)
    onehot[np.arange(27), y] = 1
    assert np.array_equal(loss.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dl.view(np.uint32), (p - onehot).astype(np.float32).view(np.uint32))
    assert np.isfinite(loss).all(), "a -inf logit off the label must contribute nothing"


@pytest.mark.parametrize("variant", [v for v in S.VARIANTS if v])
def test_wrong_variants_leave_the_bounds(variant):
    out_loss = out_grad = 0
    for names, z, y, eps, wb, same in _grid():
        _, _, rl, rg, _ = _ratios(z, y, eps, variant)
        out_loss += int((rl > 1.0).sum())
        out_grad += int((rg > 1.0).any(axis=1).sum())
    assert out_loss > 0 and out_grad > 0, f"{variant}: {out_loss} losses and {out_grad} gradient rows outside the bounds"
    print(f"{variant}: {out_loss} losses, {out_grad} gradient rows outside the bounds")
