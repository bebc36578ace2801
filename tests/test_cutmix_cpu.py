"""The CutMix draws on the CPU: loss.cutmix_draws (the package's host twin of slk_image_batch_mix's box draws)
against tests/cutmix_ref.py, the independent restatement; the box geometry; and the reference batch itself on cases
that need no GPU (prob = 0 and idx2 = idx reduce to the plain augmented batch of cifar_ref.py)."""
import numpy as np
import pytest

import cifar_ref
import cutmix_ref as M
from splitcnn import loss as L

SHAPES = [(32, 32), (28, 28)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("prob", (0.0, 0.5, 1.0))
@pytest.mark.parametrize("seed,epoch", [(0, 0), (7, 3), (0xFFFFFFFF, 0xFFFFFFFF)])
def test_host_twin_equals_the_reference(H, W, prob, seed, epoch):
    idx = np.concatenate([np.arange(300), [49999, 59999, 2 ** 31 - 1]])
    got = L.cutmix_draws(idx, epoch, seed, H, W, prob)
    want = M.boxes(idx, epoch, seed, H, W, prob)
    for g, w, name in zip(got, want, ("apply", "y1", "y2", "x1", "x2", "wb")):
        assert g.dtype == w.dtype or name == "apply", name
        assert np.array_equal(g, w), name
    apply, y1, y2, x1, x2, wb = got
    assert apply.all() if prob == 1.0 else not apply.any() if prob == 0.0 else 0 < apply.sum() < len(idx)
    assert (0 <= y1).all() and (y1 <= y2).all() and (y2 <= H).all()
    assert (0 <= x1).all() and (x1 <= x2).all() and (x2 <= W).all()
    area = np.where(apply, (y2 - y1) * (x2 - x1), 0)
    # wb * H * W is the integer area: exactly for 32 x 32 (a power of two), to within float32's rounding of the
    # quotient (2^-24 * 784 << 1/2) for 28 x 28; and wb is that quotient's float32 division either way
    prod = wb.astype(np.float64) * (H * W)
    assert np.array_equal(np.rint(prod), area) and np.abs(prod - area).max() <= 2.0 ** -24 * H * W
    if (H * W) & (H * W - 1) == 0:
        assert np.array_equal(prod, area)
    assert np.array_equal(wb, area.astype(np.float32) / np.float32(H * W))
    assert wb.dtype == np.float32 and (wb[~apply] == 0).all() and (wb < 1).all()


def test_box_statistics_at_seed_0():
    """lam ~ Beta(1, 1): side = max of two uniforms has density 2r, so E[area / HW] is about 1/3 minus the clipping."""
    apply, y1, y2, x1, x2, wb = L.cutmix_draws(np.arange(2048), 0, 0, 32, 32, 1.0)
    assert apply.all()
    assert 0.27 < wb.mean() < 0.33
    empty = (wb == 0).mean()
    assert 0 < empty < 0.02
    assert (y2 - y1).max() <= 30 and (x2 - x1).max() <= 30, "side <= H - 1, so 2 (side / 2) <= 30"
    # a sample's box does not depend on what else is in the call
    one = L.cutmix_draws(np.array([1234]), 0, 0, 32, 32, 1.0)
    assert all(np.array_equal(o[0], f[1234]) for o, f in zip(one, (apply, y1, y2, x1, x2, wb)))
    # ... and changes with the epoch and the seed
    assert not np.array_equal(L.cutmix_draws(np.arange(2048), 1, 0, 32, 32, 1.0)[5], wb)
    assert not np.array_equal(L.cutmix_draws(np.arange(2048), 0, 1, 32, 32, 1.0)[5], wb)


@pytest.mark.parametrize("shape,pad,mean,std", [((3, 32, 32), 4, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)),
                                                ((1, 28, 28), 2, (0.1307,), (0.3081,))])
def test_reference_batch_reduces_to_the_plain_batch(shape, pad, mean, std):
    images, labels = M.synthetic(64, shape, 5)
    idx = np.array([0, 63, 17, 5, 40, 63])
    idx2 = np.roll(idx, 1)
    plain_x, plain_y = cifar_ref.batch(images, labels, idx, mean, std, pad=pad, flip=True, seed=3, epoch=2)
    x0, y0 = M.batch(images, labels, idx, idx2, mean, std, pad=pad, flip=True, seed=3, epoch=2, prob=0.0)
    assert np.array_equal(x0.view(np.uint32), plain_x.view(np.uint32)) and np.array_equal(y0, plain_y)
    xs, ys = M.batch(images, labels, idx, idx, mean, std, pad=pad, flip=True, seed=3, epoch=2, prob=1.0)
    assert np.array_equal(xs.view(np.uint32), plain_x.view(np.uint32))
    a, b, wb = M.unpack(ys)
    assert np.array_equal(a, plain_y) and (np.array_equal(b[wb > 0], a[wb > 0]))
    # mixed: inside the box the partner's own augmented pixel, outside the primary's
    xm, ym = M.batch(images, labels, idx, idx2, mean, std, pad=pad, flip=True, seed=3, epoch=2, prob=1.0)
    part_x, part_y = cifar_ref.batch(images, labels, idx2, mean, std, pad=pad, flip=True, seed=3, epoch=2)
    apply, y1, y2, x1, x2, wb = L.cutmix_draws(idx, 2, 3, shape[1], shape[2], 1.0)
    for s in range(len(idx)):
        inside = np.zeros(shape[1:], dtype=bool)
        inside[y1[s]:y2[s], x1[s]:x2[s]] = True
        want = np.where(inside[None], part_x[s], plain_x[s])
        assert np.array_equal(xm[s].view(np.uint32), want.view(np.uint32)), s
        a, b, w = M.unpack(ym[s:s + 1])
        assert a[0] == plain_y[s] and w[0] == wb[s] and (b[0] == part_y[s] if wb[s] > 0 else b[0] == 0)
