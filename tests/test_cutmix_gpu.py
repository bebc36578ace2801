"""GPU tests of slk_image_batch_mix (CutMix in the batch kernel) and the loaders' mix=: both instantiations bit for
bit against the independent pixel-loop reference (tests/cutmix_ref.py) at B = 33, on indices the test picks with the
host twin (loss.cutmix_draws) so that every way a box can cut a quad occurs — and asserts that it does.

A quad is four output columns; a box edge at x1 or x2 cuts it at x mod 4, and each source is gathered forwards or
backwards (its own flip). Among non-empty boxes the reachable (x1 mod 4, x2 mod 4) pairs are the 12 with equal parity
(x2 - x1 = 2 (side / 2) unless clipped), or x1 = 0, or x2 = W; each must occur with each (flip_i, flip_i2).
Outputs are prefilled with NaN / -1 and carry a sentinel row; every comparison is np.array_equal."""
import ctypes

import numpy as np
import pytest
import torch

import cifar_ref
import cutmix_ref as M

pytestmark = pytest.mark.gpu

N = 2048
B = 33
SHAPES = {"cifar": dict(shape=(3, 32, 32), pad=4, mean=(0.4914, 0.4822, 0.4465), std=(0.2470, 0.2435, 0.2616)),
          "mnist": dict(shape=(1, 28, 28), pad=2, mean=(0.1307,), std=(0.3081,))}


@pytest.fixture(scope="module", params=list(SHAPES))
def data(request, gpu):
    d = dict(SHAPES[request.param], name=request.param)
    img, lbl = M.synthetic(N, d["shape"], 21)
    img[0], img[N - 1] = 0, 255
    d.update(img=img, lbl=lbl, dimg=torch.from_numpy(img).to(gpu), dlbl=torch.from_numpy(lbl).to(gpu))
    return d


def _floats(v):
    return (ctypes.c_float * len(v))(*v)


def _run(d, idx, idx2, gpu, **kw):
    """ops.image_batch_mix into prefilled buffers with a sentinel row; numpy (x, y, err)."""
    from splitcnn import ops
    n = len(idx)
    xf = torch.full((n + 1,) + d["shape"], float("nan"), dtype=torch.float32, device=gpu)
    yf = torch.full((n + 1,), -1, dtype=torch.int64, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    dev = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(gpu)   # noqa: E731
    x, y = ops.image_batch_mix(d["dimg"], d["dlbl"], dev(idx), dev(idx2), mean=d["mean"], std=d["std"], x=xf[:n],
                               y=yf[:n], err_flag=err, **kw)
    torch.cuda.synchronize()
    assert x.data_ptr() == xf.data_ptr() and y.data_ptr() == yf.data_ptr()
    assert bool(torch.isnan(xf[n]).all()) and int(yf[n]) == -1, "wrote behind the last row"
    return xf[:n].cpu().numpy(), yf[:n].cpu().numpy(), int(err.item())


def _check(d, idx, idx2, gpu, **kw):
    x, y, err = _run(d, idx, idx2, gpu, **kw)
    wx, wy = M.batch(d["img"], d["lbl"], idx, idx2, d["mean"], d["std"], **kw)
    assert err == 0 and not np.isnan(x).any()
    bad = [s for s in range(len(idx)) if not np.array_equal(x[s].view(np.uint32), wx[s].view(np.uint32))]
    assert not bad, f"x differs from the reference at batch positions {bad} (idx {[int(idx[s]) for s in bad]})"
    assert np.array_equal(y, wy)
    return x, y


def _plain(d, idx, gpu, **kw):
    from splitcnn import ops
    x, y = ops.image_batch(d["dimg"], d["dlbl"], torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(gpu), mean=d["mean"],
                           std=d["std"], **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), y.cpu().numpy()


def _pick(d, seed=0, epoch=0):
    """(idx, idx2, cases): primaries and partners covering every (x1 % 4, x2 % 4, flip_i, flip_i2), a box on each
    border, an empty applied box, and dataset rows 0 and N - 1 on both sides."""
    from splitcnn.cifar import augment_draws
    from splitcnn.loss import cutmix_draws
    _, H, W = d["shape"]
    allidx = np.arange(N)
    apply, y1, y2, x1, x2, wb = cutmix_draws(allidx, epoch, seed, H, W, 1.0)
    _, _, fl = augment_draws(allidx, epoch, seed, d["pad"], True)
    full = wb > 0
    pairs = {(int(a) % 4, int(b) % 4) for a, b in zip(x1[full], x2[full])}
    want = {(p, q) for p in range(4) for q in range(4) if p % 2 == q % 2} | {(0, 1), (0, 3), (1, W % 4), (3, W % 4)}
    assert pairs == want and len(want) == 12, sorted(pairs)
    idx, idx2 = [], []
    by_flip = {f: [int(i) for i in allidx[fl == f]] for f in (0, 1)}
    k = 0
    for p, q in sorted(want):
        for fi in (0, 1):
            for f2 in (0, 1):
                c = allidx[full & (x1 % 4 == p) & (x2 % 4 == q) & (fl == fi)]
                assert len(c), f"no sample with box columns ({p}, {q}) mod 4 and flip {fi}"
                idx.append(int(c[k % len(c)]))
                idx2.append(by_flip[f2][(7 * k + 3) % len(by_flip[f2])])
                k += 1
    for cond in (full & (y1 == 0), full & (y2 == H), full & (x1 == 0), full & (x2 == W), apply & ~full):
        assert cond.sum() >= 1
        idx.append(int(allidx[cond][0]))
        idx2.append(int(allidx[cond][-1]))
    assert (full & (x1 == 0)).sum() > 100 and (full & (x2 == W)).sum() > 100
    idx += [0, N - 1, 5, 6]
    idx2 += [9, 10, 0, N - 1]
    cases = {(int(x1[i]) % 4, int(x2[i]) % 4, int(fl[i]), int(fl[j])) for i, j in zip(idx, idx2) if full[i]}
    assert len(cases) == 48
    return np.array(idx), np.array(idx2)


def test_mix_bit_for_bit_on_every_quad_case(gpu, data):
    idx, idx2 = _pick(data)
    fill = (-len(idx)) % B
    idx, idx2 = np.concatenate([idx, np.arange(100, 100 + fill)]), np.concatenate([idx2, np.arange(300, 300 + fill)])
    assert len(idx) % B == 0 and len(idx) // B >= 2
    kw = dict(pad=data["pad"], flip=True, seed=0, epoch=0)
    for k in range(0, len(idx), B):
        _check(data, idx[k:k + B], idx2[k:k + B], gpu, prob=1.0, **kw)
    # prob = 0.5: the same positions, about half of them unapplied
    from splitcnn.loss import cutmix_draws
    ap = cutmix_draws(idx[:B], 0, 0, data["shape"][1], data["shape"][2], 0.5)[0]
    assert ap.any() and not ap.all()
    x, y = _check(data, idx[:B], idx2[:B], gpu, prob=0.5, **kw)
    px, py = _plain(data, idx[:B], gpu, **kw)
    assert np.array_equal(x[~ap].view(np.uint32), px[~ap].view(np.uint32)) and np.array_equal(y[~ap], py[~ap])
    # other seeds, epochs and pads (pad 0 without flip: what a loader with mix but no augment launches)
    _check(data, idx[B:2 * B], idx2[B:2 * B], gpu, prob=1.0, pad=0, flip=False, seed=5, epoch=2)
    _check(data, idx[B:2 * B], idx2[B:2 * B], gpu, prob=1.0, pad=8, flip=True, seed=0xFFFFFFFF, epoch=0x80000001)


def test_mix_prob0_and_self_partner_are_the_plain_batch(gpu, data):
    rng = np.random.default_rng(3)
    idx = np.concatenate([[0, N - 1], rng.integers(0, N, size=B - 2)])
    idx2 = np.roll(idx, 1)
    kw = dict(pad=data["pad"], flip=True, seed=2, epoch=1)
    px, py = _plain(data, idx, gpu, **kw)
    x, y, err = _run(data, idx, idx2, gpu, prob=0.0, **kw)
    assert err == 0 and np.array_equal(x.view(np.uint32), px.view(np.uint32)) and np.array_equal(y, py)
    x, y, err = _run(data, idx, idx, gpu, prob=1.0, **kw)
    assert err == 0 and np.array_equal(x.view(np.uint32), px.view(np.uint32))
    a, b, wb = M.unpack(y)
    from splitcnn.loss import cutmix_draws
    assert np.array_equal(a, py) and np.array_equal(wb, cutmix_draws(idx, 1, 2, *data["shape"][1:], 1.0)[5])
    assert (wb > 0).sum() > B // 2 and np.array_equal(b[wb > 0], a[wb > 0]) and (b[wb == 0] == 0).all()


def test_mix_fallback_and_refusals(gpu, data):
    from splitcnn import _lib, ops
    kw = dict(pad=data["pad"], flip=True, seed=0, epoch=1, prob=1.0)
    idx = np.array([5, 7, N - 1, 9, -1, 11], dtype=np.int64)
    idx2 = np.array([6, -1, N, 2 ** 40, 8, 0], dtype=np.int64)
    x, y, err = _run(data, idx, idx2, gpu, **kw)
    src, src2 = np.where((idx < 0) | (idx >= N), 0, idx), np.where((idx2 < 0) | (idx2 >= N), 0, idx2)
    wx, wy = M.batch(data["img"], data["lbl"], src, src2, data["mean"], data["std"], **kw)
    assert err == 1, "an out-of-range idx2 (or idx) sets the flag"
    assert np.array_equal(x.view(np.uint32), wx.view(np.uint32)) and np.array_equal(y, wy)   # row 0 with row 0's draws
    assert _run(data, src, src2, gpu, **kw)[2] == 0
    assert _run(data, np.array([5, 6]), np.array([7, N]), gpu, **kw)[2] == 1                 # idx2 alone
    assert _run(data, np.array([-3, 6]), np.array([7, 8]), gpu, **kw)[2] == 1                # idx alone
    # B = 1: its own partner, and another row's
    for one, two in (([7], [7]), ([7], [N - 1]), ([0], [3])):
        _check(data, np.array(one), np.array(two), gpu, **kw)

    C, H, W = data["shape"]
    ids = torch.zeros(4, dtype=torch.int64, device=gpu)
    out = torch.full((4, C, H, W), float("nan"), device=gpu)
    yo = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    args = dict(images=data["dimg"].data_ptr(), labels=data["dlbl"].data_ptr(), idx=ids.data_ptr(), idx2=ids.data_ptr(),
                x=out.data_ptr(), y=yo.data_ptr(), C=C, H=H, W=W, pad=0, prob=1.0)

    def call(**over):
        a = dict(args, **over)
        return _lib.load().slk_image_batch_mix(a["images"], a["labels"], 8, a["C"], a["H"], a["W"], a["idx"], a["idx2"], 4,
                                               _floats(data["mean"]), _floats(data["std"]), a["pad"], 0, 0, 0, a["prob"],
                                               a["x"], a["y"], None, None)
    for over in (dict(images=args["images"] + 1), dict(x=args["x"] + 4), dict(images=None), dict(labels=None),
                 dict(idx=None), dict(idx2=None), dict(x=None), dict(y=None), dict(H=H - 4), dict(C=C + 1), dict(pad=9),
                 dict(pad=-1), dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan"))):
        assert call(**over) == 1, over
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((yo == -1).all()), "a refused call launched"
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    x0, y0 = ops.image_batch_mix(data["dimg"], data["dlbl"], ids[:0], ids[:0], mean=data["mean"], std=data["std"])
    assert tuple(x0.shape) == (0, C, H, W) and tuple(y0.shape) == (0,)


# ------------------------------------------------------------------------------------ the loaders
class _Set:
    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return len(self.images)


def _loader(d, gpu, n, **kw):
    from splitcnn.cifar import CifarLoader
    from splitcnn.mnist import DeviceLoader
    if d["name"] == "cifar":
        return CifarLoader(_Set(d["img"][:n], d["lbl"][:n]), device=gpu, **kw)
    return DeviceLoader(_Set(d["img"][:n, 0], d["lbl"][:n]), device=gpu, **kw)


@pytest.mark.parametrize("augment", [True, False])
def test_loaders_mix(gpu, data, augment):
    from splitcnn.cifar import Augment
    from splitcnn.loss import CutMix, cutmix_draws
    n = 100
    aug = Augment(pad=data["pad"], flip=True, seed=4) if augment else None
    mix = CutMix(prob=1.0, seed=4)
    kw = dict(pad=data["pad"], flip=True) if augment else dict(pad=0, flip=False)
    got = {}
    for bs in (32, 25):
        ld = _loader(data, gpu, n, batch_size=bs, shuffle=False, augment=aug, mix=mix)
        ld.set_epoch(3)
        xs, ys = zip(*[(x.cpu().numpy(), y.cpu().numpy()) for x, y in ld])
        assert [len(x) for x in xs] == [bs] * (n // bs) + ([n % bs] if n % bs else []) and int(ld.err.item()) == 0
        got[bs] = (np.concatenate(xs), np.concatenate(ys))
        assert ld.epoch == 4
    # the partner of sample s is s - 1 except at a batch start: everywhere else neither x nor y depends on batch size
    inner = np.array([s for s in range(n) if s % 32 and s % 25])
    assert np.array_equal(got[32][0][inner].view(np.uint32), got[25][0][inner].view(np.uint32))
    assert np.array_equal(got[32][1][inner], got[25][1][inner])
    # y unpacks to the two dataset labels and the box's weight
    a, b, wb = M.unpack(got[32][1])
    partner = np.array([(s - 1) if s % 32 else min(s + 31, n - 1) for s in range(n)])
    assert np.array_equal(a, data["lbl"][:n]) and np.array_equal(wb, cutmix_draws(np.arange(n), 3, 4, *data["shape"][1:], 1.0)[5])
    assert np.array_equal(b[wb > 0], data["lbl"][partner][wb > 0]) and (b[wb == 0] == 0).all()
    # the ragged last batch (96..99) rolls within itself, bit for bit the reference's batch
    last = np.arange(96, 100)
    wx, wy = M.batch(data["img"], data["lbl"], last, np.roll(last, 1), data["mean"], data["std"], seed=4, epoch=3, prob=1.0, **kw)
    assert np.array_equal(got[32][0][96:].view(np.uint32), wx.view(np.uint32)) and np.array_equal(got[32][1][96:], wy)
    # shuffled: the same samples with the same boxes, whatever the order
    ld = _loader(data, gpu, n, batch_size=32, shuffle=True, seed=1, augment=aug, mix=mix)
    ld.set_epoch(3)
    state = ld.gen.get_state()
    order = ld.order().numpy()
    ld.gen.set_state(state)
    ysh = np.concatenate([y.cpu().numpy() for _, y in ld])
    sa, _, swb = M.unpack(ysh)
    assert np.array_equal(sa, data["lbl"][order]) and np.array_equal(swb, wb[order])
    # mix=None is untouched: plain labels
    ld = _loader(data, gpu, n, batch_size=32, shuffle=False, augment=aug)
    assert all(int(y.max()) < 10 for _, y in ld)
    with pytest.raises(TypeError):
        _loader(data, gpu, n, mix=0.5)
