"""GPU tests of slk_image_batch_blend (CutMix from a Beta quantile table, MixUp, and the per-sample switch) and the
loaders' mix=: both instantiations bit for bit against the independent pixel-loop reference (tests/mixup_ref.py) at
B = 33, on indices picked from the reference's own draws so that every way a box cuts a quad, every hand-made weight,
every crop offset and every mode occurs under every flip pair — the pickers assert that they do. Outputs are prefilled
with NaN / -1 and carry a sentinel row; every comparison is np.array_equal on bits."""
import ctypes

import numpy as np
import pytest
import torch

import cutmix_ref as M
import mixup_ref as R

pytestmark = pytest.mark.gpu

N, B = R.N, R.B


@pytest.fixture(scope="module", params=list(R.SHAPES))
def data(request, gpu):
    d = dict(R.SHAPES[request.param], name=request.param)
    img, lbl = R.dataset(request.param)
    d.update(img=img, lbl=lbl, dimg=torch.from_numpy(img).to(gpu), dlbl=torch.from_numpy(lbl).to(gpu))
    return d


def _floats(v):
    return (ctypes.c_float * len(v))(*v)


def _tables(gpu, cut_table=None, lam_table=None):
    """The numpy tables as the device tensors ops.image_batch_blend takes (uint32 bits in an int32 tensor)."""
    kw = {}
    if cut_table is not None:
        kw["cut_table"] = torch.from_numpy(np.ascontiguousarray(cut_table).view(np.int32)).to(gpu)
    if lam_table is not None:
        kw["lam_table"] = torch.from_numpy(np.ascontiguousarray(lam_table, dtype=np.float32)).to(gpu)
    return kw


def _run(d, idx, idx2, gpu, cut_table=None, lam_table=None, **kw):
    """ops.image_batch_blend into prefilled buffers with a sentinel row; numpy (x, y, err)."""
    from splitcnn import ops
    n = len(idx)
    xf = torch.full((n + 1,) + d["shape"], float("nan"), dtype=torch.float32, device=gpu)
    yf = torch.full((n + 1,), -1, dtype=torch.int64, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    dev = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(gpu)   # noqa: E731
    tabs = _tables(gpu, cut_table, lam_table)
    keep = {k: v.clone() for k, v in tabs.items()}
    x, y = ops.image_batch_blend(d["dimg"], d["dlbl"], dev(idx), dev(idx2), mean=d["mean"], std=d["std"], x=xf[:n],
                                 y=yf[:n], err_flag=err, **tabs, **kw)
    torch.cuda.synchronize()
    assert x.data_ptr() == xf.data_ptr() and y.data_ptr() == yf.data_ptr()
    assert bool(torch.isnan(xf[n]).all()) and int(yf[n]) == -1, "wrote behind the last row"
    assert all(torch.equal(tabs[k], keep[k]) for k in tabs), "the tables are only read"
    return xf[:n].cpu().numpy(), yf[:n].cpu().numpy(), int(err.item())


def _check(d, idx, idx2, gpu, **kw):
    x, y, err = _run(d, idx, idx2, gpu, **kw)
    info = []
    wx, wy = R.batch(d["img"], d["lbl"], idx, idx2, d["mean"], d["std"], info=info, **kw)
    assert err == 0 and not np.isnan(x).any()
    bad = [s for s in range(len(idx)) if not np.array_equal(x[s].view(np.uint32), wx[s].view(np.uint32))]
    assert not bad, f"x differs from the reference at batch positions {bad}: {[(int(idx[s]), info[s][0], info[s][7]) for s in bad]}"
    assert np.array_equal(y, wy)
    return x, y, info


def _plain(d, idx, gpu, **kw):
    from splitcnn import ops
    x, y = ops.image_batch(d["dimg"], d["dlbl"], torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(gpu), mean=d["mean"],
                           std=d["std"], **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), y.cpu().numpy()


def _mix(d, idx, idx2, gpu, **kw):
    from splitcnn import ops
    dev = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(gpu)   # noqa: E731
    x, y = ops.image_batch_mix(d["dimg"], d["dlbl"], dev(idx), dev(idx2), mean=d["mean"], std=d["std"], **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), y.cpu().numpy()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------ (a) the cut table alone
def test_cut_table_bit_for_bit_on_every_quad_case(gpu, data):
    from splitcnn.loss import cut_table, cutmix_draws, mix_draws
    _, H, W = data["shape"]
    ct = cut_table(1.0)
    d = R.draws(H, W, data["pad"], cut_table=ct)
    idx, idx2 = R.pick_cut(d, W)
    assert len(idx) % B == 0 and len(idx) // B >= 2
    # the host twin draws what the reference draws, and picks the samples slk_image_batch_mix would
    apply, cut, k, y1, y2, x1, x2, wb = mix_draws(np.arange(N), 0, 0, H, W, 1.0, 0.5, ct, None)
    assert apply.all() and cut.all() and np.array_equal(wb.view(np.uint32), d["wb"].view(np.uint32))
    assert all(np.array_equal(g, d[n]) for g, n in ((y1, "y1"), (y2, "y2"), (x1, "x1"), (x2, "x2"), (k, "k")))
    assert (wb == 0).sum() >= 1 and (x1[wb > 0] == 0).sum() > 100 and (x2[wb > 0] == W).sum() > 100
    kw = dict(pad=data["pad"], flip=True, seed=0, epoch=0)
    for j in range(0, len(idx), B):
        _check(data, idx[j:j + B], idx2[j:j + B], gpu, cut_table=ct, prob=1.0, **kw)
    # prob = 0.5: the same positions, the unapplied ones plain, and the applied ones those slk_image_batch_mix applies
    ap = cutmix_draws(idx[:B], 0, 0, H, W, 0.5)[0]
    assert ap.any() and not ap.all()
    x, y, info = _check(data, idx[:B], idx2[:B], gpu, cut_table=ct, prob=0.5, **kw)
    assert [i[0] != "plain" for i in info] == ap.tolist()
    px, py = _plain(data, idx[:B], gpu, **kw)
    assert _same(x[~ap], px[~ap]) and np.array_equal(y[~ap], py[~ap])
    # other seeds, epochs, pads and another alpha (pad 0 without flip: what a loader with mix but no augment launches)
    _check(data, idx[B:2 * B], idx2[B:2 * B], gpu, cut_table=cut_table(0.3), prob=1.0, pad=0, flip=False, seed=5, epoch=2)
    _check(data, idx[B:2 * B], idx2[B:2 * B], gpu, cut_table=cut_table(4.0), prob=1.0, pad=8, flip=True, seed=0xFFFFFFFF,
           epoch=0x80000001)


# ------------------------------------------------------------------------------------ (b) the blend
def test_blend_bit_for_bit_on_a_hand_made_table(gpu, data):
    _, H, W = data["shape"]
    table = R.hand_table()
    pad = 4                                  # both shapes: quads and rows wholly in either source's padding
    d = R.draws(H, W, pad, lam_table=table)
    idx, idx2 = R.pick_blend(d, pad)
    kw = dict(pad=pad, flip=True, seed=0, epoch=0)
    px, py = _plain(data, idx, gpu, **kw)
    p2x, _ = _plain(data, idx2, gpu, **kw)
    seen = set()
    for j in range(0, len(idx), B):
        sl = slice(j, j + B)
        x, y, info = _check(data, idx[sl], idx2[sl], gpu, lam_table=table, prob=1.0, **kw)
        a, b, wb = M.unpack(y)
        want_wb = d["wb"][idx[sl]]
        assert all(i[0] == "blend" for i in info)
        assert np.array_equal(a, data["lbl"][idx[sl]]) and np.array_equal(wb.view(np.uint32), want_wb.view(np.uint32))
        assert np.array_equal(b[want_wb > 0], data["lbl"][idx2[sl]][want_wb > 0])
        zero = want_wb == 0
        assert np.array_equal(y[zero], py[sl][zero]), "wb = 0: the plain label"
        assert ((y[want_wb > 0] >> 32) != 0).all(), "a denormal weight is still a mixed label"
        tiny = want_wb < 1e-30                # 0 and the denormal: bitwise slk_image_batch's row
        assert _same(x[tiny], px[sl][tiny])
        one = want_wb == 1
        assert _same(x[one], p2x[sl][one]), "wb = 1: the partner's plain image"
        mid = (want_wb > 0.1) & (want_wb < 0.95)
        assert all(not _same(x[s], px[sl][s]) and not _same(x[s], p2x[sl][s]) for s in np.flatnonzero(mid))
        seen |= set(want_wb.view(np.uint32).tolist())
    assert set(R.HAND_VALUES.view(np.uint32).tolist()) <= seen


# ------------------------------------------------------------------------------------ (c) the switch
def test_switch_three_modes_under_every_flip_pair(gpu, data):
    from splitcnn.loss import cut_table, lam_table, mix_draws
    _, H, W = data["shape"]
    ct, lt = cut_table(0.5), lam_table(0.4)
    d = R.draws(H, W, data["pad"], prob=0.5, switch=0.5, cut_table=ct, lam_table=lt)
    for mode in ("cut", "blend", "plain"):
        for f in (0, 1):
            assert ((d["mode"] == mode) & (d["fl"] == f)).sum() >= 200, (mode, f)
    idx, idx2 = R.pick_switch(d)
    assert len(idx) == B
    kw = dict(pad=data["pad"], flip=True, seed=0, epoch=0)
    x, y, info = _check(data, idx, idx2, gpu, cut_table=ct, lam_table=lt, prob=0.5, switch=0.5, **kw)
    assert {i[0] for i in info[:12]} == {"cut", "blend", "plain"}
    apply, cut, k, y1, y2, x1, x2, wb = mix_draws(idx, 0, 0, H, W, 0.5, 0.5, ct, lt)
    assert np.where(apply & cut, "cut", np.where(apply, "blend", "plain")).tolist() == [i[0] for i in info]
    assert np.array_equal(M.unpack(y)[2].view(np.uint32), wb.view(np.uint32))
    _check(data, idx, idx2, gpu, cut_table=ct, lam_table=lt, prob=0.7, switch=0.3, pad=0, flip=False, seed=9, epoch=4)


# ------------------------------------------------------------------------------------ (d) prob = 0
def test_prob0_is_the_plain_batch(gpu, data):
    from splitcnn.loss import cut_table, lam_table
    rng = np.random.default_rng(3)
    idx = np.concatenate([[0, N - 1], rng.integers(0, N, size=B - 2)])
    idx2 = np.roll(idx, 1)
    kw = dict(pad=data["pad"], flip=True, seed=2, epoch=1)
    px, py = _plain(data, idx, gpu, **kw)
    for tabs in (dict(cut_table=cut_table(2.0)), dict(lam_table=lam_table(2.0)),
                 dict(cut_table=cut_table(2.0), lam_table=lam_table(0.5))):
        x, y, err = _run(data, idx, idx2, gpu, prob=0.0, **tabs, **kw)
        assert err == 0 and _same(x, px) and np.array_equal(y, py)
    # the partner being the sample itself: CutMix shows the plain image; MixUp at 0.5 too (a/2 + a/2 is exact)
    x, y, err = _run(data, idx, idx, gpu, prob=1.0, cut_table=cut_table(2.0), **kw)
    assert err == 0 and _same(x, px)
    x, y, err = _run(data, idx, idx, gpu, prob=1.0, lam_table=np.full(1024, 0.5, dtype=np.float32), **kw)
    assert err == 0 and _same(x, px)
    a, b, wb = M.unpack(y)
    assert np.array_equal(a, py) and np.array_equal(b, py) and (wb == 0.5).all()


# ------------------------------------------------------------------------------------ (e) the entry's other behaviours
def test_switch_extremes_equal_the_one_table_launches(gpu, data):
    from splitcnn.loss import cut_table, lam_table
    rng = np.random.default_rng(4)
    idx = rng.integers(0, N, size=B)
    idx2 = np.roll(idx, 1)
    ct, lt = cut_table(0.5), lam_table(0.4)
    kw = dict(pad=data["pad"], flip=True, seed=1, epoch=2, prob=0.8)
    xc, yc, _ = _run(data, idx, idx2, gpu, cut_table=ct, **kw)
    xl, yl, _ = _run(data, idx, idx2, gpu, lam_table=lt, **kw)
    x1, y1, _ = _run(data, idx, idx2, gpu, cut_table=ct, lam_table=lt, switch=1.0, **kw)
    x0, y0, _ = _run(data, idx, idx2, gpu, cut_table=ct, lam_table=lt, switch=0.0, **kw)
    assert _same(x1, xc) and np.array_equal(y1, yc) and _same(x0, xl) and np.array_equal(y0, yl)
    assert not _same(xc, xl)
    # one table alone ignores `switch`
    xs, ys, _ = _run(data, idx, idx2, gpu, cut_table=ct, switch=0.0, **kw)
    assert _same(xs, xc) and np.array_equal(ys, yc)


def test_tiny_batches_fallback_and_refusals(gpu, data):
    from splitcnn import _lib, ops
    from splitcnn.loss import cut_table, lam_table
    ct, lt = cut_table(0.5), lam_table(0.4)
    kw = dict(pad=data["pad"], flip=True, seed=0, epoch=1, prob=1.0, switch=0.5, cut_table=ct, lam_table=lt)
    # B = 1 (its own partner, and another row's) and B = 0
    for one, two in (([7], [7]), ([7], [N - 1]), ([0], [3])):
        _check(data, np.array(one), np.array(two), gpu, **kw)
    tabs = _tables(gpu, ct, lt)
    ids = torch.zeros(4, dtype=torch.int64, device=gpu)
    x0, y0 = ops.image_batch_blend(data["dimg"], data["dlbl"], ids[:0], ids[:0], mean=data["mean"], std=data["std"], **tabs)
    C, H, W = data["shape"]
    assert tuple(x0.shape) == (0, C, H, W) and tuple(y0.shape) == (0,)
    # out-of-range indices: the flag, then row 0 with row 0's draws
    idx = np.array([5, 7, N - 1, 9, -1, 11], dtype=np.int64)
    idx2 = np.array([6, -1, N, 2 ** 40, 8, 0], dtype=np.int64)
    x, y, err = _run(data, idx, idx2, gpu, **kw)
    src, src2 = np.where((idx < 0) | (idx >= N), 0, idx), np.where((idx2 < 0) | (idx2 >= N), 0, idx2)
    wx, wy = R.batch(data["img"], data["lbl"], src, src2, data["mean"], data["std"], **kw)
    assert err == 1, "an out-of-range idx2 (or idx) sets the flag"
    assert _same(x, wx) and np.array_equal(y, wy)
    assert _run(data, src, src2, gpu, **kw)[2] == 0
    assert _run(data, np.array([5, 6]), np.array([7, N]), gpu, **kw)[2] == 1                 # idx2 alone
    assert _run(data, np.array([-3, 6]), np.array([7, 8]), gpu, **kw)[2] == 1                # idx alone

    out = torch.full((4, C, H, W), float("nan"), device=gpu)
    yo = torch.full((4,), -1, dtype=torch.int64, device=gpu)
    args = dict(images=data["dimg"].data_ptr(), labels=data["dlbl"].data_ptr(), idx=ids.data_ptr(), idx2=ids.data_ptr(),
                x=out.data_ptr(), y=yo.data_ptr(), C=C, H=H, W=W, pad=0, prob=1.0, switch=0.5,
                cut=tabs["cut_table"].data_ptr(), lam=tabs["lam_table"].data_ptr())

    def call(**over):
        a = dict(args, **over)
        return _lib.load().slk_image_batch_blend(a["images"], a["labels"], 8, a["C"], a["H"], a["W"], a["idx"], a["idx2"],
                                                 4, _floats(data["mean"]), _floats(data["std"]), a["pad"], 0, 0, 0,
                                                 a["prob"], a["cut"], a["lam"], a["switch"], a["x"], a["y"], None, None)
    for over in (dict(cut=None, lam=None), dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(switch=-0.1),
                 dict(switch=1.5), dict(switch=float("nan")), dict(x=args["x"] + 4), dict(images=args["images"] + 1),
                 dict(cut=args["cut"] + 2), dict(lam=args["lam"] + 1), dict(images=None), dict(labels=None), dict(idx=None),
                 dict(idx2=None), dict(x=None), dict(y=None), dict(H=H - 4), dict(C=C + 1), dict(pad=9), dict(pad=-1)):
        assert call(**over) == 1, over
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((yo == -1).all()), "a refused call launched"
    for over in ({}, dict(cut=None), dict(lam=None)):
        out.fill_(float("nan"))
        assert call(**over) == 0, over
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any())
    # the Python layer: a table of the wrong length, dtype or device, and none at all
    bad = dict(mean=data["mean"], std=data["std"])
    with pytest.raises(ValueError, match="shape"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, lam_table=tabs["lam_table"][:512], **bad)
    with pytest.raises(TypeError, match="cut_table"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, cut_table=tabs["lam_table"], **bad)
    with pytest.raises(TypeError, match="lam_table"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, lam_table=tabs["cut_table"], **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, lam_table=tabs["lam_table"].cpu(), **bad)
    with pytest.raises(ValueError, match="cut_table, lam_table or both"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, **bad)
    with pytest.raises(_lib.SLKError, match="invalid argument"):
        ops.image_batch_blend(data["dimg"], data["dlbl"], ids, ids, lam_table=tabs["lam_table"], switch=2.0, **bad)


# ------------------------------------------------------------------------------------ (f) the loaders
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


def _epoch(ld):
    xs, ys = zip(*[(x.cpu().numpy(), y.cpu().numpy()) for x, y in ld])
    return np.concatenate(xs), np.concatenate(ys)


def _mixes():
    from splitcnn.loss import CutMix, Mix, MixUp
    return {"mixup": MixUp(0.4, seed=4), "mix": Mix(0.5, 0.4, prob=0.8, switch=0.5, seed=4),
            "cutmix_alpha": CutMix(alpha=0.5, seed=4), "mixup_default": MixUp(seed=4)}


@pytest.mark.parametrize("which,augment", [("mixup", True), ("mix", True), ("cutmix_alpha", False), ("mixup_default", False)])
def test_loaders_mix(gpu, data, which, augment):
    """CifarLoader and DeviceLoader (the `data` fixture's two shapes) under each of the new mixes."""
    from splitcnn.cifar import Augment
    from splitcnn.loss import CutMix, MixUp, cut_table, lam_table
    mix = _mixes()[which]
    n = 70
    aug = Augment(pad=data["pad"], flip=True, seed=4) if augment else None
    kw = dict(pad=data["pad"], flip=True) if augment else dict(pad=0, flip=False)
    tabs = dict(cut_table=None if isinstance(mix, MixUp) else cut_table(mix.alpha if isinstance(mix, CutMix) else mix.cutmix_alpha),
                lam_table=None if isinstance(mix, CutMix) else lam_table(mix.alpha if isinstance(mix, MixUp) else mix.mixup_alpha))
    got = {}
    for bs in (32, 25):
        ld = _loader(data, gpu, n, batch_size=bs, shuffle=False, augment=aug, mix=mix)
        assert (ld._cut_table is None) == (tabs["cut_table"] is None) and (ld._lam_table is None) == (tabs["lam_table"] is None)
        ld.set_epoch(3)
        got[bs] = _epoch(ld)
        assert len(got[bs][0]) == n and int(ld.err.item()) == 0 and ld.epoch == 4
    # the partner of sample s is s - 1 except at a batch start: everywhere else neither x nor y depends on batch size
    inner = np.array([s for s in range(n) if s % 32 and s % 25])
    assert _same(got[32][0][inner], got[25][0][inner]) and np.array_equal(got[32][1][inner], got[25][1][inner])
    # every batch of the bs = 32 epoch (two full ones and the ragged 64..69) is the reference's
    for lo, hi in ((0, 32), (32, 64), (64, 70)):
        ids = np.arange(lo, hi)
        wx, wy = R.batch(data["img"], data["lbl"], ids, np.roll(ids, 1), data["mean"], data["std"], seed=4, epoch=3,
                         prob=mix.prob, switch=getattr(mix, "switch", 0.5), **tabs, **kw)
        assert _same(got[32][0][lo:hi], wx) and np.array_equal(got[32][1][lo:hi], wy), (lo, hi)
    a, b, wb = M.unpack(got[32][1])
    assert np.array_equal(a, data["lbl"][:n]) and (wb > 0).sum() > n // 2 and wb.max() <= 1
    # shuffled: the same samples with the same weights, whatever the order
    ld = _loader(data, gpu, n, batch_size=32, shuffle=True, seed=1, augment=aug, mix=mix)
    ld.set_epoch(3)
    state = ld.gen.get_state()
    order = ld.order().numpy()
    ld.gen.set_state(state)
    sa, _, swb = M.unpack(_epoch(ld)[1])
    assert np.array_equal(sa, data["lbl"][order]) and np.array_equal(swb, wb[order])


def test_loader_cutmix_default_keeps_its_launch(gpu, data):
    """CutMix() (alpha = 1) still is one slk_image_batch_mix launch with its bits; alpha = 1 through the table is not."""
    from splitcnn.cifar import Augment
    from splitcnn.loss import CutMix
    n = 40
    aug = Augment(pad=data["pad"], flip=True, seed=4)
    ld = _loader(data, gpu, n, batch_size=32, shuffle=False, augment=aug, mix=CutMix(prob=0.9))
    assert ld._cut_table is None and ld._lam_table is None
    ld.set_epoch(2)
    x, y = _epoch(ld)
    for lo, hi in ((0, 32), (32, 40)):
        ids = np.arange(lo, hi)
        mx, my = _mix(data, ids, np.roll(ids, 1), gpu, prob=0.9, pad=data["pad"], flip=True, seed=4, epoch=2)
        assert _same(x[lo:hi], mx) and np.array_equal(y[lo:hi], my)
        wx, wy = M.batch(data["img"], data["lbl"], ids, np.roll(ids, 1), data["mean"], data["std"], pad=data["pad"],
                         flip=True, seed=4, epoch=2, prob=0.9)
        assert _same(x[lo:hi], wx) and np.array_equal(y[lo:hi], wy)
    with pytest.raises(TypeError, match="MixUp"):
        _loader(data, gpu, n, mix=0.5)


# ------------------------------------------------------------------------------------ (g) into a trainer
def test_mixup_loader_batch_trains_the_wide_trainer(gpu):
    from splitcnn.cifar import Augment, CifarLoader
    from splitcnn.loss import MixUp, SoftCrossEntropy, lam_table
    from splitcnn.wide import WideTrainer, init_wide_models
    img, lbl = R.dataset("cifar")
    sh = R.SHAPES["cifar"]
    ld = CifarLoader(_Set(img[:B], lbl[:B]), batch_size=B, shuffle=False, device=gpu, augment=Augment(seed=6), mix=MixUp(0.4))
    (x, y), = list(ld)
    ids = np.arange(B)
    wx, wy = R.batch(img, lbl, ids, np.roll(ids, 1), sh["mean"], sh["std"], lam_table=lam_table(0.4), pad=4, flip=True,
                     seed=6, epoch=0)
    assert _same(x.cpu().numpy(), wx) and np.array_equal(y.cpu().numpy(), wy) and int((y >= 2 ** 32).sum()) > B // 2
    ux, uy = torch.from_numpy(wx).to(gpu), torch.from_numpy(wy).to(gpu)

    def step(xx, yy, **kw):
        tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=False, **kw)
        tr.step(xx, yy)
        torch.cuda.synchronize()
        return tr

    a, b = step(x, y, loss=SoftCrossEntropy(0.1)), step(ux, uy, loss=SoftCrossEntropy(0.1))
    a.server.check_labels()
    b.server.check_labels()
    assert torch.equal(a.client.params, b.client.params) and torch.equal(a.server.params, b.server.params)
    la, lb = [l for _, l in a.loss_log.flush()], [l for _, l in b.loss_log.flush()]
    assert la == lb and len(la) == 1 and np.isfinite(la[0])
    ref = step(x, y.clone().fill_(0), loss=SoftCrossEntropy(0.1))
    assert not torch.equal(ref.server.params, a.server.params), "the labels reach the step"
    with pytest.raises(IndexError, match=r"a label was out of range \[0, 10\).*malformed"):
        step(x, y).server.check_labels()
