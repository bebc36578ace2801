"""GPU tests of the CIFAR-10 input path: slk_image_batch (both instantiations) bit for bit against the
independent numpy reference (tests/cifar_ref.py), its fallbacks and refusals, the loaders' invariance to
batch size and shuffle order, and WideTrainer trained from a CifarLoader against the same trainer fed the
reference's batches. Outputs are prefilled with NaN / -1 and carry one sentinel row behind the last; every
comparison is np.array_equal (the kernel's arithmetic is the reference's, IEEE division included)."""
import os

import numpy as np
import pytest
import torch

import cifar_ref

pytestmark = pytest.mark.gpu

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
M_MEAN, M_STD = (0.1307,), (0.3081,)


def _cifar_data():
    r = np.random.default_rng(11)
    img = r.integers(0, 256, size=(4096, 3, 32, 32), dtype=np.uint8)
    img[0] = 0
    img[1] = 255
    c, y, x = np.meshgrid(np.arange(3), np.arange(32), np.arange(32), indexing="ij")
    img[2] = ((c * 64 + y * 37 + x * 5) % 256).astype(np.uint8)      # the value says where the pixel came from
    return img, r.integers(0, 10, size=4096, dtype=np.uint8)


def _mnist_data():
    r = np.random.default_rng(12)
    img = r.integers(0, 256, size=(300, 28, 28), dtype=np.uint8)
    img[0] = 0
    img[1] = 255
    y, x = np.meshgrid(np.arange(28), np.arange(28), indexing="ij")
    img[2] = ((y * 37 + x * 5) % 256).astype(np.uint8)
    return img, r.integers(0, 10, size=300, dtype=np.uint8)


@pytest.fixture(scope="module")
def cifar(gpu):
    img, lbl = _cifar_data()
    return {"img": img, "lbl": lbl, "dimg": torch.from_numpy(img).to(gpu), "dlbl": torch.from_numpy(lbl).to(gpu),
            "mean": MEAN, "std": STD}


@pytest.fixture(scope="module")
def mnist(gpu):
    img, lbl = _mnist_data()
    return {"img": img, "lbl": lbl, "dimg": torch.from_numpy(img).to(gpu), "dlbl": torch.from_numpy(lbl).to(gpu),
            "mean": M_MEAN, "std": M_STD}


def _run(d, idx, gpu, **kw):
    """ops.image_batch into NaN / -1 prefilled buffers with a sentinel row; returns numpy (x, y, err)."""
    from splitcnn import ops
    B = len(idx)
    shape = tuple(d["dimg"].shape[1:]) if d["dimg"].dim() == 4 else (1,) + tuple(d["dimg"].shape[1:])
    xf = torch.full((B + 1,) + shape, float("nan"), dtype=torch.float32, device=gpu)
    yf = torch.full((B + 1,), -1, dtype=torch.int64, device=gpu)
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    x, y = ops.image_batch(d["dimg"], d["dlbl"], torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(gpu),
                           mean=d["mean"], std=d["std"], x=xf[:B], y=yf[:B], err_flag=err, **kw)
    torch.cuda.synchronize()
    assert x.data_ptr() == xf.data_ptr() and y.data_ptr() == yf.data_ptr()
    assert bool(torch.isnan(xf[B]).all()) and int(yf[B]) == -1, "wrote behind the last row"
    return xf[:B].cpu().numpy(), yf[:B].cpu().numpy(), int(err.item())


def _check(d, idx, gpu, **kw):
    x, y, err = _run(d, idx, gpu, **kw)
    wx, wy = cifar_ref.batch(d["img"], d["lbl"], idx, d["mean"], d["std"], **kw)
    assert err == 0
    assert x.dtype == np.float32 and not np.isnan(x).any()
    assert np.array_equal(x, wx)
    assert np.array_equal(y, wy)
    return x


# ------------------------------------------------------------------------------------ the kernel
def test_image_batch_cifar_every_draw(gpu, cifar):
    """idx = 0..4095 at seed 0, epoch 0, pad 4, flip on: all 162 (dy, dx, flip) combinations occur
    (tests/test_cifar_cpu.py::test_augment_draws_cover_every_combination)."""
    x = _check(cifar, np.arange(4096), gpu, pad=4, flip=True, seed=0, epoch=0)
    dy, dx, fl = cifar_ref.draws(np.arange(3), 0, 0, 4)
    padv = ((np.float32(0) / np.float32(255) - np.float32(MEAN)) / np.float32(STD)).astype(np.float32)
    assert np.array_equal(x[0], np.broadcast_to(padv[:, None, None], (3, 32, 32)))     # all-zero image
    if dy[1] != 4 or dx[1] != 4:                                                        # all-255: the border shows
        assert (x[1] == padv[:, None, None]).any() and (x[1] != padv[:, None, None]).any()


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("epoch", [0, 3])
def test_image_batch_cifar_shuffled(gpu, cifar, B, epoch):
    idx = np.random.default_rng(100 + B).permutation(np.arange(1, 4095))[:max(B - 2, 0)]
    idx = np.concatenate([[4095], idx, [0]])[:B] if B > 1 else np.array([4095])
    _check(cifar, idx, gpu, pad=4, flip=True, seed=0, epoch=epoch)
    if B == 1:
        _check(cifar, np.array([0]), gpu, pad=4, flip=True, seed=0, epoch=epoch)


def test_image_batch_mnist_every_draw(gpu, mnist):
    """<1,28,28>, pad 2, flip off, idx = 0..299: all 25 (dy, dx) pairs occur."""
    _check(mnist, np.arange(300), gpu, pad=2, flip=False, seed=0, epoch=0)


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("epoch", [0, 3])
def test_image_batch_mnist_shuffled(gpu, mnist, B, epoch):
    idx = np.random.default_rng(200 + B).permutation(np.arange(1, 299))[:max(B - 2, 0)]
    idx = np.concatenate([[299], idx, [0]])[:B] if B > 1 else np.array([299])
    _check(mnist, idx, gpu, pad=2, flip=False, seed=0, epoch=epoch)
    if B == 1:
        _check(mnist, np.array([0]), gpu, pad=2, flip=False, seed=0, epoch=epoch)


@pytest.mark.parametrize("which", ["cifar", "mnist"])
def test_image_batch_widest_pad_flip_and_other_seeds(gpu, cifar, mnist, which):
    """pad 8 (quads that lie wholly beside the image), flip on for both shapes, seeds / epochs other than 0,
    repeated indices, and the first and last image of the dataset (the word clamp at both ends)."""
    d = cifar if which == "cifar" else mnist
    n = len(d["img"])
    idx = np.concatenate([[0, n - 1, n - 1, 0, 2, 2], np.random.default_rng(5).integers(0, n, size=70)])
    _check(d, idx, gpu, pad=8, flip=True, seed=7, epoch=1)
    _check(d, idx, gpu, pad=1, flip=True, seed=1, epoch=2)
    _check(d, idx, gpu, pad=0, flip=True, seed=3, epoch=0)
    _check(d, idx, gpu, pad=3, flip=False, seed=0xFFFFFFFF, epoch=0x80000001)


def test_image_batch_mnist_pad0_is_mnist_batch(gpu, mnist):
    from splitcnn import ops
    idx = np.random.default_rng(6).permutation(300)
    x = _check(mnist, idx, gpu, pad=0, flip=False)
    mx, my = ops.mnist_batch(mnist["dimg"], mnist["dlbl"], torch.from_numpy(idx).to(gpu))
    assert np.array_equal(x.view(np.int32), mx.cpu().numpy().view(np.int32))
    assert np.array_equal(my.cpu().numpy(), mnist["lbl"][idx].astype(np.int64))


def test_image_batch_fallback_and_refusals(gpu, cifar):
    from splitcnn import _lib, ops
    idx = np.array([5, -1, 4095, 4096, 5, 0, 2 ** 40], dtype=np.int64)
    src = np.array([5, 0, 4095, 0, 5, 0, 0])
    for kw in (dict(pad=4, flip=True, seed=0, epoch=2), dict(pad=0, flip=False)):
        x, y, err = _run(cifar, idx, gpu, **kw)
        wx, wy = cifar_ref.batch(cifar["img"], cifar["lbl"], src, MEAN, STD, **kw)
        assert err == 1
        assert np.array_equal(x, wx) and np.array_equal(y, wy)        # image 0's row, with image 0's draws
        assert _run(cifar, src, gpu, **kw)[2] == 0
    # shapes and pads the library does not serve: invalid argument, nothing launched (the buffers keep their NaN)
    bad = torch.zeros((8, 3, 28, 28), dtype=torch.uint8, device=gpu)
    lbl = torch.zeros(8, dtype=torch.uint8, device=gpu)
    ids = torch.zeros(4, dtype=torch.int64, device=gpu)
    out = torch.full((4, 3, 28, 28), float("nan"), device=gpu)
    with pytest.raises(_lib.SLKError, match="invalid argument"):
        ops.image_batch(bad, lbl, ids, mean=MEAN, std=STD, x=out)
    for pad in (-1, 9):
        out2 = torch.full((4, 3, 32, 32), float("nan"), device=gpu)
        with pytest.raises(_lib.SLKError, match="invalid argument"):
            ops.image_batch(cifar["dimg"], cifar["dlbl"], ids, mean=MEAN, std=STD, pad=pad, x=out2)
        assert bool(torch.isnan(out2).all())
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.SLKError, match="invalid argument"):       # misaligned dataset base
        _lib.call("slk_image_batch", cifar["dimg"].data_ptr() + 1, cifar["dlbl"].data_ptr(), 8, 3, 32, 32,
                  ids.data_ptr(), 4, _floats(MEAN), _floats(STD), 0, 0, 0, 0, out2.data_ptr(),
                  torch.empty(4, dtype=torch.int64, device=gpu).data_ptr(), None, None)
    x, y = ops.image_batch(cifar["dimg"], cifar["dlbl"], ids[:0], mean=MEAN, std=STD)    # B == 0
    assert tuple(x.shape) == (0, 3, 32, 32) and tuple(y.shape) == (0,)


def _floats(v):
    import ctypes
    return (ctypes.c_float * len(v))(*v)


# ------------------------------------------------------------------------------------ the loaders
def _write_cifar(root, img, lbl):
    from splitcnn.cifar import write_cifar_bin
    cuts = np.linspace(0, len(img), 6).astype(int)
    for k in range(5):
        write_cifar_bin(os.path.join(root, f"data_batch_{k + 1}.bin"), img[cuts[k]:cuts[k + 1]], lbl[cuts[k]:cuts[k + 1]])
    write_cifar_bin(os.path.join(root, "test_batch.bin"), img, lbl)


def _epoch_by_index(ld, n, shape):
    """One pass of a loader, scattered back by dataset index; the order is recovered from a replayed generator."""
    state = ld.gen.get_state()
    order = ld.order().numpy()
    ld.gen.set_state(state)
    X = np.full((n,) + shape, np.nan, dtype=np.float32)
    Y = np.full(n, -1, dtype=np.int64)
    pos = 0
    for x, y in ld:
        b = x.shape[0]
        X[order[pos:pos + b]] = x.cpu().numpy()
        Y[order[pos:pos + b]] = y.cpu().numpy()
        pos += b
    assert pos == n and int(ld.err.item()) == 0
    return X, Y


def test_cifar_loader_invariant_to_batch_size_and_order(gpu, tmp_path):
    from splitcnn.cifar import Augment, CifarBin, CifarLoader
    img, lbl = _cifar_data()
    img, lbl = img[:150], lbl[:150]
    _write_cifar(str(tmp_path), img, lbl)
    ds = CifarBin(str(tmp_path))
    a = CifarLoader(ds, batch_size=64, seed=1, device=gpu, augment=Augment())
    b = CifarLoader(ds, batch_size=50, seed=2, device=gpu, augment=Augment())
    assert [tuple(x.shape) for x, _ in a] == [(64, 3, 32, 32), (64, 3, 32, 32), (22, 3, 32, 32)] and a.epoch == 1
    a.set_epoch(0)
    xa0, ya0 = _epoch_by_index(a, 150, (3, 32, 32))
    xb0, yb0 = _epoch_by_index(b, 150, (3, 32, 32))
    want, wy = cifar_ref.batch(img, lbl, np.arange(150), MEAN, STD, pad=4, flip=True, seed=0, epoch=0)
    assert np.array_equal(xa0, want) and np.array_equal(ya0, wy)
    assert np.array_equal(xb0, xa0) and np.array_equal(yb0, ya0)      # same (seed, epoch): same image per index
    assert a.epoch == 1 and b.epoch == 1
    xa1, _ = _epoch_by_index(a, 150, (3, 32, 32))                      # the next epoch draws again
    xb1, _ = _epoch_by_index(b, 150, (3, 32, 32))
    assert np.array_equal(xa1, xb1)
    assert np.array_equal(xa1, cifar_ref.batch(img, lbl, np.arange(150), MEAN, STD, pad=4, flip=True, epoch=1)[0])
    differs = [not np.array_equal(xa0[i], xa1[i]) for i in range(2, 150)]     # images 0 and 1 are constant
    assert sum(differs) > 0.9 * len(differs)
    a.set_epoch(0)
    assert np.array_equal(_epoch_by_index(a, 150, (3, 32, 32))[0], xa0)
    # another Augment seed is another stream
    c = CifarLoader(ds, batch_size=150, shuffle=False, device=gpu, augment=Augment(seed=9))
    (xc, _), = list(c)
    assert np.array_equal(xc.cpu().numpy(), cifar_ref.batch(img, lbl, np.arange(150), MEAN, STD, pad=4, flip=True, seed=9)[0])


def test_cifar_loader_without_augment_is_plain_normalise(gpu, tmp_path):
    from splitcnn.cifar import CifarBin, CifarLoader
    img, lbl = _cifar_data()
    img, lbl = img[:150], lbl[:150]
    _write_cifar(str(tmp_path), img, lbl)
    ld = CifarLoader(CifarBin(str(tmp_path), train=False), batch_size=64, shuffle=False, device=gpu)
    want = cifar_ref.normalize(img, MEAN, STD)
    for _ in range(2):                                                  # the epoch plays no part
        got = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in ld]
        assert [g[0].shape[0] for g in got] == [64, 64, 22]
        assert np.array_equal(np.concatenate([g[0] for g in got]), want)
        assert np.array_equal(np.concatenate([g[1] for g in got]), lbl.astype(np.int64))
    ld2 = CifarLoader(CifarBin(str(tmp_path), train=False), batch_size=64, shuffle=False, device=gpu,
                      mean=(0.5, 0.5, 0.5), std=(0.25, 0.5, 1.0))
    x, _ = next(iter(ld2))
    assert np.array_equal(x.cpu().numpy(), cifar_ref.normalize(img[:64], (0.5, 0.5, 0.5), (0.25, 0.5, 1.0)))


def test_device_loader_augment_routes_mnist_through_image_batch(gpu, tmp_path):
    from splitcnn import ops
    from splitcnn.cifar import Augment
    from splitcnn.mnist import DeviceLoader, MnistIDX, write_idx
    img, lbl = _mnist_data()
    write_idx(os.path.join(str(tmp_path), "train-images-idx3-ubyte"), img)
    write_idx(os.path.join(str(tmp_path), "train-labels-idx1-ubyte"), lbl)
    ds = MnistIDX(str(tmp_path))
    ld = DeviceLoader(ds, batch_size=64, seed=3, device=gpu, augment=Augment(pad=2, flip=False))
    for epoch in range(2):
        assert ld.epoch == epoch
        x, y = _epoch_by_index(ld, 300, (1, 28, 28))
        wx, wy = cifar_ref.batch(img, lbl, np.arange(300), M_MEAN, M_STD, pad=2, flip=False, seed=0, epoch=epoch)
        assert np.array_equal(x, wx) and np.array_equal(y, wy)
    # augment=None, the default: today's batches, bitwise slk_mnist_batch
    plain = DeviceLoader(ds, batch_size=64, seed=3, device=gpu)
    state = plain.gen.get_state()
    order = plain.order()
    plain.gen.set_state(state)
    got = [(x.clone(), y.clone()) for x, y in plain]
    assert [g[0].shape[0] for g in got] == [64, 64, 64, 64, 44]
    mx, my = ops.mnist_batch(plain.images, plain.labels, order.to(gpu))
    assert torch.equal(torch.cat([g[0] for g in got]).view(torch.int32), mx.view(torch.int32))
    assert torch.equal(torch.cat([g[1] for g in got]), my)


# ------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("graph", [True, False])
def test_wide_trainer_from_cifar_loader_equals_reference_batches(gpu, tmp_path, graph):
    """Two epochs (batches 64 / 64 / 22) from a CifarLoader with Augment() against the same trainer fed the
    reference's batches from numpy: parameters and losses bit for bit. With graph=True the loader's two buffer
    pairs get graphs of their own from their second sighting on."""
    from splitcnn.cifar import Augment, CifarBin, CifarLoader
    from splitcnn.wide import WideTrainer, init_wide_models
    img, lbl = _cifar_data()
    img, lbl = img[:150], lbl[:150]
    _write_cifar(str(tmp_path), img, lbl)
    ds = CifarBin(str(tmp_path))
    ld = CifarLoader(ds, batch_size=64, seed=4, device=gpu, augment=Augment())
    twin = CifarLoader(ds, batch_size=64, seed=4, device="cpu")          # the same permutations, on the host
    tr = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph)
    ref = WideTrainer(*init_wide_models(seed=0), device=gpu, graph=graph)
    sizes = []
    for epoch in range(2):
        order = twin.order().numpy()
        assert ld.epoch == epoch
        for k, (x, y) in enumerate(ld):
            tr.step(x, y)
            idx = order[64 * k:64 * (k + 1)]
            wx, wy = cifar_ref.batch(img, lbl, idx, MEAN, STD, pad=4, flip=True, seed=0, epoch=epoch)
            ref.step(torch.from_numpy(wx).to(gpu), torch.from_numpy(wy).to(gpu))
            sizes.append(x.shape[0])
    torch.cuda.synchronize()
    assert sizes == [64, 64, 22] * 2 and int(ld.err.item()) == 0
    assert torch.equal(tr.client.params.view(torch.int32), ref.client.params.view(torch.int32))
    assert torch.equal(tr.server.params.view(torch.int32), ref.server.params.view(torch.int32))
    la, lb = tr.loss_log.flush(), ref.loss_log.flush()
    assert len(la) == 6 and la == lb and all(np.isfinite(v) for _, v in la)
    if graph:   # the loader's 64-row ring replays graphs captured on its own buffers
        assert tr._n_caller_graphs(64) == 2

    res = tr.evaluate(CifarLoader(ds, 64, shuffle=False, device=gpu))
    assert res.n == 150 and int(res.confusion.sum()) == 150 and res.bad_labels == 0
    pred = tr.predict(torch.from_numpy(cifar_ref.normalize(img, MEAN, STD)).to(gpu)).cpu().numpy()
    assert res.correct == int((pred == lbl.astype(np.int64)).sum())
    assert res.accuracy == float(np.mean(pred == lbl.astype(np.int64)))
