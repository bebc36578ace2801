"""CIFAR-10 input path, the parts that need no GPU: the two on-disk formats (synthetic files written in the
real formats: no CIFAR-10 exists offline), the allow-listed unpickler, the host twin of the augmentation
draws against the independent reference (tests/cifar_ref.py), the reference itself against oracle/mnist.py
and hand-made images, and the loader contract."""
import os
import pickle

import numpy as np
import pytest
import torch

import cifar_ref

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)


def _synthetic(n, seed=0):
    r = np.random.default_rng(seed)
    img = r.integers(0, 256, size=(n, 3, 32, 32), dtype=np.uint8)
    return img, r.integers(0, 10, size=n, dtype=np.uint8)


def _write_bin(d, img, lbl, train=True):
    from splitcnn.cifar import write_cifar_bin
    os.makedirs(d, exist_ok=True)
    if not train:
        write_cifar_bin(os.path.join(d, "test_batch.bin"), img, lbl)
        return
    cuts = np.linspace(0, len(img), 6).astype(int)
    for k in range(5):
        write_cifar_bin(os.path.join(d, f"data_batch_{k + 1}.bin"), img[cuts[k]:cuts[k + 1]], lbl[cuts[k]:cuts[k + 1]])


# ------------------------------------------------------------------------------------ file formats
@pytest.mark.parametrize("sub", ["", "cifar-10-batches-bin"])
def test_binary_roundtrip_both_layouts(tmp_path, sub):
    from splitcnn.cifar import RECORD, CifarBin
    img, lbl = _synthetic(37)
    d = os.path.join(str(tmp_path), sub)
    _write_bin(d, img, lbl)
    _write_bin(d, img[:7], lbl[:7], train=False)
    ds = CifarBin(str(tmp_path), train=True)
    assert len(ds) == 37 and np.array_equal(ds.images, img) and np.array_equal(ds.labels, lbl)
    assert ds.images.dtype == np.uint8 and ds.labels.dtype == np.uint8
    te = CifarBin(str(tmp_path), train=False)
    assert len(te) == 7 and np.array_equal(te.images, img[:7]) and np.array_equal(te.labels, lbl[:7])
    # the record layout of the real files: label, 1024 R, 1024 G, 1024 B
    raw = open(os.path.join(d, "test_batch.bin"), "rb").read()
    assert RECORD == 3073 and len(raw) == 7 * 3073 and raw[3073] == lbl[1]
    assert raw[3073 + 1:3073 + 1025] == img[1, 0].tobytes() and raw[3073 + 2049:2 * 3073] == img[1, 2].tobytes()


def _write_py(d, img, lbl, train=True, byte_keys=True):
    os.makedirs(d, exist_ok=True)
    names = [f"data_batch_{k + 1}" for k in range(5)] if train else ["test_batch"]
    cuts = np.linspace(0, len(img), len(names) + 1).astype(int)
    for k, name in enumerate(names):
        a, b = cuts[k], cuts[k + 1]
        key = (lambda s: s.encode()) if byte_keys else (lambda s: s)
        rec = {key("batch_label"): "training batch", key("labels"): [int(v) for v in lbl[a:b]],
               key("data"): img[a:b].reshape(b - a, 3072), key("filenames"): [f"img_{i}.png" for i in range(a, b)]}
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump(rec, f, protocol=2)


@pytest.mark.parametrize("byte_keys", [True, False])
def test_python_format_roundtrip(tmp_path, byte_keys):
    from splitcnn.cifar import CifarBin
    img, lbl = _synthetic(23, seed=1)
    d = os.path.join(str(tmp_path), "cifar-10-batches-py")
    _write_py(d, img, lbl, byte_keys=byte_keys)
    _write_py(d, img[:5], lbl[:5], train=False, byte_keys=byte_keys)
    ds = CifarBin(str(tmp_path), train=True)
    assert len(ds) == 23 and np.array_equal(ds.images, img) and np.array_equal(ds.labels, lbl)
    assert ds.images.dtype == np.uint8 and ds.labels.dtype == np.uint8
    te = CifarBin(str(tmp_path), train=False)
    assert np.array_equal(te.images, img[:5]) and np.array_equal(te.labels, lbl[:5])


class _Evil:
    def __init__(self, path):
        self.path = path

    def __reduce__(self):
        return (os.system, (f"touch {self.path}",))


def test_pickle_naming_another_global_is_refused_without_running(tmp_path):
    from splitcnn.cifar import CifarBin, read_cifar_py
    d = tmp_path / "cifar-10-batches-py"
    d.mkdir()
    marker = tmp_path / "executed"
    (d / "test_batch").write_bytes(pickle.dumps({"data": _Evil(str(marker)), "labels": [0]}, protocol=2))
    with pytest.raises(pickle.UnpicklingError, match="refused to unpickle"):
        read_cifar_py(str(d / "test_batch"))
    with pytest.raises(pickle.UnpicklingError, match="refused to unpickle"):
        CifarBin(str(tmp_path), train=False)
    assert not marker.exists()
    # a codec other than the one protocol-2 bytes travel in is not looked up either
    (d / "test_batch").write_bytes(b"\x80\x02c_codecs\nencode\nX\x01\x00\x00\x00aX\x05\x00\x00\x00rot13\x86R.")
    with pytest.raises(pickle.UnpicklingError, match="refused to encode"):
        read_cifar_py(str(d / "test_batch"))


def test_bad_files_raise_as_specified(tmp_path):
    from splitcnn.cifar import CifarBin, read_cifar_bin, write_cifar_bin
    img, lbl = _synthetic(10, seed=2)
    with pytest.raises(FileNotFoundError):
        CifarBin(str(tmp_path), train=True)                # nothing there
    _write_bin(str(tmp_path), img, lbl)
    with pytest.raises(FileNotFoundError):
        CifarBin(str(tmp_path), train=False)               # the other split is missing
    os.remove(os.path.join(str(tmp_path), "data_batch_3.bin"))
    with pytest.raises(FileNotFoundError, match="data_batch_3"):
        CifarBin(str(tmp_path), train=True)                # one of the five is missing
    p = os.path.join(str(tmp_path), "test_batch.bin")
    write_cifar_bin(p, img, lbl)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:-5])                          # truncated
    with pytest.raises(ValueError, match="multiple"):
        read_cifar_bin(p)
    with pytest.raises(ValueError, match="multiple"):
        CifarBin(str(tmp_path), train=False)
    bad = bytearray(raw)
    bad[2 * 3073] = 10                                     # a label > 9
    open(p, "wb").write(bytes(bad))
    with pytest.raises(ValueError, match="labels"):
        CifarBin(str(tmp_path), train=False)
    with pytest.raises(ValueError, match="labels"):
        write_cifar_bin(p, img, np.full(10, 11, dtype=np.uint8))
    with pytest.raises(ValueError, match="images"):
        write_cifar_bin(p, img[:, :, :28, :28], lbl)
    # python version: wrong shapes and labels
    d = os.path.join(str(tmp_path), "py", "cifar-10-batches-py")
    os.makedirs(d)
    for rec, what in (({"data": img.reshape(10, 3072)[:, :3000], "labels": list(map(int, lbl))}, "data"),
                      ({"data": img.reshape(10, 3072), "labels": list(map(int, lbl[:9]))}, "labels"),
                      ({"data": img.reshape(10, 3072), "labels": [10] * 10}, "labels"),
                      ({"data": img.reshape(10, 3072)}, "labels")):
        with open(os.path.join(d, "test_batch"), "wb") as f:
            pickle.dump(rec, f, protocol=2)
        with pytest.raises(ValueError, match=what):
            CifarBin(os.path.join(str(tmp_path), "py"), train=False)


# ------------------------------------------------------------------------------------ the entry point
def test_image_batch_argument_validation_without_gpu():
    import ctypes
    from splitcnn import _lib, ops
    lib = _lib.load()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def call(C, H, W, B, pad, images=None):
        return lib.slk_image_batch(images, None, 10, C, H, W, None, B, f3, f3, pad, 1, 0, 0, None, None, None, None)

    assert call(3, 32, 32, 0, 4) == 0 and call(1, 28, 28, 0, 0) == 0       # empty batch: no launch
    assert call(3, 28, 28, 0, 4) == 1 and call(1, 32, 32, 0, 0) == 1       # hipErrorInvalidValue: other shapes
    assert call(3, 32, 32, 0, -1) == 1 and call(3, 32, 32, 0, 9) == 1 and call(3, 32, 32, 0, 8) == 0
    assert call(3, 32, 32, -1, 4) == 1
    assert call(3, 32, 32, 4, 4) == 1                                      # null buffers
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_batch(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                        torch.zeros(2, dtype=torch.int64), mean=(0.5,) * 3, std=(0.5,) * 3)
    with pytest.raises(ValueError, match="mean / std"):
        ops.image_batch(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                        torch.zeros(2, dtype=torch.int64), mean=(0.5,), std=(0.5,))


# ------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("epoch", [0, 1, 3])
def test_augment_draws_equal_reference(seed, epoch):
    from splitcnn.cifar import augment_draws
    idx = np.arange(4096)
    for pad, flip in ((4, True), (2, False), (0, True), (8, True)):
        got = augment_draws(idx, epoch, seed, pad, flip)
        want = cifar_ref.draws(idx, epoch, seed, pad, flip)
        for g, w in zip(got, want):
            assert g.shape == (4096,) and np.array_equal(g, w), (pad, flip)


def test_augment_draws_cover_every_combination():
    """Conditions on the chosen inputs (the GPU tests rely on them to exercise every offset)."""
    from splitcnn.cifar import augment_draws
    dy, dx, fl = augment_draws(np.arange(4096), 0, 0, 4)
    assert dy.min() == 0 and dy.max() == 8 and dx.min() == 0 and dx.max() == 8
    assert len(set(zip(dy.tolist(), dx.tolist(), fl.tolist()))) == 9 * 9 * 2
    dy, dx, fl = augment_draws(np.arange(300), 0, 0, 2, flip=False)
    assert not fl.any() and len(set(zip(dy.tolist(), dx.tolist()))) == 25
    # two epochs draw independently: the full triple agrees for about 1 / 162 of the samples
    a, b = augment_draws(np.arange(4096), 0, 0, 4), augment_draws(np.arange(4096), 1, 0, 4)
    same = (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2])
    assert same.mean() < 0.03
    # keyed on the dataset index alone: any subset, any order
    sub = np.array([4095, 17, 0, 2048])
    for full, part in zip(a, augment_draws(sub, 0, 0, 4)):
        assert np.array_equal(full[sub], part)


# ------------------------------------------------------------------------------------ the reference itself
def test_reference_without_augmentation_is_the_mnist_oracle():
    from oracle.mnist import MEAN as M, STD as S, transform
    img = np.random.default_rng(3).integers(0, 256, size=(40, 28, 28), dtype=np.uint8)
    lbl = np.arange(40, dtype=np.uint8) % 10
    idx = np.random.default_rng(4).permutation(40)
    x, y = cifar_ref.batch(img, lbl, idx, (float(M),), (float(S),))
    assert x.dtype == np.float32 and np.array_equal(x, transform(img[idx]))
    assert y.dtype == np.int64 and np.array_equal(y, lbl[idx])


def test_reference_places_corners_and_padding():
    img = np.full((3, 32, 32), 100, dtype=np.uint8)
    corners = {(0, 0): 11, (0, 31): 22, (31, 0): 33, (31, 31): 44}
    for (r, c), v in corners.items():
        img[:, r, c] = v
    mean32, std32 = np.float32(MEAN), np.float32(STD)

    def val(p):
        return ((np.float32(p) / np.float32(255) - mean32) / std32).astype(np.float32)

    for dy, dx, flip in [(0, 0, 0), (4, 4, 0), (4, 4, 1), (8, 8, 0), (8, 0, 1), (1, 6, 1), (7, 2, 0)]:
        out = cifar_ref.normalize(cifar_ref.crop_flip(img, dy, dx, flip, 4), MEAN, STD)
        assert out.shape == (3, 32, 32) and out.dtype == np.float32
        want = np.empty((3, 32, 32), dtype=np.float32)
        want[:] = val(0)[:, None, None]                       # the padding: (0 - mean) / std, not 0
        # source pixel (r, c) sits at padded (r + 4, c + 4), so at window (r + 4 - dy, c + 4 - dx)
        for r in range(32):
            for c in range(32):
                yo, xo = r + 4 - dy, c + 4 - dx
                if 0 <= yo < 32 and 0 <= xo < 32:
                    want[:, yo, 31 - xo if flip else xo] = val(img[0, r, c])
        assert np.array_equal(out, want), (dy, dx, flip)
        for (r, c), v in corners.items():
            yo, xo = r + 4 - dy, c + 4 - dx
            if 0 <= yo < 32 and 0 <= xo < 32:
                assert np.array_equal(out[:, yo, 31 - xo if flip else xo], val(v)), (dy, dx, flip, r, c)
    # the documented formula xs = (flip ? W-1-xo : xo) + dx - pad, ys = yo + dy - pad, on a random image
    rnd = np.random.default_rng(5).integers(0, 256, size=(3, 32, 32), dtype=np.uint8)
    for dy, dx, flip in [(0, 8, 1), (5, 3, 0), (8, 8, 1)]:
        out = cifar_ref.crop_flip(rnd, dy, dx, flip, 4)
        for yo, xo in [(0, 0), (0, 31), (31, 0), (31, 31), (13, 7), (4, 27)]:
            xs, ys = (31 - xo if flip else xo) + dx - 4, yo + dy - 4
            p = rnd[:, ys, xs] if 0 <= xs < 32 and 0 <= ys < 32 else 0
            assert np.array_equal(out[:, yo, xo], np.broadcast_to(p, 3))
    assert np.array_equal(cifar_ref.normalize(np.zeros((3, 2, 2), np.uint8), MEAN, STD)[:, 0, 0], -mean32 / std32)


# ------------------------------------------------------------------------------------ the loader contract
def test_loader_batches_like_reference_dataloader(tmp_path):
    from splitcnn.cifar import CIFAR_MEAN, CIFAR_STD, Augment, CifarBin, CifarLoader
    assert CIFAR_MEAN == MEAN and CIFAR_STD == STD
    img, lbl = _synthetic(150)
    _write_bin(str(tmp_path), img, lbl)
    ds = CifarBin(str(tmp_path))
    ld = CifarLoader(ds, batch_size=64, seed=5, device="cpu", augment=Augment())
    assert len(ld) == 3                                    # 64, 64, 22 (drop_last=False)
    o1 = ld.order()
    assert sorted(o1.tolist()) == list(range(150))
    assert not torch.equal(ld.order(), o1)                 # the generator moves on: another permutation
    ld2 = CifarLoader(ds, batch_size=64, seed=5, device="cpu")
    assert torch.equal(ld2.order(), o1)
    assert not torch.equal(CifarLoader(ds, batch_size=64, seed=6, device="cpu").order(), o1)
    assert torch.equal(CifarLoader(ds, batch_size=64, shuffle=False, device="cpu").order(), torch.arange(150))
    assert len(CifarLoader(ds, batch_size=64, device="cpu", drop_last=True)) == 2
    assert len(CifarLoader(ds, batch_size=50, device="cpu")) == 3 and len(CifarLoader(ds, batch_size=150, device="cpu")) == 1
    assert ld.epoch == 0 and ld2.augment is None and ld.augment == Augment(pad=4, flip=True, seed=0)
    ld.set_epoch(7)
    assert ld.epoch == 7
    assert ld.images.dtype == torch.uint8 and tuple(ld.images.shape) == (150, 3, 32, 32)
    assert ld.err.dtype == torch.int32 and int(ld.err) == 0
    with pytest.raises(ValueError, match="pad"):
        Augment(pad=9)


def test_device_loader_accepts_augment_without_gpu(tmp_path):
    from splitcnn.cifar import Augment
    from splitcnn.mnist import DeviceLoader, MnistIDX, write_idx
    r = np.random.default_rng(0)
    write_idx(os.path.join(str(tmp_path), "train-images-idx3-ubyte"), r.integers(0, 256, size=(10, 28, 28), dtype=np.uint8))
    write_idx(os.path.join(str(tmp_path), "train-labels-idx1-ubyte"), r.integers(0, 10, size=10, dtype=np.uint8))
    ld = DeviceLoader(MnistIDX(str(tmp_path)), batch_size=4, device="cpu", augment=Augment(pad=2, flip=False))
    assert len(ld) == 3 and ld.augment.pad == 2 and ld.epoch == 0
    assert DeviceLoader(MnistIDX(str(tmp_path)), batch_size=4, device="cpu").augment is None
