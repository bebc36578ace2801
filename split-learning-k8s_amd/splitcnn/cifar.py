"""CIFAR-10 input path of the widened model (wide.WideTrainer), offline: the dataset files from a local
path, the u8 dataset resident in HBM (150 MB for the 50k training images), and each training batch one
`slk_image_batch` launch that gathers the shuffled rows and applies torchvision's usual CIFAR pipeline

    RandomCrop(32, padding=4) -> RandomHorizontalFlip() -> ToTensor() -> Normalize(CIFAR_MEAN, CIFAR_STD)

on the device. The crop offsets and the flip are not torch's random stream: they are a counter-based hash
of (dataset index, epoch, seed) (include/slk.h), the same distribution, so a sample's augmentation in an
epoch does not depend on batch size, shuffle order or the ragged last batch, and `augment_draws`
reproduces an epoch on the host.
"""
import io
import os
import pickle
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import ops
from .loss import draw_chain
from .mnist import ResidentLoader

CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2470, 0.2435, 0.2616)
RECORD = 1 + 3 * 32 * 32   # binary version: 1 label byte, then 1024 R, 1024 G, 1024 B

_BIN_DIR, _PY_DIR = "cifar-10-batches-bin", "cifar-10-batches-py"
_BIN_FILES = {True: [f"data_batch_{i}.bin" for i in range(1, 6)], False: ["test_batch.bin"]}
_PY_FILES = {True: [f"data_batch_{i}" for i in range(1, 6)], False: ["test_batch"]}


# ------------------------------------------------------------------------------------ file formats
def _check(images: np.ndarray, labels: np.ndarray, where: str):
    if images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (3, 32, 32):
        raise ValueError(f"{where}: images: expected u8 [N,3,32,32], got {images.dtype} {images.shape}")
    if labels.shape != (images.shape[0],):
        raise ValueError(f"{where}: labels: expected [{images.shape[0]}], got {labels.shape}")
    if labels.size and (int(labels.max()) > 9 or int(labels.min()) < 0):
        raise ValueError(f"{where}: labels must be in [0, 10)")


def read_cifar_bin(path: str):
    """(images u8 [N,3,32,32], labels u8 [N]) of one file of the CIFAR-10 binary version."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) % RECORD:
        raise ValueError(f"{path}: {len(raw)} bytes is not a multiple of the {RECORD}-byte record")
    rec = np.frombuffer(raw, dtype=np.uint8).reshape(-1, RECORD)
    images, labels = rec[:, 1:].reshape(-1, 3, 32, 32).copy(), rec[:, 0].copy()
    _check(images, labels, path)
    return images, labels


def write_cifar_bin(path: str, images: np.ndarray, labels: np.ndarray) -> None:
    """Write u8 images [N,3,32,32] and labels [N] as one file of the binary version — for fixtures and tests."""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    _check(images, labels, path)
    rec = np.concatenate([labels[:, None], images.reshape(len(images), -1)], axis=1)
    with open(path, "wb") as f:
        f.write(rec.tobytes())


def _latin1_encode(s, encoding="latin1"):
    # how a protocol-2 pickle written by Python 3 carries bytes (an array's data); no other codec is looked up
    if encoding.lower().replace("-", "").replace("_", "") != "latin1":
        raise pickle.UnpicklingError(f"refused to encode with {encoding!r}")
    return s.encode("latin1")


_ALLOWED = {("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "_reconstruct"),
            ("numpy._core.multiarray", "_reconstruct")}


class _ArrayUnpickler(pickle.Unpickler):
    """Unpickle only numpy arrays and builtin containers (what a CIFAR-10 python-version batch holds)."""

    def find_class(self, module, name):
        if (module, name) == ("_codecs", "encode"):
            return _latin1_encode
        if (module, name) in _ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refused to unpickle {module}.{name}")

    def persistent_load(self, pid):
        raise pickle.UnpicklingError("persistent ids are not accepted")


def read_cifar_py(path: str):
    """(images, labels) of one batch file of the python version (a pickled dict with 'data' u8 [N,3072] and
    'labels'), through the allow-listed unpickler: a pickle naming any other global raises."""
    with open(path, "rb") as f:
        d = _ArrayUnpickler(io.BytesIO(f.read()), encoding="latin1").load()
    if not isinstance(d, dict):
        raise ValueError(f"{path}: expected a pickled dict, got {type(d).__name__}")
    d = {(k.decode("latin1") if isinstance(k, bytes) else k): v for k, v in d.items()}
    if "data" not in d or "labels" not in d:
        raise ValueError(f"{path}: no 'data' / 'labels' entries")
    data, labels = np.asarray(d["data"]), np.asarray(d["labels"])
    if data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != 3072:
        raise ValueError(f"{path}: data: expected u8 [N,3072], got {data.dtype} {data.shape}")
    if labels.ndim != 1 or labels.dtype.kind not in "iu":
        raise ValueError(f"{path}: labels: expected integers [N], got {labels.dtype} {labels.shape}")
    images = np.ascontiguousarray(data.reshape(-1, 3, 32, 32))
    _check(images, labels, path)
    return images, labels.astype(np.uint8)


class CifarBin:
    """The CIFAR-10 split at `root`: the binary version (data_batch_1..5.bin / test_batch.bin under root or
    root/cifar-10-batches-bin) or, failing that, the python version torchvision leaves on disk
    (root/cifar-10-batches-py/data_batch_N, test_batch). images u8 [N,3,32,32], labels u8 [N]."""

    def __init__(self, root: str, train: bool = True):
        for d, names, read in ((root, _BIN_FILES, read_cifar_bin), (os.path.join(root, _BIN_DIR), _BIN_FILES, read_cifar_bin),
                               (os.path.join(root, _PY_DIR), _PY_FILES, read_cifar_py)):
            paths = [os.path.join(d, n) for n in names[train]]
            if os.path.exists(paths[0]):
                break
        else:
            raise FileNotFoundError(f"{_BIN_FILES[train][0]} not found under {root} (or its {_BIN_DIR}), nor "
                                    f"{_PY_FILES[train][0]} under its {_PY_DIR}")
        for p in paths:
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} is missing")
        parts = [read(p) for p in paths]
        self.images = np.concatenate([p[0] for p in parts])
        self.labels = np.concatenate([p[1] for p in parts])

    def __len__(self):
        return int(self.images.shape[0])


# ------------------------------------------------------------------------------------ augmentation
@dataclass(frozen=True)
class Augment:
    """RandomCrop(H, padding=pad) and, with `flip`, RandomHorizontalFlip(0.5); `seed` keys the draws."""
    pad: int = 4
    flip: bool = True
    seed: int = 0

    def __post_init__(self):
        if not 0 <= int(self.pad) <= 8:
            raise ValueError(f"Augment: pad must be in [0, 8], got {self.pad}")


def augment_draws(idx, epoch: int, seed: int, pad: int, flip: bool = True):
    """(dy, dx, flip) int64 arrays, the draws slk_image_batch makes for the dataset indices `idx` in `epoch`
    under `seed`: the host twin of the kernel's hash (include/slk.h), in uint32 / uint64 numpy arithmetic.
    The crop window of sample i starts at (dy - pad, dx - pad); dy, dx are in [0, 2 * pad]."""
    h0, h1, h2 = draw_chain(idx, epoch, seed, 3)
    span = np.uint64(2 * pad + 1)
    dy = (h0.astype(np.uint64) * span) >> np.uint64(32)
    dx = (h1.astype(np.uint64) * span) >> np.uint64(32)
    f = (h2 >> np.uint32(31)) if flip else np.zeros_like(h2)
    return dy.astype(np.int64), dx.astype(np.int64), f.astype(np.int64)


class CifarLoader(ResidentLoader):
    """ResidentLoader over CifarBin (any dataset with u8 `images` [N,3,32,32] and `labels` [N]): x f32
    [B,3,32,32] and y i64 [B] by one slk_image_batch launch per batch, eagerly, so every batch sees the
    loader's current `epoch`. `augment=None` (use it for the test split) is no crop and no flip: gather +
    ToTensor + Normalize(mean, std). `mix=CutMix(...)` (splitcnn.loss) pastes a box of the previous sample of the
    batch into each sample in the same launch (slk_image_batch_mix) and yields mixed labels; `mix=MixUp(...)` blends
    the two, `mix=Mix(...)` chooses per sample, and CutMix at another alpha draws from a Beta quantile table (all
    three one slk_image_batch_blend launch)."""

    sample_shape = (3, 32, 32)

    def __init__(self, dataset, batch_size: int = 64, shuffle: bool = True, seed: Optional[int] = None,
                 device="cuda", drop_last: bool = False, augment: Optional[Augment] = None, mean=CIFAR_MEAN,
                 std=CIFAR_STD, mix=None):
        super().__init__(dataset, batch_size, shuffle, seed, device, drop_last, augment, mix)
        self.mean, self.std = tuple(mean), tuple(std)

    def _batch(self, idx, x, y):
        if self.mix is not None:
            return self._mix_batch(idx, x, y, self.mean, self.std)
        return ops.image_batch(self.images, self.labels, idx, mean=self.mean, std=self.std, x=x, y=y,
                               err_flag=self.err, **self._augment_args())
