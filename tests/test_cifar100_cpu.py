"""cifar.Cifar100Bin on both on-disk versions of CIFAR-100: the binary records and the python version's pickled dict
(through the allow-listed unpickler), fine and coarse labels, and the label bounds."""
import os
import pickle

import numpy as np
import pytest


@pytest.mark.parametrize("version", ["binary", "python"])
def test_cifar100_versions_and_label_kinds(tmp_path, version):
    from splitcnn.cifar import Cifar100Bin, write_cifar100_bin
    rng = np.random.default_rng(1)
    images = rng.integers(0, 256, (12, 3, 32, 32), dtype=np.uint8)
    fine = rng.integers(0, 100, 12)
    fine[0], fine[1] = 99, 0
    if version == "binary":
        write_cifar100_bin(str(tmp_path / "train.bin"), images, fine, fine // 5)
    else:
        os.makedirs(tmp_path / "cifar-100-python")
        with open(tmp_path / "cifar-100-python" / "train", "wb") as f:
            pickle.dump({b"data": images.reshape(12, -1), b"fine_labels": [int(v) for v in fine],
                         b"coarse_labels": [int(v) for v in fine // 5]}, f, protocol=2)
    for kind, want, ncls in (("fine", fine, 100), ("coarse", fine // 5, 20)):
        ds = Cifar100Bin(str(tmp_path), train=True, labels=kind)
        assert ds.num_classes == ncls and len(ds) == 12 and ds.labels.dtype == np.uint8
        assert np.array_equal(ds.images, images) and np.array_equal(ds.labels, want)
    with pytest.raises(ValueError, match="'fine'"):
        Cifar100Bin(str(tmp_path), labels="both")
    with pytest.raises(FileNotFoundError):
        Cifar100Bin(str(tmp_path), train=False)
    with pytest.raises(ValueError, match=r"\[0, 20\)"):
        write_cifar100_bin(str(tmp_path / "bad.bin"), images, fine, fine // 5 + 1)
