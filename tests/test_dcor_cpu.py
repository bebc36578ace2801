"""The Python side of privacy.distance_correlation without a GPU: its refusals, and the float64 reference of
tests/test_dcor_gpu.py against the textbook double-centred statistic."""
import numpy as np
import pytest
import torch

from test_dcor_gpu import statistic


def test_refusals():
    from splitcnn import privacy
    x, z = torch.zeros(4, 64), torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        privacy.distance_correlation(x, z)
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        privacy.distance_correlation(x.numpy(), z)
    xc, zc = torch.zeros(4, 3, 64), torch.zeros(4, 128, dtype=torch.bfloat16)
    for bad_x, bad_z, exc, words in (
            (xc.double(), zc, TypeError, "x: expected torch.float32"),
            (xc, zc.float(), TypeError, "z: expected torch.bfloat16"),
            (torch.zeros(256), zc, ValueError, "at least 2 dimensions"),
            (torch.zeros(4, 100), zc, ValueError, "x: 100 elements per sample"),
            (xc, torch.zeros(4, 0, dtype=torch.bfloat16), ValueError, "z: 0 elements per sample")):
        with pytest.raises(exc, match=words):
            privacy.distance_correlation(bad_x, bad_z)
    with pytest.raises(AttributeError):
        privacy.DistanceCorrelation(torch.zeros(4)).dcorr
    assert privacy.DistanceCorrelation(torch.tensor([0.5, 1, 2, 3])).dcor == 0.5
    assert (privacy.dcor_tau("x"), privacy.dcor_tau("z")) == (3200 * 2.0 ** -24, 16512 * 2.0 ** -24)


def test_reference_is_the_textbook_statistic():
    """n = 5, tau = 0: the closed form over raw distances equals the mean of the products of the double-centred
    distance matrices (Szekely et al. 2007, definition 4)."""
    g = np.random.default_rng(3)
    x, z = g.standard_normal((5, 64)), g.standard_normal((5, 128))
    got, _ = statistic(x, z, 0.0, 0.0, np.float64)

    def centred(v):
        d = np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1))
        return d - d.mean(0, keepdims=True) - d.mean(1, keepdims=True) + d.mean()
    A, B = centred(x), centred(z)
    cov, vx, vz = (A * B).mean(), (A * A).mean(), (B * B).mean()
    np.testing.assert_allclose(got, [np.sqrt(cov / np.sqrt(vx * vz)), cov, vx, vz], rtol=1e-12)
