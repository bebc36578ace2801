"""privacy.DPSGD without a GPU: the Renyi accountant and the host twin of slk_dp_noise's draws."""
import math

import numpy as np
import pytest


def dpsgd(sigma, seed=0):
    from splitcnn import privacy
    return privacy.DPSGD(1.0, sigma, seed=seed, device="cpu")


@pytest.mark.parametrize("sigma,steps,delta", ((0.7, 1, 1e-5), (1.1, 1000, 1e-5), (4.0, 20000, 1e-6)))
def test_accountant_at_full_sampling_is_the_gaussian_closed_form(sigma, steps, delta):
    from splitcnn.privacy import DP_ORDERS
    want = min(a / (2 * sigma ** 2) * steps + math.log(1 / delta) / (a - 1) for a in DP_ORDERS)
    assert dpsgd(sigma).epsilon(steps, 1.0, delta) == pytest.approx(want, rel=1e-12)


def test_accountant_is_monotone_in_steps_and_in_one_over_sigma():
    eps = [dpsgd(1.0).epsilon(s, 0.01, 1e-5) for s in (1, 10, 100, 1000, 10000)]
    eps2 = [dpsgd(s).epsilon(1000, 0.01, 1e-5) for s in (4.0, 2.0, 1.0, 0.7, 0.5)]
    assert all(0 < a < b < math.inf for e in (eps, eps2) for a, b in zip(e, e[1:]))


def test_host_twin_moments_on_2_to_20_draws():
    """The stated law is a unit normal cut at sqrt(48 ln 2) = 5.77 (mass beyond: 8e-9, variance deficit below 1e-6). With
    n = 2^20 draws the mean's standard error is n^-1/2 and the variance's sqrt(2 / n); both within 5 of them."""
    n = 1 << 20
    z = dpsgd(1.0, seed=11).noise_draws(np.arange(n), 3)
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    assert np.abs(z).max() <= math.sqrt(48 * math.log(2))
