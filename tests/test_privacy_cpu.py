"""The RDP accountant of ``ddl25spring_amd.fl.privacy`` (sampled Gaussian mechanism, integer orders)."""
import math

import numpy as np
import pytest

from ddl25spring_amd.fl import privacy


def test_full_participation_is_the_gaussian_mechanism():
    """q = 1: no subsampling, eps(alpha) = alpha / (2 z^2)."""
    for z in (0.5, 1.1, 4.0):
        orders = list(range(2, 65))
        got = privacy.rdp_subsampled_gaussian(1.0, z, orders)
        for a, e in zip(orders, got):
            assert abs(e - a / (2 * z * z)) <= 1e-12 * max(1.0, a / (2 * z * z)), (z, a)


def _quadrature(alpha, q, z, h):
    """E_{x ~ N(0, z^2)} [((1 - q) + q exp((2x - 1) / (2 z^2)))^alpha] by the trapezoid rule with
    step h over +-40 z (the integrand is analytic and decays like a Gaussian there)."""
    x = np.arange(-40.0 * z, 40.0 * z + h, h)
    dens = np.exp(-x * x / (2 * z * z)) / (z * math.sqrt(2 * math.pi))
    return float(np.sum(dens * ((1 - q) + q * np.exp((2 * x - 1) / (2 * z * z))) ** alpha) * h)


@pytest.mark.parametrize("alpha", range(2, 9))
def test_moment_equals_quadrature(alpha):
    q, z = 0.1, 1.1
    coarse, fine = _quadrature(alpha, q, z, 2e-3), _quadrature(alpha, q, z, 1e-3)
    tol = max(10 * abs(coarse - fine) / fine, 1e-12)  # the quadrature's own convergence
    eps = privacy.rdp_subsampled_gaussian(q, z, [alpha])[0]
    got = math.exp(eps * (alpha - 1))
    print(f"alpha={alpha}: A={got:.15g} quadrature={fine:.15g} tol={tol:.1e}")
    assert abs(got - fine) <= tol * fine


def test_epsilon_monotone():
    d = 1e-5
    by_rounds = [privacy.epsilon(r, 0.05, 1.1, d) for r in (1, 2, 10, 100, 1000)]
    assert all(a < b for a, b in zip(by_rounds, by_rounds[1:])), by_rounds
    by_q = [privacy.epsilon(100, q, 1.1, d) for q in (0.001, 0.01, 0.05, 0.2, 1.0)]
    assert all(a < b for a, b in zip(by_q, by_q[1:])), by_q
    by_z = [privacy.epsilon(100, 0.05, z, d) for z in (0.6, 0.8, 1.1, 2.0, 5.0)]
    assert all(a > b for a, b in zip(by_z, by_z[1:])), by_z
    assert privacy.epsilon(0, 0.05, 1.1, d) == 0.0


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        privacy.rdp_subsampled_gaussian(0.1, 0.0, [2])
    with pytest.raises(ValueError):
        privacy.rdp_subsampled_gaussian(1.5, 1.0, [2])
    with pytest.raises(ValueError):
        privacy.rdp_subsampled_gaussian(0.1, 1.0, [1.5])
    with pytest.raises(ValueError):
        privacy.epsilon(10, 0.1, 1.0, 0.0)
