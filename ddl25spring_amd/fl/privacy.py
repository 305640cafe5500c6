"""Privacy accounting for DP-FedAvg (``fl.aggregate.ClippedMean`` with noise): host-only.

Rényi DP of the Poisson-subsampled Gaussian mechanism at integer orders (Mironov, Talwar, Zhang
2019, "Rényi differential privacy of the sampled Gaussian mechanism", eq. for integer alpha):

    A_alpha = sum_{k=0..alpha} C(alpha, k) (1 - q)^(alpha - k) q^k exp((k^2 - k) / (2 z^2))
    eps(alpha) = ln A_alpha / (alpha - 1)

with sampling rate q and noise multiplier z (noise std = z x sensitivity). RDP composes additively
over rounds, and (alpha, eps)-RDP gives (eps + ln(1 / delta) / (alpha - 1), delta)-DP.

Caveats of the number this reports for a federated run:

* the server samples a fixed-size set of clients without replacement; the bound is for Poisson
  sampling at rate q = K / N, the usual approximation;
* the kernel's normal draws come from 24-bit uniforms (Box-Muller), so |z| <= 5.77: the Gaussian
  tail beyond that is missing;
* BatchNorm running statistics are averaged outside the clipped, noised vector.
"""
from __future__ import annotations

import math


def _logsumexp(xs) -> float:
    m = max(xs)
    if m == -math.inf:
        return -math.inf
    return m + math.log(sum(math.exp(x - m) for x in xs))


def rdp_subsampled_gaussian(q: float, z: float, orders) -> list[float]:
    """eps(alpha) of one step of the sampled Gaussian mechanism at the integer ``orders`` (>= 2),
    evaluated in log space."""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"sampling rate q must be in [0, 1], got {q}")
    if not z > 0.0:
        raise ValueError(f"noise multiplier z must be positive, got {z}")
    out = []
    for a in orders:
        if int(a) != a or a < 2:
            raise ValueError(f"orders must be integers >= 2, got {a}")
        a = int(a)
        if q == 0.0:
            out.append(0.0)
            continue
        terms = []
        for k in range(a + 1):
            if q == 1.0 and k < a:
                continue  # (1 - q)^(alpha - k) = 0
            t = math.log(math.comb(a, k)) + k * math.log(q) + (k * k - k) / (2.0 * z * z)
            if k < a:
                t += (a - k) * math.log1p(-q)
            terms.append(t)
        out.append(_logsumexp(terms) / (a - 1))
    return out


def epsilon(rounds: int, q: float, z: float, delta: float, orders=range(2, 257)) -> float:
    """(epsilon, delta)-DP after ``rounds`` steps: min over alpha of rounds * eps(alpha) +
    ln(1 / delta) / (alpha - 1)."""
    if not 0.0 < delta < 1.0:
        raise ValueError(f"delta must be in (0, 1), got {delta}")
    if rounds <= 0 or q == 0.0:
        return 0.0
    orders = list(orders)
    rdp = rdp_subsampled_gaussian(q, z, orders)
    return min(rounds * e + math.log(1.0 / delta) / (a - 1) for a, e in zip(orders, rdp))
