"""Float64 oracle of the robust learning rate's kernels (``ddl_rlr_sum`` / ``ddl_rlr_flip`` in
csrc/kernels/clip_agg.hip), numpy on the host, written from the definitions: it shares no code with
the kernels or their torch twins.

Over the rows with cs_k != 0 (the others are neither read nor counted), with u_ki = fl32(x_ki - c_i)
(x_ki itself without a centre; ``clip_oracle.updates``: the one fp32 rounding of the definition):

* s_i = sum_k sgn(u_ki), sgn(+-0) = sgn(NaN) = 0. One IEEE fp32 subtraction and two comparisons:
  exact, so the kernel's votes must equal these.
* delta_i = sum_k cs_k u_ki in float64, mass_i = sum_k |cs_k u_ki|.
* flipped_i = |s_i| < theta; the result is -delta_i there, delta_i elsewhere. Negation is exact, so
  the error bound of the result is the sum's (``clip_oracle.sum_bound``).
"""
import numpy as np

import clip_oracle as C


def votes(X, c, cs):
    """-> s [n] float64, whole numbers."""
    u = C.updates(X, c)
    live = np.asarray(C._f64(cs)) != 0
    with np.errstate(all="ignore"):
        return ((u[live] > 0).astype(np.float64) - (u[live] < 0).astype(np.float64)).sum(0)


def weighted(X, c, cs):
    """-> (delta [n], mass [n]) in float64 for given fp32 row scales cs [G]."""
    u = C.updates(X, c)
    w = C._f64(cs)
    delta, mass = np.zeros(u.shape[1]), np.zeros(u.shape[1])
    for k in range(u.shape[0]):
        if w[k] != 0:
            delta += w[k] * u[k]
            mass += np.abs(w[k] * u[k])
    return delta, mass


def flipped(s, theta):
    return np.abs(s) < float(np.float32(theta))


def rlr(X, c, cs, theta):
    """-> (result [n], mass [n], s [n], flipped [n] bool)."""
    delta, mass = weighted(X, c, cs)
    s = votes(X, c, cs)
    flip = flipped(s, theta)
    return np.where(flip, -delta, delta), mass, s, flip
