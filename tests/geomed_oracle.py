"""Float64 oracle of the geometric median by the smoothed Weiszfeld iteration (RFA: Pillutla,
Kakade, Harchaoui 2022), written from the definition.

numpy on the host; it shares no code with the kernels (csrc/kernels/clip_agg.hip: ``ddl_gm_scales``)
or their torch twins, both of which are checked against it.

    v^0 = 0 ("zero")  or  sum_k a_k u_k / sum_k a_k ("mean"), u_k = x_k - c
    d_k = ||x_k - (c + v)||,  beta_k = a_k / max(nu, d_k),  b_k = beta_k / sum_j beta_j
    v <- v + sum_k b_k (x_k - (c + v)),  L times;  out = c + v

A row whose squared distance is NaN / Inf has beta_k = 0.
"""
import numpy as np

import clip_oracle as C


def scales(sq, coeff, nu, init=False, total=None):
    """-> (norms [G], cs [G] = beta_k / T unrounded, S = sum_k beta_k in index order), float64."""
    sq = np.asarray(sq, dtype=np.float64)
    a = C._f32(coeff).astype(np.float64)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(sq)
        beta = a if init else a / np.maximum(nu, nrm)
    beta = np.where(sq < np.inf, beta, 0.0)  # false for NaN and +inf
    S = 0.0
    for b in beta:
        S += float(b)
    T = S if total is None else float(total)
    cs = np.zeros_like(beta) if T == 0.0 else beta / T
    return nrm, cs, S


def geomed(X, c, coeff, iters, nu, init="zero"):
    """-> (out [n], the last iteration's b [G], per iteration the distances [G]), float64."""
    x = C._f64(X)
    base = np.zeros(x.shape[1]) if c is None else C._f64(c)
    v = np.zeros(x.shape[1])
    b, dists = np.zeros(x.shape[0]), []
    for mean_step in [True] * (init == "mean") + [False] * iters:
        with np.errstate(all="ignore"):
            d = x - (base + v)[None, :]
            sq = (d * d).sum(1)
        nrm, b, _ = scales(sq, coeff, nu, mean_step)
        dists.append(nrm)
        for k in range(x.shape[0]):
            if b[k] != 0:
                v = v + b[k] * d[k]
    return base + v, b, dists
