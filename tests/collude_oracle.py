"""Float64 oracle of the colluding attacks (ALIE, IPM).

numpy on the host, written from the definitions, two passes (the mean, then the deviations from it):
it shares no code with the kernel (csrc/kernels/collude.hip) or its torch twin
(``ddl25spring_amd.ops.reference.collude_rows``), both of which are checked against it.

* update d_ji = fl32(s_ji - c_i) over the source rows (the one fp32 rounding the definition
  contains); a d that is NaN / Inf is left out, m_i = the finite ones of coordinate i;
* mu_i = mean, sigma_i = population std of the finite d_ji, in float64; m_i = 0: p_i = 0;
* ALIE p_i = mu_i - coef * sigma_i, IPM p_i = -coef * mu_i, in float64 (the kernel rounds it to fp32);
* every destination row is c_i + p_i.
"""
import numpy as np

EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24
ALIE, IPM = 0, 1


def _f32(t):
    return t.detach().cpu().float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def moments(S, c=None):
    """Source rows S [ns, n], centre c [n] or None -> (mu [n], sigma [n], m [n]) float64."""
    s = _f32(S)
    with np.errstate(all="ignore"):
        d = (s if c is None else s - _f32(c)[None, :]).astype(np.float64)
    ok = np.isfinite(d)
    m = ok.sum(0)
    cnt = np.maximum(m, 1)
    mu = np.where(ok, d, 0.0).sum(0) / cnt
    dev = np.where(ok, d - mu[None, :], 0.0)
    sigma = np.sqrt((dev * dev).sum(0) / cnt)
    return mu, sigma, m


def malicious(S, c, mode, coef):
    """-> (p [n] float64, bound [n]): the colluders' update and the error allowed to the kernel's
    fp32 p, 2^-23 (|mu| + coef sigma): one fp32 rounding of p and as much again for the error of
    the double-side one-pass moments."""
    mu, sigma, m = moments(S, c)
    p = mu - coef * sigma if mode == ALIE else -coef * mu
    p = np.where(m > 0, p, 0.0)
    return p, EPS23 * (np.abs(mu) + abs(coef) * sigma)


def row_bound(c, p, bound):
    """Error allowed to the written row fl32(c + p_kernel) against c + p: the bound on p and the add's
    rounding, 2^-24 |c + p_kernel| with |c + p_kernel| <= |c + p| + bound."""
    if c is None:
        return bound
    return bound + EPS24 * (np.abs(_f32(c).astype(np.float64) + p) + bound)
