"""Float64 oracle of Bulyan (El Mhamdi, Guerraoui, Rouault 2018), written from its definition.

Plain torch on the CPU; it shares no code with ``ddl25spring_amd.ops``: the kernels
(csrc/kernels/aggregate.hip: ``ddl_bulyan_select``, ``ddl_bulyan_coord``) and their CPU twins are
both checked against it. The rules for non-finite values are ``robust_oracle``'s.

* Selection. R = all K clients; for t = 0 .. theta-1 (theta = K - 2f), with n' = K - t clients left:
  nb_t = min(max(n' - f - 2, 1), n' - 1); score_i = the sum of the nb_t smallest squared distances
  from i to the others in R (a distance that is not finite counts as +inf); the least (score, key)
  is picked and leaves R (a score that is not finite ranks as +inf).
* Coordinates. The theta picked values of a coordinate sorted ascending to s, a NaN as +inf;
  a = (theta-1)//2, b = theta//2, beta = theta - 2f; the kept window is [lo, lo + beta) with
  lo = #{ i in [0, theta - beta) : s[i] + s[i+beta] < s[a] + s[b] }; the result is its mean.
"""
import math

import torch

import robust_oracle as O

INF = O.INF


def distances(X):
    """Squared distances straight from the rows -> float64 [K, K], +inf where not finite and on
    the diagonal."""
    x = X.detach().cpu().double()
    K = x.shape[0]
    d2 = torch.full((K, K), INF, dtype=torch.float64)
    for i in range(K):
        t = ((x[i][None, :] - x) ** 2).sum(1)
        t = torch.where(torch.isfinite(t), t, torch.full_like(t, INF))
        t[i] = INF
        d2[i] = t
    return d2


def select(X, f, keys=None):
    """-> (the winners' scores, the picked rows in order of selection, the number of picks that
    only the keys decided: another client left had the winner's score)."""
    K = X.shape[0]
    assert f >= 0 and K >= 4 * f + 3
    keys = list(range(K)) if keys is None else [int(k) for k in keys]
    d2 = distances(X)
    left, sel, win, ties = list(range(K)), [], [], 0
    for t in range(K - 2 * f):
        n1 = K - t
        nb = min(max(n1 - f - 2, 1), n1 - 1)
        idx = torch.tensor(left)
        near = torch.sort(d2[idx][:, idx], 1).values  # the diagonal (+inf) sorts last
        acc = torch.zeros(n1, dtype=torch.float64)
        for j in range(nb):  # ascending
            acc = acc + near[:, j]
        score = {i: (s if math.isfinite(s) else INF) for i, s in zip(left, acc.tolist())}
        w = min(left, key=lambda i: (score[i], keys[i]))
        ties += any(i != w and score[i] == score[w] for i in left)
        left.remove(w)
        sel.append(w)
        win.append(score[w])
    return win, sel, ties


def window_lo(s, beta):
    """s float64 [theta, n] sorted ascending -> lo int64 [n], the count definition."""
    theta = s.shape[0]
    span = theta - beta
    mid = s[(theta - 1) // 2] + s[theta // 2]
    return ((s[:span] + s[beta:beta + span]) < mid).sum(0)


def window(s, beta):
    """-> float64 [beta, n]: the kept values, ascending."""
    lo = window_lo(s, beta)
    return torch.stack([s.gather(0, (lo + j)[None])[0] for j in range(beta)])


def window_brute(s, beta):
    """The same window by its meaning: the beta values nearest the median, ties to the lower index
    -> float64 [beta, n] ascending."""
    theta = s.shape[0]
    med = 0.5 * (s[(theta - 1) // 2] + s[theta // 2])
    order = torch.sort((s - med).abs(), dim=0, stable=True).indices[:beta]  # stable: ties by index
    return torch.sort(s.gather(0, order), 0).values


def coord(X, sel, beta):
    """-> (the result float64 [n], the per-coordinate bound of an fp32 kernel): as
    ``robust_oracle.trimmed_bound``, a sequential fp32 sum of beta values errs by at most
    (beta - 1) 2^-24 sum|kept|, the division by beta scales that to the mean and adds one rounding,
    one more unit for rounding the float64 result to fp32: (beta + 1) 2^-24 mean|kept|."""
    s = O.sorted_clients(X[torch.as_tensor(sel, dtype=torch.long)])
    kept = window(s, beta)
    return kept.mean(0), (beta + 1) * 2.0 ** -24 * kept.abs().mean(0)
