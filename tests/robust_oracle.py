"""Float64 oracle of the Byzantine-robust aggregation rules, and the hostile inputs they are tested on.

Plain torch on the CPU, written from the rules' definitions (coordinate-wise median / trimmed mean:
Yin et al. 2018; Krum / multi-Krum: Blanchard et al. 2017). It shares no code with
``ddl25spring_amd.ops.functional`` or ``ddl25spring_amd.ops.reference``: the kernels and their CPU
twins are both checked against it.

The semantics below are the specification for non-finite inputs:

* coordinate selection sorts with a NaN ordered (and counted) as +inf;
* a squared distance that is not finite counts as +inf, so a row holding a NaN / Inf entry is
  infinitely far from everyone;
* a Krum score that is not finite ranks as +inf, ties go to the smaller key;
* multi-Krum selects min(m, K) clients.
"""
import math

import torch

INF = float("inf")


# ------------------------------------------------------------------------------------- the oracle
def sorted_clients(X):
    """X [K, n] -> float64 [K, n] sorted along the client axis, NaN replaced by +inf."""
    x = X.detach().cpu().double()
    x = torch.where(torch.isnan(x), torch.full_like(x, INF), x)
    return torch.sort(x, 0).values


def select(X, mode, trim=0):
    """Coordinate-wise 'median' (0.5 * (s[(K-1)//2] + s[K//2])) or 'trimmed' mean (the mean of
    s[trim : K-trim]) over the K rows of X -> float64 [n]."""
    s = sorted_clients(X)
    K = s.shape[0]
    if mode == "median":
        return 0.5 * (s[(K - 1) // 2] + s[K // 2])
    assert mode == "trimmed" and K - 2 * trim >= 1
    return s[trim:K - trim].mean(0)


def trimmed_bound(X, trim):
    """Per-coordinate error allowed to an fp32 trimmed mean: a sequential fp32 sum of the
    n = K - 2*trim kept values errs by at most (n - 1) * 2**-24 * sum|kept|, the division by n
    scales that to (n - 1) * 2**-24 * mean|kept| and adds one rounding of the result (at most
    2**-24 * mean|kept|), and one more unit covers the rounding of the float64 oracle to fp32:
    (n + 1) * 2**-24 * mean|kept|."""
    s = sorted_clients(X)
    K = s.shape[0]
    kept = s[trim:K - trim]
    return (K - 2 * trim + 1) * 2.0 ** -24 * kept.abs().mean(0)


def krum(X, nb, m, keys=None):
    """Krum / multi-Krum over the rows of X [K, P] -> (scores float64 [K], the selected rows as a
    list of min(m, K) indices, best first).

    Squared distances straight from the rows (no Gram); a distance that is not finite counts as
    +inf; score_i = the sum of the nb smallest distances from i to the others (with fewer than nb
    others, the missing ones count as +inf); clients ordered by (score, key), a score that is not
    finite counting as +inf."""
    x = X.detach().cpu().double()
    K = x.shape[0]
    keys = list(range(K)) if keys is None else [int(k) for k in keys]
    d2 = torch.full((K, K), INF, dtype=torch.float64)
    for i in range(K):
        t = ((x[i][None, :] - x) ** 2).sum(1)
        t = torch.where(torch.isfinite(t), t, torch.full_like(t, INF))
        t[i] = INF  # not a neighbour of itself
        d2[i] = t
    scores = torch.sort(d2, 1).values[:, :nb].sum(1)
    rank_by = [s if math.isfinite(s) else INF for s in scores.tolist()]
    order = sorted(range(K), key=lambda i: (rank_by[i], keys[i]))
    return scores, order[:min(m, K)]


def gram(X, c=None):
    """(X - c)(X - c)^T in float64."""
    x = X.detach().cpu().double()
    if c is not None:
        x = x - c.detach().cpu().double()
    return x @ x.t()


def rel_err(got, want):
    """max|got - want| / max|want| in float64 (the fp32 kernels' tolerance is 1e-5 of this)."""
    got = got.detach().cpu().double()
    want = want.detach().cpu().double()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


# ------------------------------------------------------------------------------ inputs under test
def strided(X, dev="cpu"):
    """The rows as the FL loop hands them over: a view into a wider flat buffer whose row stride
    is no multiple of 4 floats for aligned n and whose first column is not 16-byte aligned."""
    K, n = X.shape
    buf = torch.full((K, n + 13), -12345.0, dtype=X.dtype)
    buf[:, 5:5 + n] = X
    return buf.to(dev)[:, 5:5 + n]


BAD_KINDS = ("nan", "+inf", "-inf", "mix", "one_nan")       # coordinate selection
KRUM_BAD_KINDS = ("nan", "+inf", "-inf", "3e38", "1e30", "one_nan")
PLACEMENTS = ("first", "last", "interleaved")


def bad_index(K, f, where):
    """The rows of the f attackers among K clients."""
    if where == "first":
        return list(range(f))
    if where == "last":
        return list(range(K - f, K))
    assert where == "interleaved"
    return [(i * K) // f for i in range(f)]  # distinct (K >= f), row 0 among them


def attack_rows(K, f, n, kind, where, seed=0):
    """K client rows [K, n] fp32: honest rows 1 + 0.05 * randn, f bad rows of ``kind`` placed
    ``where`` -> (X, honest row indices, bad row indices)."""
    g = torch.Generator().manual_seed(1000 * K + 10 * f + seed)
    X = 1.0 + 0.05 * torch.randn(K, n, generator=g)
    bad = bad_index(K, f, where)
    assert len(set(bad)) == f
    for t, r in enumerate(bad):
        if kind == "nan":
            X[r] = float("nan")
        elif kind == "+inf":
            X[r] = INF
        elif kind == "-inf":
            X[r] = -INF
        elif kind == "mix":
            vals = torch.tensor([float("nan"), INF, -INF])
            X[r] = vals[(torch.arange(n) + t) % 3]
        elif kind == "3e38":
            X[r] = 3e38
        elif kind == "1e30":
            X[r] = 1e30
        elif kind == "one_nan":
            X[r, (7 * t + 3) % n] = float("nan")  # honest everywhere else
        else:
            raise ValueError(kind)
    honest = [i for i in range(K) if i not in set(bad)]
    return X, honest, bad
