"""Clipped FedAvg aggregation (csrc/kernels/clip_agg.hip: update norms, clip scales, clipped sum,
update + Gaussian noise) against the float64 oracle of tests/clip_oracle.py.

The ``check_*`` functions take the device, so tests/test_clipped_agg_cpu.py runs the same cases on
the torch twins; here they run on the kernels."""
import math

import numpy as np
import pytest
import torch

import clip_oracle as C
import robust_oracle as O
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

NORM_N = (1, 3, 4, 5, 255, 1024, 1027)
NORM_G = (1, 2, 7, 33, 200)
BIG_N = 8192 * 256 * 4 + 5  # one element quad per thread at the grid cap, and 5 more: a second pass
HOSTILE_K = (5, 65, 200)
EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24


def centers(c, dev):
    """-> [(tag, device centre or None, host centre or None)]: absent, 16-B aligned, and at a base
    one float past a 16-B boundary."""
    off = torch.zeros(c.numel() + 1, device=dev)[1:]
    off.copy_(c)
    if dev.type == "cuda":
        assert off.data_ptr() % 16 == 4
    return [("none", None, None), ("aligned", c.to(dev), c), ("misaligned", off, c)]


# ------------------------------------------------------------------------------------- 1: norms
def assert_norms(X, c_dev, c, rows, tag):
    sq = Fn.update_sqnorm(rows, c_dev)
    assert sq.dtype == torch.float64
    got = sq.sqrt().cpu().numpy()
    want = C.norms(X, c)
    worst = float((np.abs(got - want) / np.maximum(want, 1e-300)).max())
    print(f"norms {tag}: worst rel err {worst:.3e} (allowed {EPS23:.3e})")
    assert bool((np.abs(got - want) <= EPS23 * want).all()), f"norms {tag}: rel err {worst}"
    # and through clip_scales, rounded to fp32
    nrm, _ = Fn.clip_scales(sq, torch.ones(X.shape[0], device=rows.device), 1.0)
    assert nrm.dtype == torch.float32
    got = nrm.cpu().double().numpy()
    assert bool((np.abs(got - want) <= EPS23 * want).all()), f"fp32 norms {tag}"


def check_norms(G, dev):
    for n in NORM_N:
        g = torch.Generator().manual_seed(1000 * G + n)
        X = torch.randn(G, n, generator=g)
        c = torch.randn(n, generator=g)
        for tag, c_dev, c_host in centers(c, dev):
            assert_norms(X, c_dev, c_host, X.to(dev), f"G={G} n={n} {tag}")
            assert_norms(X, c_dev, c_host, O.strided(X, dev), f"G={G} n={n} {tag} strided")


def check_norms_second_pass(dev):
    """n just past 8192 blocks x 256 threads x 4, the streaming kernels' grid cap: every thread runs
    the grid-stride loop more than once (the norm kernel caps its grid lower still), the last on a
    partial quad. The tail is scaled by 30 so that a dropped element cannot hide in the tolerance."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(2, BIG_N, generator=g)
    X[:, BIG_N - 5:] *= 30.0
    c = torch.randn(BIG_N, generator=g)
    Xd = X.to(dev)
    assert_norms(X, None, None, Xd, "big")
    assert_norms(X, c.to(dev), c, Xd, "big centred")
    # the sum and the update pass at the same size: their grids are at the cap
    coeff = torch.tensor([0.75, 0.25])
    want, mass, _ = C.clipped_sum(X, c, coeff, 1000.0)
    delta, _, _ = pipeline(Xd, c.to(dev), coeff.to(dev), 1000.0)
    err = np.abs(delta.cpu().double().numpy() - want)
    assert bool((err <= C.sum_bound(2, None, mass)).all())
    w = torch.empty_like(delta)
    Fn.apply_update(w, c.to(dev), delta, 0.5, NOISE_SEED, 1)
    tail = torch.empty(9, device=dev)
    Fn.apply_update(tail, c.to(dev)[BIG_N - 9:], delta[BIG_N - 9:], 0.5, NOISE_SEED, 1, offset=BIG_N - 9)
    assert torch.equal(w[BIG_N - 9:], tail)
    z = (w - (c.to(dev) + delta)).cpu().double().numpy() / 0.5  # std * z, up to the add's rounding
    assert np.abs(z - C.normals(BIG_N, NOISE_SEED, 1)).max() <= 1e-5 + 2 * EPS24 * float(w.abs().max()) / 0.5


@pytest.mark.parametrize("G", NORM_G)
def test_update_norms(cuda, G):
    check_norms(G, cuda)


def test_update_norms_second_grid_stride_iteration(cuda):
    check_norms_second_pass(cuda)


# ------------------------------------------------------------------------------- 2: clipped sum
def pipeline(rows, c_dev, coeff, clip, out=None, accumulate=False):
    """update_sqnorm -> clip_scales -> clipped_sum -> (delta, norms, cs)."""
    sq = Fn.update_sqnorm(rows, c_dev)
    nrm, cs = Fn.clip_scales(sq, coeff, clip)
    if out is None:
        out = torch.empty(rows.shape[1], dtype=torch.float32, device=rows.device)
    Fn.clipped_sum(rows, c_dev, cs, out, accumulate)
    return out, nrm, cs


def assert_sum(X, c, c_dev, rows, coeff, clip, tag):
    G = X.shape[0]
    dev = rows.device
    want, mass, want_cs = C.clipped_sum(X, c, coeff, clip)
    delta, _, cs = pipeline(rows, c_dev, coeff.to(dev), clip)
    cs_err = np.abs(cs.cpu().double().numpy() - want_cs)
    assert bool((cs_err <= EPS23 * np.abs(want_cs)).all()), f"{tag}: cs off by more than an ulp"
    # delta alone (no centre term in the bound), then w = c + delta through apply_update
    err = np.abs(delta.cpu().double().numpy() - want)
    bound = C.sum_bound(G, None, mass)
    print(f"clipped_sum {tag}: worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"clipped_sum {tag}"
    w = torch.empty_like(delta)
    Fn.apply_update(w, c_dev, delta)
    err = np.abs(w.cpu().double().numpy() - (want + (0.0 if c is None else C._f64(c))))
    assert bool((err <= C.sum_bound(G, c, mass)).all()), f"c + delta {tag}"
    # accumulate: the rows in two calls are the same ordered sum, bit for bit
    if G >= 2:
        h = G // 2
        acc = torch.empty_like(delta)
        Fn.clipped_sum(rows[:h], c_dev, cs[:h].contiguous(), acc, False)
        Fn.clipped_sum(rows[h:], c_dev, cs[h:].contiguous(), acc, True)
        assert torch.equal(acc, delta), f"accumulate {tag}"
    return delta


def check_clipped_sum(G, dev):
    for n in (1, 5, 1024, 1027):
        g = torch.Generator().manual_seed(77 * G + n)
        c = torch.randn(n, generator=g)
        X = c + torch.randn(G, 1, generator=g).exp() * torch.randn(G, n, generator=g) / math.sqrt(n)
        coeff = torch.rand(G, generator=g) + 0.1
        coeff /= coeff.sum()
        clip = 1.0  # update norms are lognormal around 1: some rows clipped, some not
        for tag, c_dev, c_host in centers(c, dev):
            Xc = X if c_host is not None else X - c
            a = assert_sum(Xc, c_host, c_dev, Xc.to(dev), coeff, clip, f"G={G} n={n} {tag}")
            b = assert_sum(Xc, c_host, c_dev, O.strided(Xc, dev), coeff, clip, f"G={G} n={n} {tag} strided")
            assert torch.equal(a, b), f"G={G} n={n} {tag}: vector and scalar paths differ"
        if G >= 7 and n >= 5:  # the case is about both kinds of row
            nrm = C.norms(X, c)
            assert (nrm > clip).any() and (nrm <= clip).any()


@pytest.mark.parametrize("G", NORM_G)
def test_clipped_sum(cuda, G):
    check_clipped_sum(G, cuda)


# ---------------------------------------------------------------------------- 3: exact boundary
def check_exact_boundary(dev):
    """||u|| = 5 exactly (entries 3 and 4): C = 5 leaves s = 1.0 and the bits of C = inf; C = 2.5
    halves exactly."""
    G, n = 6, 40
    g = torch.Generator().manual_seed(9)
    c = torch.randint(-4, 5, (n,), generator=g).float()
    U = torch.zeros(G, n)
    for k in range(G):
        i, j = (3 * k) % n, (7 * k + 11) % n
        U[k, i], U[k, j] = (3.0, -4.0) if k % 2 else (4.0, 3.0)
    X = c + U
    coeff = torch.tensor([0.25, 0.125, 0.0625, 0.3125, 0.125, 0.125])
    rows, c_dev = O.strided(X, dev), c.to(dev)
    at, nrm, cs = pipeline(rows, c_dev, coeff.to(dev), 5.0)
    assert nrm.cpu().tolist() == [5.0] * G
    assert torch.equal(cs.cpu(), coeff)  # s_k == 1.0
    free, _, _ = pipeline(rows, c_dev, coeff.to(dev), math.inf)
    assert torch.equal(at, free)
    assert torch.equal(at.cpu(), (coeff[:, None] * U).sum(0))  # exact in fp32
    half, _, cs = pipeline(rows, c_dev, coeff.to(dev), 2.5)
    assert torch.equal(cs.cpu(), coeff * 0.5)  # s_k == 0.5
    assert torch.equal(half.cpu(), 0.5 * at.cpu())
    # a zero update has norm 0 <= C: s = 1, not 0 / 0
    zero, nrm, cs = pipeline(c_dev[None, :].clone(), c_dev, coeff[:1].to(dev), 5.0)
    assert nrm.cpu().tolist() == [0.0] and torch.equal(cs.cpu(), coeff[:1]) and not bool(zero.any())


def test_exact_boundary(cuda):
    check_exact_boundary(cuda)


# ------------------------------------------------------------------------------ 4: hostile rows
def check_hostile(K, kind, dev):
    n, clip = 300, 0.5
    f = K // 4
    c = torch.ones(n)
    for where in O.PLACEMENTS:
        X, honest, bad = O.attack_rows(K, f, n, kind, where)
        tag = f"K={K} {kind} {where}"
        g = torch.Generator().manual_seed(K)
        coeff = torch.rand(K, generator=g) + 0.5
        coeff /= coeff.sum()
        want, mass, want_cs = C.clipped_sum(X, c, coeff, clip)
        if kind in ("nan", "+inf", "-inf", "one_nan"):
            assert not want_cs[bad].any() and want_cs[honest].all(), tag  # the oracle drops them
        else:
            assert want_cs.all(), tag                                     # ... and clips these
        rows, c_dev = O.strided(X, dev), c.to(dev)
        delta, nrm, cs = pipeline(rows, c_dev, coeff.to(dev), clip)
        assert torch.equal(cs.cpu() == 0, torch.from_numpy(want_cs == 0)), tag
        if kind == "3e38":
            assert bool(torch.isinf(nrm.cpu()[bad]).all()), tag  # finite rows, norm past fp32
        w = torch.empty_like(delta)
        Fn.apply_update(w, c_dev, delta)
        got = w.cpu().double().numpy()
        assert np.isfinite(got).all(), tag
        err = np.abs(got - (want + 1.0))
        bound = C.sum_bound(K, c, mass)
        assert bool((err <= bound).all()), f"{tag}: err / bound = {float((err / bound).max())}"
        moved = float(np.sqrt(((got - 1.0) ** 2).sum()))
        assert moved <= clip * float(coeff.double().sum()) * (1 + 2.0 ** -20), f"{tag}: moved {moved}"


@pytest.mark.parametrize("kind", O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K", HOSTILE_K)
def test_hostile_rows(cuda, K, kind):
    check_hostile(K, kind, cuda)


# ------------------------------------------------------------------------------ 5: determinism
def check_deterministic(dev):
    g = torch.Generator().manual_seed(11)
    n, G = 300_003, 7  # several hundred blocks of partial norms
    c = torch.randn(n, generator=g)
    X = c + 0.01 * torch.randn(G, n, generator=g)
    rows, c_dev = X.to(dev), c.to(dev)
    coeff = torch.full((G,), 1.0 / G, device=dev)
    a, na, _ = pipeline(rows, c_dev, coeff, 1.0)
    sq_a = Fn.update_sqnorm(rows, c_dev)
    b, nb, _ = pipeline(rows, c_dev, coeff, 1.0)
    assert torch.equal(sq_a, Fn.update_sqnorm(rows, c_dev))
    assert torch.equal(a, b) and torch.equal(na, nb)


def test_two_calls_are_bit_equal(cuda):
    check_deterministic(cuda)


# ------------------------------------------------------------------------------------- 6: noise
NOISE_N, NOISE_SEED = 1 << 20, (5 << 32) | 12345


def draws(n, seed, rnd, dev, offset=0):
    z = torch.empty(n, dtype=torch.float32, device=dev)
    Fn.apply_update(z, None, torch.zeros(n, device=dev), 1.0, seed, rnd, offset)
    return z


def check_noise_matches_oracle(dev):
    """Within 1e-5 absolute: the fp32 rounding of 2 pi U moves the angle by at most 4e-7 and
    R <= 5.77; logf / sqrtf / sincosf add a few ulps of values below 5.77."""
    z = draws(NOISE_N, NOISE_SEED, 3, dev).cpu().double().numpy()
    want = C.normals(NOISE_N, NOISE_SEED, 3)
    # the oracle's own draws meet the five-sigma moment conditions for this seed ...
    assert abs(want.mean()) <= 5 / math.sqrt(NOISE_N) and abs(want.var() - 1) <= 5 * math.sqrt(2 / NOISE_N)
    assert np.abs(want).max() <= 5.77
    err = float(np.abs(z - want).max())
    print(f"noise: max |z - oracle| = {err:.3e}")
    assert err <= 1e-5
    # ... and so do the op's
    assert abs(z.mean()) <= 5 / math.sqrt(NOISE_N), z.mean()
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / NOISE_N), z.var()


def check_noise_purity(dev):
    n = 1027
    g = torch.Generator().manual_seed(2)
    c, delta = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    full = torch.empty(n, device=dev)
    Fn.apply_update(full, c, delta, 0.3, NOISE_SEED, 7)
    for a in (1, 2, 3, 5):
        for b in (n, n - 2):
            sub = torch.empty(b - a, device=dev)
            Fn.apply_update(sub, c[a:b], delta[a:b], 0.3, NOISE_SEED, 7, offset=a)
            assert torch.equal(sub, full[a:b]), f"slice [{a}, {b})"
    sub = torch.empty(n - 8, device=dev)  # an aligned slice: the vector path again
    Fn.apply_update(sub, c[8:], delta[8:], 0.3, NOISE_SEED, 7, offset=8)
    assert torch.equal(sub, full[8:])
    # another round or seed: other draws; the same: the same
    z = draws(n, NOISE_SEED, 7, dev)
    assert torch.equal(z, draws(n, NOISE_SEED, 7, dev))
    assert not torch.equal(z, draws(n, NOISE_SEED, 8, dev))
    assert not torch.equal(z, draws(n, NOISE_SEED + 1, 7, dev))
    assert not torch.equal(z, draws(n, NOISE_SEED + (1 << 32), 7, dev))
    # w = c + delta + std * z, each step rounded; in place over c as well
    want = (c + delta) + torch.tensor(0.3, device=dev) * z
    assert torch.equal(full, want)
    w = c.clone()
    Fn.apply_update(w, w, delta, 0.3, NOISE_SEED, 7)
    assert torch.equal(w, full)


def check_zero_std(dev):
    for n in (1, 5, 1027):
        g = torch.Generator().manual_seed(n)
        c, delta = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
        w = torch.empty(n, device=dev)
        Fn.apply_update(w, c, delta, 0.0, NOISE_SEED, 1)
        assert torch.equal(w, c + delta)
        Fn.apply_update(w, None, delta, 0.0, NOISE_SEED, 1)
        assert torch.equal(w, delta)
        w = torch.zeros(n + 1, device=dev)[1:]  # misaligned output: the scalar path
        Fn.apply_update(w, c, delta)
        assert torch.equal(w, c + delta)


def test_noise_matches_oracle_and_moments(cuda):
    check_noise_matches_oracle(cuda)


def test_noise_is_a_pure_function_of_seed_round_index(cuda):
    check_noise_purity(cuda)


def test_zero_std_is_exactly_center_plus_delta(cuda):
    check_zero_std(cuda)


# --------------------------------------------------------------------------- 7: the aggregator
# These cases run from tests/test_clipped_agg_cpu.py, parametrised over the device (its device half
# is marked gpu), so that each exists once.
def check_aggregator(weighting, dev):
    K, P, clip = 200, 515, 0.7
    ctx = DistContext()
    g = torch.Generator().manual_seed(21)
    c = torch.randn(P, generator=g)
    X = c + torch.randn(K, 1, generator=g).exp() * torch.randn(K, P, generator=g) / math.sqrt(P)
    X[17] = float("nan")
    coeff = torch.rand(K, generator=g) + 0.5
    coeff /= coeff.sum()
    used = coeff if weighting == "samples" else torch.full((K,), 1.0 / K)
    want, mass, _ = C.clipped_sum(X, c, used, clip)
    agg = A.make_aggregator("norm_clip", clip=clip, weighting=weighting)
    assert agg.name == "clipped_mean" and agg.takes_center and not agg.needs_all
    w = c.clone().to(dev)
    out = agg(ctx, O.strided(X, dev), coeff.to(dev), w, center=w, counts=[K])
    assert out is w
    err = np.abs(w.cpu().double().numpy() - (want + C._f64(c)))
    assert bool((err <= C.sum_bound(K, c, mass)).all()), weighting
    nrm = np.array(agg.last_norms)
    ref = C.norms(X, c)
    assert len(nrm) == K and math.isnan(nrm[17])
    keep = np.arange(K) != 17
    assert bool((np.abs(nrm[keep] - ref[keep]) <= EPS23 * ref[keep]).all())
    assert agg.state_dict()["rounds"] == 1 and agg.epsilon(1000, 1e-5) == math.inf


def check_aggregator_noise(dev):
    K, P, clip, zmul, seed = 200, 515, 0.7, 1.3, 77
    ctx = DistContext()
    g = torch.Generator().manual_seed(22)
    c = torch.randn(P, generator=g)
    X = c + torch.randn(K, P, generator=g) / math.sqrt(P)
    with pytest.raises(ValueError):
        A.ClippedMean(clip, noise_multiplier=zmul)  # samples weighting: sensitivity is not C / K
    with pytest.raises(ValueError):
        A.make_aggregator("clipped", clip=clip, noise_multiplier=zmul, weighting="samples")
    with pytest.raises(ValueError):
        A.ClippedMean(0.0)
    agg = A.ClippedMean(clip, zmul, seed, "uniform")
    rows = X.to(dev)
    outs = []
    for r in range(3):
        out = torch.empty(P, device=dev)
        agg(ctx, rows, None, out, center=c.to(dev), counts=[K])
        outs.append(out.cpu())
    want, mass, _ = C.clipped_sum(X, c, torch.full((K,), 1.0 / K), clip)
    std = zmul * clip / K
    for r, out in enumerate(outs):
        ref = want + C._f64(c) + float(np.float32(std)) * C.normals(P, seed, r)
        err = np.abs(out.double().numpy() - ref)
        # the sum's bound, the noise draw's 1e-5 absolute (times std) and the two roundings of
        # std * z and its add
        bound = C.sum_bound(K, c, mass) + std * 1e-5 + 2 * EPS24 * (np.abs(ref) + std * 5.77)
        assert bool((err <= bound).all()), f"round {r}"
    assert not torch.equal(outs[0], outs[1])  # the round counter moves the noise
    # the counter is the state: a fresh object loaded with it continues the stream
    sd = agg.state_dict()
    assert sd["rounds"] == 3
    fresh = A.ClippedMean(clip, zmul, seed, "uniform")
    fresh.load_state_dict(sd)
    a, b = torch.empty(P, device=dev), torch.empty(P, device=dev)
    agg(ctx, rows, None, a, center=c.to(dev), counts=[K])
    fresh(ctx, rows, None, b, center=c.to(dev), counts=[K])
    assert torch.equal(a, b) and not torch.equal(a.cpu(), outs[2])
    eps = agg.epsilon(1000, 1e-5)
    assert 0 < eps < math.inf and agg.epsilon(2000, 1e-5) < eps
    # a rank without clients contributes a zero delta
    out = torch.empty(P, device=dev)
    A.ClippedMean(clip)(ctx, rows[:0], torch.empty(0, device=dev), out, center=c.to(dev), counts=[0])
    assert torch.equal(out.cpu(), c)
