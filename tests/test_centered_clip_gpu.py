"""Centered clipping (``CenteredClip``; csrc/kernels/clip_agg.hip: the fused step ``ddl_cc_step``)
against the float64 oracle of tests/clip_oracle.py, one step at a time.

The ``check_*`` functions take the device, so tests/test_centered_clip_cpu.py runs the same cases on
the torch twins; here they run on the kernels."""
import math

import numpy as np
import pytest
import torch

import clip_oracle as C
import robust_oracle as O
from test_clipped_agg_gpu import BIG_N
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

FUSED_G = (1, 2, 4, 5, 8, 16)
UNFUSED_G = (17, 33)
STEP_N = (1, 5, 1027)
EPS23, EPS24 = 2.0 ** -23, 2.0 ** -24


def step_fused(rows, c, ctr, v, cs, want_norms=True):
    """-> (v_out, ctr_out, next squared norms) of one ``Fn.cc_step``."""
    v_out, ctr_out = torch.empty_like(v), torch.empty_like(v)
    sq = Fn.cc_step(rows, c, ctr, v, cs, v_out, ctr_out, want_norms)
    return v_out, ctr_out, sq


def step_unfused(rows, c, ctr, v, cs, want_norms=True):
    """The same step on the clipped mean's ops, as ``CenteredClip``'s unfused route takes it."""
    delta = torch.empty_like(v)
    Fn.clipped_sum(rows, ctr, cs, delta)
    v_out = v + delta
    ctr_out = torch.empty_like(v)
    Fn.apply_update(ctr_out, c, v_out)
    return v_out, ctr_out, Fn.update_sqnorm(rows, ctr_out) if want_norms else None


def scales_at(rows, ctr, coeff, tau):
    return Fn.clip_scales(Fn.update_sqnorm(rows, ctr), coeff, tau)


def problem(G, n, seed, with_v):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, generator=g)
    X = c + torch.randn(G, 1, generator=g).exp() * torch.randn(G, n, generator=g) / math.sqrt(n)
    coeff = torch.rand(G, generator=g) + 0.1
    coeff /= coeff.sum()
    v = 0.3 * torch.randn(n, generator=g) / math.sqrt(n) if with_v else torch.zeros(n)
    return X, c, coeff, v


# ------------------------------------------------------------------------------------ 1: one step
def assert_step(step, X, c, coeff, v, tau, dev, tag, next_norms, rows=None):
    G = X.shape[0]
    ctr = v if c is None else c + v  # fl32(c + v)
    rows = X.to(dev) if rows is None else rows
    c_dev = None if c is None else c.to(dev)
    _, cs = scales_at(rows, ctr.to(dev), coeff.to(dev), tau)
    v_out, ctr_out, sq = step(rows, c_dev, ctr.to(dev), v.to(dev), cs)
    want, mass, _ = C.clipped_sum(X, ctr, coeff, tau)
    v_want = C._f64(v) + want
    bound = C.sum_bound(G, v, mass)
    err = np.abs(v_out.cpu().double().numpy() - v_want)
    print(f"cc step {tag}: worst err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), f"v_out {tag}"
    if c is None:
        assert torch.equal(ctr_out, v_out), tag
    else:
        assert torch.equal(ctr_out, c_dev + v_out), f"ctr_out != fl32(c + v_out) {tag}"
        ctr_want = C._f64(c) + v_want
        err = np.abs(ctr_out.cpu().double().numpy() - ctr_want)
        assert bool((err <= bound + EPS24 * (np.abs(ctr_want) + bound)).all()), f"ctr_out {tag}"
    if next_norms:
        got = sq.sqrt().cpu().numpy()
        want_n = C.norms(X, ctr_out.cpu())
        live = cs.cpu().numpy() != 0
        assert bool((np.abs(got - want_n)[live] <= EPS23 * want_n[live]).all()), f"next norms {tag}"
        assert bool(np.isinf(got[~live]).all()), f"rows not read {tag}"
    return v_out, ctr_out, sq


def check_one_step(G, dev, fused):
    step = step_fused if fused else step_unfused
    for n in STEP_N:
        for with_v in (False, True):
            X, c, coeff, v = problem(G, n, 31 * G + n, with_v)
            nrm = C.norms(X, c + v)
            for where, tau in (("below", 0.5 * nrm.min()), ("inside", float(np.median(nrm))), ("above", 2.0 * nrm.max())):
                tag = f"{'fused' if fused else 'unfused'} G={G} n={n} v={'random' if with_v else 0} tau {where}"
                a = assert_step(step, X, c, coeff, v, float(tau), dev, tag, True)
                b = assert_step(step, X, c, coeff, v, float(tau), dev, tag + " strided", True, O.strided(X, dev))
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"{tag}: vector and scalar paths differ"
                assert torch.equal(a[2], b[2]), f"{tag}: the norms of the two paths differ"
            # without a centre the rows are the updates and ctr is v itself
            assert_step(step, X - c, None, coeff, v, float(np.median(nrm)), dev, f"G={G} n={n} no centre", True)
        if G >= 4 and n >= 5:  # the case is about both kinds of row
            assert (nrm > np.median(nrm)).any() and (nrm <= np.median(nrm)).any()


def check_step_second_pass(dev, fused=True):
    """n past the grid cap of every streaming kernel: a second grid-stride pass ending on a partial
    quad, the tail scaled by 30 so that a dropped element cannot hide in the tolerance."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(2, BIG_N, generator=g)
    X[:, BIG_N - 5:] *= 30.0
    c = torch.randn(BIG_N, generator=g)
    v = torch.zeros(BIG_N)
    assert_step(step_fused if fused else step_unfused, X, c, torch.tensor([0.75, 0.25]), v, 3000.0, dev, "big", True)


@pytest.mark.parametrize("G", FUSED_G)
def test_fused_step(cuda, G):
    check_one_step(G, cuda, True)


@pytest.mark.parametrize("G", FUSED_G + UNFUSED_G)
def test_unfused_step(cuda, G):
    check_one_step(G, cuda, False)


def test_fused_step_second_grid_stride_iteration(cuda):
    check_step_second_pass(cuda)


def test_fused_step_is_deterministic_and_takes_at_most_16_rows(cuda):
    X, c, coeff, v = problem(8, 300_003, 5, True)  # several hundred blocks of partial norms
    rows, ctr = X.to(cuda), (c + v).to(cuda)
    _, cs = scales_at(rows, ctr, coeff.to(cuda), 1.0)
    a = step_fused(rows, c.to(cuda), ctr, v.to(cuda), cs)
    b = step_fused(rows, c.to(cuda), ctr, v.to(cuda), cs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # in place: v_out over v_in, ctr_out over ctr_in
    vi, ci = v.to(cuda), ctr.clone()
    sq = Fn.cc_step(rows, c.to(cuda), ci, vi, cs, vi, ci)
    assert torch.equal(vi, a[0]) and torch.equal(ci, a[1]) and torch.equal(sq, a[2])
    with pytest.raises(ValueError):
        Fn.cc_step(torch.zeros(17, 8, device=cuda), None, ctr[:8], ctr[:8], torch.zeros(17, device=cuda),
                   torch.empty(8, device=cuda), torch.empty(8, device=cuda))


# ------------------------------------------------------------------------------------- 2: limits
def call(agg, rows, coeff, c, dev, K=None):
    out = torch.empty(rows.shape[1], device=dev)
    agg(DistContext(), rows, coeff.to(dev), out, center=None if c is None else c.to(dev),
        counts=[rows.shape[0] if K is None else K])
    return out


def check_limits(dev, fuse):
    G, n = 7, 1027
    X, c, coeff, v = problem(G, n, 77, True)
    rows = X.to(dev)
    # tau = inf, one iteration, v = 0: the weighted mean
    agg = A.make_aggregator("cc", tau=math.inf, iters=1)
    agg.fuse = fuse
    assert agg.name == "centered_clip" and agg.takes_center and not agg.needs_all
    out = call(agg, rows, coeff, c, dev)
    want, mass, _ = C.clipped_sum(X, c, coeff, 1e30)
    err = np.abs(out.cpu().double().numpy() - (C._f64(c) + want))
    assert bool((err <= C.sum_bound(G, c, mass)).all())
    nrm, ref = np.array(agg.last_norms), C.norms(X, c)
    assert bool((np.abs(nrm - ref) <= EPS23 * ref).all())
    assert agg.state_dict()["rounds"] == 1 and agg.last_k == G and agg.epsilon(100, 1e-5) == math.inf
    # no iteration: the centre plus the carried v
    agg = A.CenteredClip(1.0, iters=0)
    agg.fuse = fuse
    agg.load_state_dict({"rounds": 0, "last_k": 0, "v": v})
    assert torch.equal(call(agg, rows, coeff, c, dev).cpu(), c + v)
    assert torch.equal(call(agg, rows - c.to(dev), coeff, None, dev).cpu(), v)
    # a row of NaN / Inf is dropped in every iteration: the bits of the run without it
    for bad in (float("nan"), float("inf"), float("-inf")):
        Xb = X.clone()
        Xb[3, 500] = bad
        keep = [k for k in range(G) if k != 3]
        a, b = A.CenteredClip(0.8, iters=3), A.CenteredClip(0.8, iters=3)
        a.fuse = b.fuse = fuse
        got = call(a, Xb.to(dev), coeff, c, dev)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, call(b, X[keep].to(dev), coeff[keep], c, dev)), bad
        assert not math.isfinite(a.last_norms[3])
    with pytest.raises(ValueError):
        A.CenteredClip(0.0)
    with pytest.raises(ValueError):
        A.CenteredClip(1.0, iters=-1)


def check_zero_weight_rows_are_not_read(dev):
    X, c, coeff, v = problem(5, 1027, 9, True)
    X[1] = float("nan")
    cs = torch.tensor([0.2, 0.0, 0.3, 0.0, 0.1])
    X[3] = float("nan")
    ctr = c + v
    for step in (step_fused, step_unfused):
        v_out, ctr_out, sq = step(X.to(dev), c.to(dev), ctr.to(dev), v.to(dev), cs.to(dev))
        assert bool(torch.isfinite(v_out).all()) and bool(torch.isfinite(ctr_out).all())
        if step is step_fused:
            assert sq.cpu().tolist()[1] == math.inf and sq.cpu().tolist()[3] == math.inf
        assert bool(torch.isfinite(sq.cpu()[[0, 2, 4]]).all())


@pytest.mark.parametrize("fuse", [True, False])
def test_limits(cuda, fuse):
    check_limits(cuda, fuse)


def test_zero_weight_rows_are_not_read(cuda):
    check_zero_weight_rows_are_not_read(cuda)


# --------------------------------------------------------------------------------- 3: aggregator
def iterate(step, rows, c_dev, coeff, v, tau, L):
    """L steps from v on one route -> (v^L, ctr^L, first norms, [(v^l, ctr^l) before each step])."""
    ctr = v.clone() if c_dev is None else torch.empty_like(v)
    if c_dev is not None:
        Fn.apply_update(ctr, c_dev, v)
    sq = Fn.update_sqnorm(rows, ctr)
    first, trace = None, []
    for l in range(L):
        norms, cs = Fn.clip_scales(sq, coeff, tau)
        first = norms if l == 0 else first
        trace.append((v, ctr))
        v, ctr, sq = step(rows, c_dev, ctr, v, cs, l < L - 1)
        if sq is None and l < L - 1:
            sq = Fn.update_sqnorm(rows, ctr)
    return v, ctr, first, trace


def check_aggregator(dev, fused):
    """``fused``: the route under test (a GPU with G <= 16 takes the fused one; everything else the
    unfused one whatever ``fuse`` says)."""
    G, n, tau, L = 8, 1027, 0.7, 3
    X, c, coeff, _ = problem(G, n, 21, False)
    rows, c_dev, cf = O.strided(X, dev), c.to(dev), coeff.to(dev)
    step = step_fused if fused else step_unfused
    for weighting in ("samples", "uniform"):
        used = cf if weighting == "samples" else torch.full((G,), 1.0 / G, device=dev)
        agg = A.CenteredClip(tau, L, weighting)
        agg.fuse = fused
        v = torch.zeros(n, device=dev)
        for rnd in range(2):  # the second round starts from the first one's v
            out = call(agg, rows, coeff, c, dev)
            v, ctr, first, _ = iterate(step, rows, c_dev, used, v, tau, L)
            assert torch.equal(out, ctr) and torch.equal(agg.v, v), (weighting, rnd)
            assert agg.last_norms == first.tolist()
        assert agg.rounds == 2 and agg.last_k == G
    # in place over the centre, as FedAvg calls it
    a, b = A.CenteredClip(tau, L), A.CenteredClip(tau, L)
    a.fuse = b.fuse = fused
    w = c_dev.clone()
    assert a(DistContext(), rows, cf, w, center=w, counts=[G]) is w
    assert torch.equal(w, call(b, rows, coeff, c, dev))
    # warm_start=False forgets v; state_dict carries it
    cold = A.CenteredClip(tau, L, warm_start=False)
    cold.fuse = fused
    first = call(cold, rows, coeff, c, dev)
    assert torch.equal(first, call(cold, rows, coeff, c, dev))
    warm = A.CenteredClip(tau, L)
    warm.fuse = fused
    assert torch.equal(first, call(warm, rows, coeff, c, dev)) and not torch.equal(first, call(warm, rows, coeff, c, dev))
    sd = a.state_dict()
    assert sd["rounds"] == 1 and sd["v"].device.type == "cpu" and torch.equal(sd["v"], a.v.cpu())
    fresh = A.CenteredClip(tau, L)
    fresh.fuse = fused
    fresh.load_state_dict(sd)
    assert torch.equal(call(fresh, rows, coeff, c, dev), call(a, rows, coeff, c, dev))
    assert A.CenteredClip(tau, L).state_dict() == {"rounds": 0, "last_k": 0, "v": None}


def check_routes_agree(dev):
    """The fused order of the sum (``Fn.cc_step``) against the unfused route: within twice the
    one-step bound summed over the L steps. A step hands on v_out and ctr_out = fl32(c + v_out), and
    the next step subtracts ctr from every row, so what one step can add to the distance of the two
    routes is the bound of its ctr_out, ``sum_bound`` and one more 2^-24 |c + v| (the rounding at the
    magnitude of the centre, which re-enters v with weight sum_k cs_k <= 1); each route may be that
    far from the exact step, hence twice."""
    G, n, tau, L = 8, 1027, 0.7, 3
    X, c, coeff, _ = problem(G, n, 23, False)
    rows, c_dev, cf = X.to(dev), c.to(dev), coeff.to(dev)
    vf, cf_out, _, trace = iterate(step_fused, rows, c_dev, cf, torch.zeros(n, device=dev), tau, L)
    agg = A.CenteredClip(tau, L)
    agg.fuse = False
    out = call(agg, rows, coeff, c, dev)
    bound = np.zeros(n)
    for v_l, ctr_l in trace:
        _, mass, _ = C.clipped_sum(X, ctr_l.cpu(), coeff, tau)
        bound += 2 * (C.sum_bound(G, v_l.cpu(), mass) + EPS24 * np.abs(C._f64(ctr_l)))
    err = np.abs(C._f64(agg.v) - C._f64(vf))
    print(f"routes: worst err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    err = np.abs(C._f64(out) - C._f64(cf_out))
    assert bool((err <= bound).all())
    if dev.type == "cuda":  # the aggregator's two routes themselves
        fused = A.CenteredClip(tau, L)
        assert torch.equal(call(fused, rows, coeff, c, dev), cf_out)


@pytest.mark.parametrize("fused", [True, False])
def test_aggregator(cuda, fused):
    check_aggregator(cuda, fused)


def test_routes_agree(cuda):
    check_routes_agree(cuda)


# ------------------------------------------------------- 4: it defends where the mean does not
def check_defends_against_ipm(dev, fuse):
    """8 clients, 2 of them sending -100 x the benign mean: the plain mean points against the benign
    mean (-24 |mu|^2); three centered-clipping steps of radius the median benign norm point along it."""
    K, f, P = 8, 2, 4096
    g = torch.Generator().manual_seed(1)
    grad = torch.randn(P, generator=g) / math.sqrt(P)
    U = grad + 0.5 * torch.randn(K, P, generator=g) / math.sqrt(P)
    mu = U[f:].double().mean(0)
    U[:f] = (-100.0 * mu).float()
    mean = U.double().mean(0)
    assert float(mean @ mu) < -20 * float(mu @ mu)
    tau = float(U[f:].double().norm(dim=1).median())
    agg = A.CenteredClip(tau, iters=1, weighting="uniform")
    agg.fuse = fuse
    prev = torch.zeros(P, dtype=torch.float64)
    rows = U.to(dev)
    for l in range(3):  # one iteration per call from the carried v: the three steps of iters = 3
        v = call(agg, rows, torch.full((K,), 1.0 / K), None, dev).cpu().double()
        assert float((v - prev).norm()) <= tau * (1 + 2.0 ** -20), l
        prev = v
    once = A.CenteredClip(tau, iters=3, weighting="uniform")
    once.fuse = fuse
    assert torch.equal(call(once, rows, torch.full((K,), 1.0 / K), None, dev).cpu().double(), v)
    cos = float(v @ mu) / float(mu @ mu)
    rel = float((v - mu).norm() / mu.norm())
    print(f"centered clipping: <v, mu> / |mu|^2 = {cos:.3f}, |v - mu| / |mu| = {rel:.3f}")
    assert cos > 0


@pytest.mark.parametrize("fuse", [True, False])
def test_defends_against_ipm(cuda, fuse):
    check_defends_against_ipm(cuda, fuse)
