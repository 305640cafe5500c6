"""The geometric median / RFA (``GeometricMedian``; csrc/kernels/clip_agg.hip: ``ddl_gm_scales`` and the
centered-clipping step it drives) against the float64 oracle of tests/geomed_oracle.py.

The ``check_*`` functions take the device, so tests/test_geomed_cpu.py runs the same cases on the
torch twins; here they run on the kernels."""
import math

import numpy as np
import pytest
import torch

import clip_oracle as C
import geomed_oracle as GO
import robust_oracle as O
import test_centered_clip_gpu as CC
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

SCALES_G = (1, 2, 5, 16, 17, 33, 300)
FUSED_G = (1, 4, 5, 16)
UNFUSED_G = (5, 17, 33)
INFLUENCE_KF = ((9, 2), (16, 3), (33, 8))
EPS24 = 2.0 ** -24
NU = 1e-6


# ------------------------------------------------------------------------------------ 1: gm_scales
def one_ulp(got, want64):
    """got fp32 within one fp32 ulp of the float64 value rounded to fp32; non-finite values alike."""
    got = got.cpu().numpy()
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    fin = np.isfinite(want)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    with np.errstate(invalid="ignore"):  # inf - inf, spacing(inf): those entries take `same`
        near = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))
    return bool(np.where(fin, near, same).all())


def check_gm_scales(G, dev):
    g = torch.Generator().manual_seed(G)
    rows = torch.randn(G, 1, generator=g).exp() * torch.randn(G, 40, generator=g)
    sq = rows.double().square().sum(1)
    if G >= 5:
        sq[1], sq[2], sq[3] = float("nan"), float("inf"), 0.0
    elif G == 2:
        sq[1] = 0.0  # the nu floor: beta = coeff / nu, finite
    dead = ~torch.isfinite(sq)
    coeff = torch.rand(G, generator=g) + 0.1
    coeff /= coeff.sum()
    for init in (False, True):
        S0 = GO.scales(sq.numpy(), coeff, NU, init)[2]
        for total in (None, 1.7 * S0):
            tag = f"G={G} init={init} total={total}"
            t_dev = None if total is None else torch.tensor([total], dtype=torch.float64, device=dev)
            norms, cs, bs = Fn.gm_scales(sq.to(dev), coeff.to(dev), NU, init, t_dev)
            want_n, want_cs, S = GO.scales(sq.numpy(), coeff, NU, init, total)
            assert norms.dtype == cs.dtype == torch.float32 and bs.dtype == torch.float64 and bs.numel() == 1
            assert one_ulp(norms, want_n), f"norms {tag}"
            assert one_ulp(cs, want_cs), f"cs {tag}"
            assert abs(float(bs.cpu()) - S) <= G * 2.0 ** -52 * S, f"beta_sum {tag}"
            assert bool((cs.cpu()[dead] == 0).all()), f"dropped rows {tag}"
            if total is None:
                assert abs(float(cs.cpu().double().sum()) - 1.0) <= G * EPS24, f"sum of cs {tag}"
        _, cs, bs = Fn.gm_scales(sq.to(dev), torch.zeros(G, device=dev), NU, init)
        assert bool((cs.cpu() == 0).all()) and float(bs.cpu()) == 0.0
    with pytest.raises(ValueError):
        Fn.gm_scales(sq.to(dev), coeff.to(dev), 0.0)


@pytest.mark.parametrize("G", SCALES_G)
def test_gm_scales(cuda, G):
    check_gm_scales(G, cuda)


# ---------------------------------------------------------------------- 2: aggregator = its ops
def compose(rows, c_dev, coeff, iters, init, fused, scales=None):
    """``GeometricMedian``'s op sequence by hand on one route -> (out, first norms, last cs,
    [(v^l, ctr^l, cs^l) before each step]). ``scales``: the cs of every step, instead of gm_scales."""
    n = rows.shape[1]
    v = torch.zeros(n, device=rows.device)
    ctr = v.clone() if c_dev is None else torch.empty_like(v)
    if c_dev is not None:
        Fn.apply_update(ctr, c_dev, v)
    steps = [True] * (init == "mean") + [False] * iters
    first = cs = sq = None
    trace = []
    for l, mean_step in enumerate(steps):
        if scales is not None:
            cs = scales[l]
        else:
            if sq is None:
                sq = Fn.update_sqnorm(rows, ctr)
            norms, cs, _ = Fn.gm_scales(sq, coeff, NU, mean_step)
            first = norms if l == 0 else first
        trace.append((v, ctr, cs))
        v, ctr, sq = (CC.step_fused if fused else CC.step_unfused)(rows, c_dev, ctr, v, cs, fused and l < len(steps) - 1)
    return ctr, first, cs, trace


def check_aggregator_is_its_ops(G, dev, fuse):
    """``fuse``: the aggregator's switch; the fused route is taken on a GPU with G <= 16 only."""
    fused = fuse and dev.type == "cuda" and G <= Fn.CC_MAX_ROWS
    for n in (5, 1027):
        X, c, coeff, _ = CC.problem(G, n, 41 * G + n, False)
        for with_c in (True, False):
            rows = O.strided(X if with_c else X - c, dev)
            c_dev = c.to(dev) if with_c else None
            for init, weighting in (("zero", "samples"), ("mean", "samples"), ("zero", "uniform")):
                tag = f"G={G} n={n} centre={with_c} {init} {weighting} fused={fused}"
                agg = A.GeometricMedian(3, NU, weighting, init)
                agg.fuse = fuse
                out = CC.call(agg, rows, coeff, c if with_c else None, dev)
                used = coeff.to(dev) if weighting == "samples" else torch.full((G,), 1.0 / G, device=dev)
                want, first, cs, _ = compose(rows, c_dev, used, 3, init, fused)
                assert torch.equal(out, want), tag
                assert agg.last_norms == first.tolist() and agg.last_weights == cs.tolist(), tag
                assert agg.rounds == 1 and agg.last_k == G
    # in place over the centre, as FedAvg calls it
    a, b = A.GeometricMedian(), A.GeometricMedian()
    a.fuse = b.fuse = fuse
    rows, w = X.to(dev), c.to(dev).clone()
    assert a(CC.DistContext(), rows, coeff.to(dev), w, center=w, counts=[G]) is w
    assert torch.equal(w, CC.call(b, rows, coeff, c, dev))


def check_routes_agree(dev):
    """The fused and the unfused order of the sum on the same per-step scales (those of the fused
    run): within the bound ``test_centered_clip_gpu.check_routes_agree`` sums, per step
    2 * (sum_bound + 2^-24 |ctr|)."""
    G, n, L = 8, 1027, 3
    X, c, coeff, _ = CC.problem(G, n, 43, False)
    rows, c_dev = X.to(dev), c.to(dev)
    out_f, _, _, trace = compose(rows, c_dev, coeff.to(dev), L, "zero", True)
    out_u, _, _, trace_u = compose(rows, c_dev, None, L, "zero", False, scales=[t[2] for t in trace])
    bound = np.zeros(n)
    for v_l, ctr_l, cs_l in trace:
        mass = (np.abs(C.updates(X, ctr_l.cpu())) * np.abs(C._f64(cs_l))[:, None]).sum(0)
        bound += 2 * (C.sum_bound(G, v_l.cpu(), mass) + EPS24 * np.abs(C._f64(ctr_l)))
    err = np.abs(C._f64(out_u) - C._f64(out_f))
    print(f"geomed routes: worst err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("G", FUSED_G)
def test_aggregator_is_its_ops_fused(cuda, G):
    check_aggregator_is_its_ops(G, cuda, True)


@pytest.mark.parametrize("G", UNFUSED_G)
def test_aggregator_is_its_ops_unfused(cuda, G):
    check_aggregator_is_its_ops(G, cuda, False)


def test_routes_agree(cuda):
    check_routes_agree(cuda)


# ------------------------------------------------------------------------------- 3: fixed points
def check_fixed_points(dev, fuse):
    G, n = 5, 1027
    X, c, coeff, _ = CC.problem(G, n, 47, False)
    # identical rows give that row
    same = X[2].repeat(G, 1)
    agg = A.GeometricMedian()
    agg.fuse = fuse
    out = CC.call(agg, same.to(dev), coeff, c, dev)
    bound = C.sum_bound(G, c, np.abs(C.updates(X[2:3], c))[0])
    assert bool((np.abs(C._f64(out) - C._f64(X[2])) <= bound).all())
    # no iteration: the centre, or with init="mean" the weighted mean
    agg = A.GeometricMedian(iters=0)
    agg.fuse = fuse
    assert torch.equal(CC.call(agg, X.to(dev), coeff, c, dev).cpu(), c)
    assert not bool(CC.call(agg, (X - c).to(dev), coeff, None, dev).any())
    agg = A.GeometricMedian(iters=0, init="mean")
    agg.fuse = fuse
    out = CC.call(agg, X.to(dev), coeff, c, dev)
    want, b, _ = GO.geomed(X, c, coeff, 0, NU, "mean")
    mass = (np.abs(C.updates(X, c)) * b[:, None]).sum(0)
    assert bool((np.abs(C._f64(out) - want) <= C.sum_bound(G, c, mass)).all())
    # the geometric median of collinear points is their median
    g = torch.Generator().manual_seed(3)
    x, e, c3 = torch.randn(64, generator=g), torch.randn(64, generator=g), torch.randn(64, generator=g)
    e /= e.norm()
    rows3 = torch.stack([x, x + e, x + 10 * e])
    third = torch.full((3,), 1.0 / 3)
    want = GO.geomed(rows3, c3, third, 30, NU)[0]
    assert np.linalg.norm(want - C._f64(x + e)) <= 1e-3  # |e| = 1: the oracle meets it first
    agg = A.GeometricMedian(iters=30, weighting="uniform")
    agg.fuse = fuse
    out = CC.call(agg, rows3.to(dev), third, c3, dev)
    assert float((out.cpu().double() - (x + e).double()).norm()) <= 1e-3
    for kw in ({"iters": -1}, {"nu": 0.0}, {"init": "median"}, {"weighting": "equal"}):
        with pytest.raises(ValueError):
            A.GeometricMedian(**kw)
    for name in ("geomed", "rfa", "geometric_median"):
        agg = A.make_aggregator(name, gm_iters=2, gm_nu=1e-5, weighting="uniform")
        assert (agg.name, agg.iters, agg.nu, agg.weighting, agg.init) == ("geomed", 2, 1e-5, "uniform", "zero")
        assert agg.takes_center and not agg.needs_all and agg.state_dict() == {"rounds": 0, "last_k": 0}


@pytest.mark.parametrize("fuse", [True, False])
def test_fixed_points(cuda, fuse):
    check_fixed_points(cuda, fuse)


# -------------------------------------------------------------------------- 4: bounded influence
def check_bounded_influence(K, f, dev, fuse):
    """From the centre, three iterations stay within one honest radius of the honest mean whatever
    the magnitude of the f bad rows (the oracle sits near f / (K - f)); from the mean they do not."""
    n = 300
    c = torch.full((n,), 0.9)
    uni = torch.full((K,), 1.0 / K)
    for where in O.PLACEMENTS:
        outs, wants = [], []
        for value in (100.0, 1e30, 3e38):
            X, honest, bad = O.attack_rows(K, f, n, "1e30", where)
            X[bad] = value
            hm = X[honest].double().mean(0)
            radius = float((X[honest].double() - hm).norm(dim=1).max())
            tag = f"K={K} f={f} {value:g} {where}"
            want = torch.from_numpy(GO.geomed(X, c, uni, 3, NU)[0])
            assert float((want - hm).norm()) <= 1.0 * radius, f"oracle {tag}"
            agg = A.GeometricMedian(3, NU, "uniform")
            agg.fuse = fuse
            out = CC.call(agg, X.to(dev), uni, c, dev).cpu().double()
            dist = float((out - hm).norm()) / radius
            print(f"geomed {tag}: {dist:.3f} honest radii from the honest mean (oracle {float((want - hm).norm()) / radius:.3f})")
            assert dist <= 1.0, tag
            outs.append(out)
            wants.append(want)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert float((wants[a] - wants[b]).norm()) <= 1e-4 * radius
            assert float((outs[a] - outs[b]).norm()) <= 1e-4 * radius, f"K={K} f={f} {where}: magnitudes {a}, {b}"
        for kind in ("nan", "+inf", "one_nan"):
            X, honest, bad = O.attack_rows(K, f, n, kind, where)
            agg = A.GeometricMedian(3, NU, "uniform")
            agg.fuse = fuse
            out = CC.call(agg, X.to(dev), uni, c, dev).cpu()
            w = agg.last_weights
            assert bool(torch.isfinite(out).all()) and all(w[k] == 0.0 for k in bad) and all(w[k] > 0 for k in honest)
            assert all(not math.isfinite(agg.last_norms[k]) for k in bad)
    # why the default start is the centre: from the mean, rows of 100 already carry the result off
    X, honest, bad = O.attack_rows(K, f, n, "1e30", "first")
    X[bad] = 100.0
    hm = X[honest].double().mean(0)
    radius = float((X[honest].double() - hm).norm(dim=1).max())
    want = torch.from_numpy(GO.geomed(X, c, uni, 3, NU, "mean")[0])
    assert float((want - hm).norm()) > 1.0 * radius
    agg = A.GeometricMedian(3, NU, "uniform", "mean")
    agg.fuse = fuse
    out = CC.call(agg, X.to(dev), uni, c, dev).cpu().double()
    assert float((out - hm).norm()) > 1.0 * radius


@pytest.mark.parametrize("K,f", INFLUENCE_KF)
def test_bounded_influence(cuda, K, f):
    check_bounded_influence(K, f, cuda, True)  # 9 and 16 rows fused, 33 unfused
