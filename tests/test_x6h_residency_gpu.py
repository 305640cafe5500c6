"""Halo kernel at three workgroups per CU (csrc/kernels/conv_x6h.hip, the 26,624-byte halo tier of
the BP 64 instances): the instances that moved compute, bit for bit, what the untouched BP 128
instance computes on the same geometry (the reduction order of an output element is chunk-outer,
tap-inner whatever BP is), a geometry whose halo does not fit the tier still runs, the occupancy
query gives three per CU for the moved instances and the old value for the others, and a graph of
a FWD plus a fused DGRAD replays to equal bits.

The padded-width (PADW) 1x1 case is 16 rows of 14 pixels: the kernel's tiles are whole rows, 128 / 16 = 8
padded rows per tile, and it declines images whose height is not a multiple of that (14x14), so the
smallest image with rows of 14 that reaches the PADW instances is 16 tall. The 3x3 DGRAD at BP 64 has
no instance on the new tier (it would spill); its cases compare two instances that did not change.
"""
import pytest
import torch

from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.ops import functional_f32 as F32
from ddl25spring_amd.ops.functional import ConvGeom

from test_fp32_gpu import _close, _weights, ref_dgrad, ref_fwd

pytestmark = pytest.mark.gpu

FWD, DGRAD = F32.F_FWD, F32.F_DGRAD
TINY, SMALL, LARGE = F32.HALO_TINY, F32.HALO_SMALL, F32.HALO_LARGE

GEOMS = [
    ConvGeom(G=2, N=3, H=32, W=32, C=64, K=64, R=3, S=3, stride=1, pad=1),   # one segment; tiles cross images
    ConvGeom(G=1, N=5, H=16, W=16, C=128, K=64, R=3, S=3, stride=1, pad=1),  # a ragged last tile
    ConvGeom(G=2, N=4, H=8, W=8, C=64, K=128, R=3, S=3, stride=1, pad=1),    # two segments; two P tiles (FWD)
    ConvGeom(G=1, N=2, H=16, W=14, C=32, K=64, R=1, S=1, stride=1, pad=0),   # PADW (rows of 14 padded to 16)
    ConvGeom(G=2, N=2, H=16, W=16, C=64, K=64, R=1, S=1, stride=1, pad=0),
    # DGRAD with two P tiles at BP 64: dyb_out is written by the first P tile only
    ConvGeom(G=2, N=4, H=8, W=8, C=128, K=64, R=3, S=3, stride=1, pad=1),
]
IDS = [f"{g.C}x{g.K}_{g.H}x{g.W}_{g.R}n{g.N}" for g in GEOMS]


@pytest.fixture(autouse=True)
def _x6():
    old = F32.math()
    F32.set_math("x6")
    yield
    F32.set_math(old)


def _both(mode, g, fn):
    """fn() under the pinned BP 64 plan, then under BP 128 -> (outputs at 64, outputs at 128)."""
    outs = []
    try:
        for bp in (64, 128):
            F32.set_plan(mode, g, bp, 128, 1, "x6h")
            assert F32.uses_halo(mode, g)
            outs.append(fn())
    finally:
        F32.clear_plan(mode, g)
    return outs


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_fwd_bp64_equals_bp128(cuda, geom):
    g = geom
    torch.manual_seed(11)
    x = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    w = _weights(g, cuda)
    sc = torch.rand(g.G, g.C, device=cuda) + 0.5
    sh = torch.randn(g.G, g.C, device=cuda) * 0.3
    bias = torch.randn(g.G, g.K, device=cuda)
    res = torch.randn(g.G, g.N, g.P, g.Q, g.K, device=cuda)

    def run():
        st, st2 = F32.SlotStats(), F32.SlotStats()
        y1 = Fn.conv_fwd(x, w, g, stats=st, in_bn=(sc, sh))          # operand BN + ReLU, statistics
        y2 = Fn.conv_fwd(x, w, g, bias=bias, relu=True, residual=res, stats=st2)
        y3 = Fn.conv_fwd(x, w, g)
        return y1, st.t, y2, st2.t, y3

    a, b = _both(FWD, g, run)
    _same(a, b)
    xa = (x.double() * sc.double()[:, None, None, None] + sh.double()[:, None, None, None]).clamp_min(0)
    _close(a[0], ref_fwd(xa.cpu(), w.cpu(), g))


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_dgrad_bp64_equals_bp128(cuda, geom):
    g = geom
    torch.manual_seed(12)
    dy = torch.randn(g.G, g.N, g.P, g.Q, g.K, device=cuda)
    xb = torch.randn_like(dy)
    coef = torch.randn(g.G, 3, g.K, device=cuda)
    w = _weights(g, cuda)
    res = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    mask = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    bx = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    mean = torch.randn(g.G, g.C, device=cuda) * 0.1
    rstd = torch.rand(g.G, g.C, device=cuda) + 0.5
    sc = torch.rand(g.G, g.C, device=cuda) + 0.5
    sh = torch.randn(g.G, g.C, device=cuda) * 0.2
    even = g.H % 2 == 0
    rc = torch.randn(g.G, g.N, (g.H + 1) // 2, (g.W + 1) // 2, g.C, device=cuda)

    def run():
        d1 = Fn.conv_dgrad(dy, w, g)
        dc = torch.full_like(dy, float("nan"))
        d2 = Fn.conv_dgrad(dy, w, g, dy_bn=(xb, coef), dy_bn_out=dc)
        d3, p3 = Fn.conv_dgrad(dy, w, g, residual=res, mask=mask, bn=(bx, mean, rstd))
        d4, p4 = Fn.conv_dgrad(dy, w, g, bn=(bx, mean, rstd), mask_bn=(sc, sh))
        out = [d1, d2, dc, d3, p3, d4, p4]
        if even:
            out += list(Fn.conv_dgrad(dy, w, g, residual=rc, residual_sub=2, mask=mask, bn=(bx, mean, rstd)))
        return out

    a, b = _both(DGRAD, g, run)
    _same(a, b)
    _close(a[0], ref_dgrad(dy.cpu(), w.cpu(), g))
    c = coef.cpu().double()
    _close(a[2], c[:, 0, None, None, None] * dy.cpu().double() + c[:, 1, None, None, None] * xb.cpu().double()
           + c[:, 2, None, None, None], rel=1e-6)


def test_tiers_of_the_shapes(cuda):
    """The shapes above reach the new tier where an instance has one, and every layout is the one
    the search finds without the tier (the tier never changes ROWB / SEGB)."""
    for g in GEOMS:
        for mode in (FWD, DGRAD):
            lay = F32.halo_layout(mode, g, 64)
            assert lay is not None and lay["HP"] <= 208
            has = F32.halo_residency(mode, 64, g.R, TINY, g.Q & (g.Q - 1) != 0) > 0
            assert lay["tier"] == (TINY if has and lay["HBYTES"] <= TINY else SMALL)
            assert F32.halo_layout(mode, g, 128)["tier"] == SMALL
            assert {k: lay[k] for k in ("ROWB", "SEGB")} == {k: F32.halo_layout(mode, g, 128)[k] for k in ("ROWB", "SEGB")}
    assert F32.halo_layout(FWD, GEOMS[0], 64)["tier"] == TINY
    assert F32.halo_layout(FWD, GEOMS[1], 64)["tier"] == TINY
    assert F32.halo_layout(DGRAD, GEOMS[4], 64)["tier"] == TINY


def _no_fit_geom():
    """A BP 64 geometry whose halo does not fit the new tier (chosen from the layout search)."""
    cands = [ConvGeom(G=1, N=3, H=64, W=64, C=32, K=64, R=3, S=3, stride=1, pad=1),  # 264 halo pixels
             ConvGeom(G=1, N=9, H=4, W=4, C=32, K=64, R=3, S=3, stride=1, pad=1),    # 8 segments
             ConvGeom(G=1, N=4, H=8, W=8, C=32, K=64, R=3, S=3, stride=1, pad=1)]
    for g in cands:
        lay = F32.halo_layout(FWD, g, 64)
        if lay is not None and lay["tier"] != TINY:
            return g, lay
    raise AssertionError("no candidate misses the tier")


def test_geometry_past_the_tier_still_launches(cuda):
    g, lay = _no_fit_geom()
    assert lay["HBYTES"] > TINY or lay["HP"] > 208
    torch.manual_seed(13)
    x = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    dy = torch.randn(g.G, g.N, g.P, g.Q, g.K, device=cuda)
    w = _weights(g, cuda)
    try:
        F32.set_plan(FWD, g, 64, 128, 1, "x6h")
        F32.set_plan(DGRAD, g, 64, 128, 1, "x6h")
        _close(Fn.conv_fwd(x, w, g), ref_fwd(x.cpu(), w.cpu(), g))
        _close(Fn.conv_dgrad(dy, w, g), ref_dgrad(dy.cpu(), w.cpu(), g))
    finally:
        F32.clear_plan(FWD, g)
        F32.clear_plan(DGRAD, g)


def test_residency(cuda):
    """Three workgroups per CU for every instance of the new tier; two (BP 128, 32 KiB halo) and
    one (BP 128, 45,056-byte halo) as before for the instances that did not move; no BP 128
    instance of the new tier."""
    moved = [(mode, rs, padw) for mode in (FWD, DGRAD) for rs in (1, 3) for padw in (False, True)
             if F32.halo_residency(mode, 64, rs, TINY, padw) >= 0]
    assert (FWD, 3, False) in moved and (FWD, 1, False) in moved and (DGRAD, 1, False) in moved
    for mode, rs, padw in moved:
        assert F32.halo_residency(mode, 64, rs, TINY, padw) >= 3, (mode, rs, padw)
    assert F32.halo_residency(FWD, 128, 3, SMALL) == 2
    assert F32.halo_residency(DGRAD, 128, 3, LARGE) == 1
    assert F32.halo_residency(FWD, 64, 3, LARGE) == 2
    assert F32.halo_residency(FWD, 128, 3, TINY) == -1


def test_graph_replay(cuda):
    """A FWD plus a fused DGRAD of the first shape in one graph: two replays give equal bits."""
    g = GEOMS[0]
    torch.manual_seed(14)
    x = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    dy = torch.randn(g.G, g.N, g.P, g.Q, g.K, device=cuda)
    w = _weights(g, cuda)
    sc = torch.rand(g.G, g.C, device=cuda) + 0.5
    sh = torch.randn(g.G, g.C, device=cuda) * 0.3
    res = torch.randn(g.G, g.N, g.H, g.W, g.C, device=cuda)
    mask = torch.randn_like(res)
    bx = torch.randn_like(res)
    mean = torch.randn(g.G, g.C, device=cuda) * 0.1
    rstd = torch.rand(g.G, g.C, device=cuda) + 0.5
    try:
        F32.set_plan(FWD, g, 64, 128, 1, "x6h")
        F32.set_plan(DGRAD, g, 64, 128, 1, "x6h")
        F32.ensure_workspace(cuda)

        def run():
            st = F32.SlotStats()
            y = Fn.conv_fwd(x, w, g, stats=st, in_bn=(sc, sh))
            dx, part = Fn.conv_dgrad(dy, w, g, residual=res, mask=mask, bn=(bx, mean, rstd))
            return y, st.t, dx, part

        eager = [t.clone() for t in run()]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run()
        graph.replay()
        torch.cuda.synchronize()
        first = [t.clone() for t in outs]
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same(first, outs)
        _same(first, eager)
    finally:
        F32.clear_plan(FWD, g)
        F32.clear_plan(DGRAD, g)
