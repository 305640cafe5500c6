"""conv_x6hw.hip, the pipelined halo WGRAD: staging waves fill one LDS stage while the compute
waves run the MFMAs of the other, over 64-pixel tiles; 4-wide images read two halo rows per lane.

Every case runs on the halo engine only (a fall-back to conv_f32.hip fails the test), in both call
forms (plain; accumulating with a gscale and the operand-side BN + ReLU of X), against float64 on
the CPU at the suite's fp32 tolerance, and twice (bitwise repeatable).

A tile is 64 output pixels, so an image of 16x16 is 4 tiles, 32x32 is 16, 8x8 is one, and a tile
holds four 4x4 images: partial last tiles arise on 4-wide images only (N not a multiple of 4 at 4x4,
N = 3 at 8x4). Slices are cut in units of two tiles (128 pixels), so a slice with an odd tile count
is the last one that holds any."""
import ctypes

import pytest
import torch

from ddl25spring_amd.ops import _lib
from ddl25spring_amd.ops import functional_f32 as F32
from ddl25spring_amd.ops.functional import ConvGeom

from test_fp32_gpu import _close, ref_wgrad

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _halo_engine_only(monkeypatch):
    old = F32.math()
    F32.set_math("x6")
    monkeypatch.setattr(F32, "HALO_WGRAD", [True])
    monkeypatch.setattr(F32, "HW_MIN_W", 0)  # every geometry the kernel takes

    def no_fallback(*args, **kw):
        raise AssertionError("conv_wgrad fell back to conv_f32.hip")
    monkeypatch.setattr(F32, "_launch", no_fallback)
    yield
    F32.set_math(old)


def g3(G, N, H, W, C, K):
    return ConvGeom(G=G, N=N, H=H, W=W, C=C, K=K, R=3, S=3, stride=1, pad=1)


def g1(G, N, H, W, C, K):
    return ConvGeom(G=G, N=N, H=H, W=W, C=C, K=K, R=1, S=1, stride=1, pad=0)


def _tiles(geom):
    """64-pixel tiles per group, after checking that the halo WGRAD takes the geometry."""
    a = F32._args(geom)
    assert _lib.kernels().ddl_x6hw_ok(ctypes.byref(a)), "geometry must take the halo WGRAD"
    assert F32.uses_halo_wgrad(geom)
    ntile = -(-geom.N * geom.H * geom.W // 64)
    assert int(_lib.kernels().ddl_x6hw_tiles(ctypes.byref(a))) == -(-ntile // 2)  # the planner's 128-pixel units
    return ntile


def _inputs(geom, cuda, ramp=False):
    torch.manual_seed(3)
    x = torch.randn(geom.G, geom.N, geom.H, geom.W, geom.C, device=cuda)
    if ramp:
        # every pixel of every image its own value (border pixels included), times a per-channel factor:
        # a window shifted by one column or row changes the result at first order
        pix = torch.arange(geom.N * geom.H * geom.W, dtype=torch.float32, device=cuda).view(1, geom.N, geom.H, geom.W, 1)
        x = (1.0 + pix) * (0.5 + torch.rand(geom.G, 1, 1, 1, geom.C, device=cuda))
    dy = torch.randn(geom.G, geom.N, geom.P, geom.Q, geom.K, device=cuda)
    sc = torch.rand(geom.G, geom.C, device=cuda) + 0.5
    sh = torch.randn(geom.G, geom.C, device=cuda) * 0.3
    w0 = torch.randn(geom.G, geom.K, geom.R, geom.S, geom.C, device=cuda)
    return x, dy, sc, sh, w0


def _refs(geom, x, dy, sc, sh, w0):
    """The two float64 results, computed once per geometry and shared by its splits."""
    ref = ref_wgrad(dy.cpu(), x.cpu(), geom)
    b = lambda t: t.cpu().double()[:, None, None, None]  # noqa: E731
    xa = torch.relu(x.cpu().double() * b(sc) + b(sh))
    return ref, w0.cpu().double() - 0.5 * ref_wgrad(dy.cpu(), xa, geom)


def _run(geom, split, x, dy, sc, sh, w0):
    dw = torch.full_like(w0, float("nan"))
    F32.conv_wgrad(dy, x, geom, dw, accumulate=False, split_k=split)
    w = w0.clone()
    F32.conv_wgrad(dy, x, geom, w, accumulate=True, gscale=-0.5, in_bn=(sc, sh), split_k=split)
    return dw, w


def _case(cuda, geom, splits, per_slice=None, ramp=False):
    ntile = _tiles(geom)
    ins = _inputs(geom, cuda, ramp)
    ref, ref_acc = _refs(geom, *ins)
    for i, split in enumerate(splits):
        if per_slice is not None:  # the tile counts of the slices this case is about
            per = 2 * -(-(-(-ntile // 2)) // split)
            assert [max(0, min(per, ntile - s * per)) for s in range(split)] == per_slice[i], (ntile, split)
        dw, w = _run(geom, split, *ins)
        _close(dw, ref)
        _close(w, ref_acc)
        dw2, w2 = _run(geom, split, *ins)
        assert torch.equal(dw, dw2) and torch.equal(w, w2), f"split {split}: not repeatable"


# ---- the two-stage ring: 1, 2, 3 and 4 tiles per slice, unequal slices, a slice with no tile
RING = [
    (g3(2, 1, 16, 16, 32, 64), [1, 2, 3], [[4], [2, 2], [2, 2, 0]]),
    (g3(1, 1, 32, 32, 32, 64), [3, 5], [[6, 6, 4], [4, 4, 4, 4, 0]]),
    (g3(2, 1, 8, 8, 32, 64), [1], [[1]]),
    (g3(2, 3, 8, 8, 32, 64), [1, 2], [[3], [2, 1]]),
    (g3(1, 5, 8, 8, 32, 64), [2], [[4, 1]]),
]


@pytest.mark.parametrize("geom,splits,per_slice", RING, ids=["16x16", "32x32", "8x8n1", "8x8n3", "8x8n5"])
def test_ring_parity_and_drain(cuda, geom, splits, per_slice):
    _case(cuda, geom, splits, per_slice)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_width8(cuda, n):
    _case(cuda, g3(1, n, 8, 8, 32, 64), [1, 2] if n == 5 else [1])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9, 11])
def test_width4(cuda, n):
    """4x4 images, four per tile: fewer than a tile holds (1, 3), whole tiles (4, 8), one image into
    the next tile (5, 9), and 11 (2 3/4 tiles), also split into slices of 2 and 1 tiles."""
    _case(cuda, g3(2, n, 4, 4, 32, 64), [1, 2] if n == 11 else [1])


def test_width4_taller_than_wide(cuda):
    _case(cuda, g3(1, 3, 8, 4, 64, 64), [1])  # two images per tile, the last tile half full


def test_width4_window_shift(cuda):
    _case(cuda, g3(1, 5, 4, 4, 32, 64), [1], ramp=True)


@pytest.mark.parametrize("geom", [g1(2, 1, 32, 32, 32, 64), g1(2, 5, 4, 4, 64, 64)], ids=["32x32", "4x4"])
def test_1x1(cuda, geom):
    _case(cuda, geom, [1, 2])


def test_multi_block(cuda):
    _case(cuda, g3(1, 2, 16, 16, 64, 128), [1, 3])  # 2 k blocks x 2 c blocks of workgroups


def test_headline_grid_4x4(cuda):
    _case(cuda, g3(1, 2, 4, 4, 512, 512), [1])  # 8 x 16 workgroups, one half-full tile each


def test_graph_replay_matches_eager(cuda):
    """One captured call, replayed twice, equals the eager call bit for bit: the hand-over between
    the staging and the compute waves keeps no state from one launch to the next."""
    geom = g3(2, 2, 16, 16, 32, 64)
    _tiles(geom)
    x, dy, sc, sh, w0 = _inputs(geom, cuda)
    F32.ensure_workspace(cuda)
    eager = torch.zeros_like(w0)
    F32.conv_wgrad(dy, x, geom, eager, accumulate=False, split_k=3)
    torch.cuda.synchronize()
    out = torch.zeros_like(w0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F32.conv_wgrad(dy, x, geom, out, accumulate=False, split_k=3)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
