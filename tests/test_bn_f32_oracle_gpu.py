"""fp32 BatchNorm on the device (csrc/kernels/bn_f32.hip and the statistics epilogues of the fp32
convs) against the float64 oracle of tests/bn_f32_oracle.py.

A. conv -> per-tile (sum, M2) slots -> ``Fn.bn_finalize`` (Chan's merge, ``slot_fold_chan``) for
   every conv engine, on zero-mean and on shifted-mean data (|mean| / std > 100, where a single-pass
   sum / sum-of-squares epilogue is off by > 2e-3: tests/test_bn_f32_oracle_cpu.py), at slot counts
   on both sides of the fold's 8-slots-in-flight loop (S > 224) up to the benchmark's S = 800. The
   reference is the float64 statistics of the device's own fp32 output.
B. the streaming passes and folds over channel tilings C in {4, 24, 64, 96, 1024, 2048} x row counts
   M in {1, 7, 777} and one M above each tiling's grid cap, G in {1, 3}, under the three variants
   of the backward fold.

Tolerances are the project's: 1e-5 of the result's max-abs, 2e-5 for raw sums, d(gamma), d(beta)
and the coefficients derived from them. Every figure is printed before it is asserted.
"""
import math

import pytest
import torch

import bn_f32_oracle as O
from ddl25spring_amd.ops import _lib
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.ops import functional_f32 as F32
from ddl25spring_amd.ops.functional import ConvGeom

pytestmark = pytest.mark.gpu

EPS = O.EPS
HOST_NUMEL = 1 << 21  # larger tensors keep their float64 reference arithmetic on the device


@pytest.fixture(params=["mfma32", "x6", "auto"])
def fmath(request):
    """Both fp32 product engines — the exact fp32 MFMA and the 3-way-split bf16 MFMA (x6) — and
    the default per-layer mix of the two (auto: the tuned plans pick the engine)."""
    old = F32.math()
    F32.set_math(request.param)
    yield request.param
    F32.set_math(old)


def _err(a, b, scale=None):
    b = b.double()
    a = a.double().to(b.device)
    if scale is None:
        scale = b.abs().max().item()
    return (a - b).abs().max().item() / (scale + 1e-30)


def _close(tag, a, b, rel=1e-5, scale=None):
    e = _err(a, b, scale)
    print(f"BNF32 {tag} err={e:.3g} tol={rel:g}")
    assert e <= rel, f"{tag}: relative max err {e:.3g} > {rel:g}"


def _strided(v, pad=8, fill=7.0):
    """v [G, C] as a group-strided view into a wider buffer (the flat parameter store's layout)
    -> (buffer, view); ``_pad_intact`` checks that nothing wrote beside the view."""
    G, C = v.shape
    flat = torch.full((G, C + 2 * pad), fill, device=v.device)
    flat[:, pad:pad + C] = v
    return flat, flat[:, pad:pad + C]


def _pad_intact(flat, pad=8, fill=7.0):
    return bool((flat[:, :pad] == fill).all()) and bool((flat[:, -pad:] == fill).all())


# ============================================================================ A. conv statistics
def _g(G, N, H, W, C, K, R, stride=1):
    return ConvGeom(G=G, N=N, H=H, W=W, C=C, K=K, R=R, S=R, stride=stride, pad=(R - 1) // 2)


# (geometry, split_k, expected halo (rows, slots) | None, expected minimum slots on any engine)
CONV_CASES = [
    (_g(2, 3, 9, 9, 64, 128, 3, 2), 0, None, 1),      # register-staged engine, M = 75: one ragged tile
    (_g(2, 5, 8, 8, 64, 64, 3), 0, (128, 3), 3),      # halo, power-of-two width, partial last tile
    (_g(1, 3, 14, 14, 32, 48, 3), 0, None, 5),        # ResNet-50 widths the halo kernel declines (14 % 8,
    (_g(1, 5, 7, 7, 32, 32, 3), 0, None, 2),          # 16 % 7): register engine, ragged tails
    (_g(1, 2, 28, 28, 32, 48, 3), 0, (112, 14), 13),  # halo, rows padded 28 -> 32: 4 x 28 real pixels per tile
    (_g(1, 5, 8, 7, 32, 32, 3), 0, (112, 3), 3),      # halo, rows padded 7 -> 8, two images per tile, ragged tail (56)
    (_g(2, 3, 20, 20, 48, 64, 1), 0, None, 10),       # 1x1, width not a power of two
    (_g(1, 3, 4, 4, 512, 512, 3), 3, (128, 1), 1),    # statistics written by the split-K epilogue
    (_g(1, 30, 32, 32, 32, 64, 1), 0, (128, 240), 240),   # S = 240: the unrolled fold loop plus a tail
    (_g(1, 100, 32, 32, 64, 64, 3), 0, (128, 800), 800),  # the benchmark's layer-1 shape
]
CONV_IDS = [f"{g.C}x{g.K}_{g.H}x{g.W}_n{g.N}_{g.R}s{g.stride}" + (f"_k{sk}" if sk else "") for g, sk, _, _ in CONV_CASES]


def _engine_class(geom):
    """Which statistics path a FWD launch of geom takes under the current engine."""
    lg = F32._launch_geom(geom, "f")
    if not F32.uses_halo(F32.F_FWD, lg):
        return "register"
    return "halo_padded" if lg.Q & (lg.Q - 1) else "halo_pow2"


class _LaunchSpy:
    """Records what conv launches actually ran: the library entry point and the split-K count."""

    def __init__(self, monkeypatch):
        self.entries, self.splits = [], []
        lib = _lib.kernels()
        for name in ("ddl_x6h", "ddl_convf32"):
            orig = getattr(lib, name)

            def wrap(*a, _orig=orig, _name=name):
                self.entries.append(_name)
                return _orig(*a)
            monkeypatch.setattr(lib, name, wrap)
        launch = F32._launch

        def spy(a, mode, geom, device, split_k=0, ws_role="main"):
            launch(a, mode, geom, device, split_k, ws_role)
            self.splits.append(int(a.split_k))
        monkeypatch.setattr(F32, "_launch", spy)


def _run_conv(geom, split_k, regime, dev):
    inp = O.conv_inputs(regime, geom)
    inner = geom.K * geom.R * geom.S * geom.C
    wflat = torch.zeros(geom.G, inner + 96, device=dev)  # group-strided weights, like the flat parameter store
    w = wflat[:, 16:16 + inner].unflatten(1, (geom.K, geom.R, geom.S, geom.C))
    w.copy_(inp["w"])
    st = F32.SlotStats()
    cu = lambda t: None if t is None else t.to(dev)  # noqa: E731
    y = Fn.conv_fwd(inp["x"].to(dev), w, geom, bias=cu(inp["bias"]), relu=inp["relu"], stats=st,
                    residual=cu(inp["residual"]), split_k=split_k)
    return y, st


@pytest.mark.parametrize("regime", O.REGIMES)
@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_conv_slots_finalize(cuda, fmath, case, regime, monkeypatch):
    """conv epilogue slots -> bn_finalize (tile_rows > 0: Chan's merge) vs the float64 statistics
    of the device's own output; then that BN's backward on the same (possibly shifted) activations."""
    geom, split_k, halo_slots, min_slots = case
    spy = _LaunchSpy(monkeypatch)
    y, st = _run_conv(geom, split_k, regime, cuda)
    G, K, M = geom.G, geom.K, geom.N * geom.P * geom.Q
    # which engine ran, and the slot layout it left
    lg = F32._launch_geom(geom, "f")
    cls = _engine_class(geom)
    assert spy.entries == ["ddl_x6h" if cls != "register" else "ddl_convf32"], (spy.entries, cls)
    if split_k:
        assert spy.splits == [split_k] and split_k > 1
    rows, S = st.rows, st.t.shape[1]
    assert rows > 0 and rows == F32.slot_rows(F32.F_FWD, lg) and S == -(-M // rows) and S >= min_slots
    if cls != "register":
        assert (rows, S) == halo_slots
        assert (rows == 112) == (cls == "halo_padded")
    else:
        assert rows in (64, 128)
    if regime == "zerovar":
        assert bool((y[..., O.zero_channel(K)] == 40).all())
    torch.manual_seed(11)
    gamma, beta = torch.rand(G, K, device=cuda) + 0.5, torch.randn(G, K, device=cuda) * 0.1
    rm0, rv0 = torch.randn(G, K, device=cuda) * 0.2, torch.rand(G, K, device=cuda) + 0.5
    gflat, gv = _strided(gamma)
    bflat, bv = _strided(beta)
    rmflat, rm = _strided(rm0)
    rvflat, rv = _strided(rv0)
    sc, sh, mu, rs = Fn.bn_finalize(st, gv, bv, rm, rv, M)
    side = lambda *ts: tuple(t if y.numel() > HOST_NUMEL else t.cpu() for t in ts)  # noqa: E731
    ref = O.bn_train(*side(y.reshape(G, M, K), gamma, beta, rm0, rv0))
    ratio = (ref["mean"].abs() / torch.sqrt(ref["var"] + 1e-300)).min().item()
    print(f"BNF32 A/{regime} S={S} rows={rows} engine={cls} min|mean|/std={ratio:.3g}")
    tag = f"A/{regime}/"
    _close(tag + "mean", mu, ref["mean"])
    _close(tag + "rstd", rs, ref["rstd"])
    _close(tag + "scale", sc, ref["scale"])
    _close(tag + "shift", sh, ref["shift"])
    _close(tag + "running_mean", rm, ref["running_mean"])
    _close(tag + "running_var", rv, ref["running_var"])
    assert all(_pad_intact(f) for f in (gflat, bflat, rmflat, rvflat))
    if regime == "zerovar":
        k0 = O.zero_channel(K)
        want = 1.0 / math.sqrt(EPS)
        e = (rs[:, k0].double() - want).abs().max().item() / want
        print(f"BNF32 A/zerovar/rstd0 err={e:.3g} tol=1e-05")
        assert e <= 1e-5
        assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
        _close(tag + "mean0", mu[:, k0], torch.full((G,), 40.0, dtype=torch.float64))
    # the BN backward on these activations, given the forward's own (mean, rstd)
    dy = torch.randn(G, M, K, device=cuda)
    dgflat, dg = _strided(torch.full((G, K), 0.25, device=cuda))
    dbflat, db = _strided(torch.full((G, K), -0.5, device=cuda))
    x = y.reshape(G, M, K)
    dx = Fn.bn_backward(dy, None, x, mu, rs, gv, dg, db)
    bw = O.bn_backward(*side(dy, x, mu, rs, gamma))
    _close(tag + "dx", dx, bw["dx"])
    _close(tag + "dgamma", dg, bw["dgamma"] + 0.25, rel=2e-5)
    _close(tag + "dbeta", db, bw["dbeta"] - 0.5, rel=2e-5)
    assert _pad_intact(dgflat) and _pad_intact(dbflat) and F32.fold_tickets_clean()


def test_conv_cases_cover_every_statistics_path(cuda):
    """Under at least one engine the cases above run a row-padded halo launch, a power-of-two halo
    launch and a register-engine launch (each case asserts that the launch it made is the planned
    one), and the fold sees slot counts on both sides of its unrolled loop (S > 7 * 32)."""
    old = F32.math()
    seen = {}
    try:
        for m in F32.MATHS:
            F32.set_math(m)
            seen[m] = {_engine_class(g) for g, _, _, _ in CONV_CASES}
    finally:
        F32.set_math(old)
    print("BNF32 engines", seen)
    assert any({"halo_padded", "halo_pow2", "register"} <= s for s in seen.values()), seen
    assert "register" in seen["mfma32"] and seen["mfma32"] == {"register"}
    slots = sorted(c[3] for c in CONV_CASES)
    assert slots[0] <= 7 * 32 < slots[-2] and slots[-1] == 800


def test_finalize2_different_channels_and_slots(cuda, fmath):
    """One launch finalizing two BatchNorms of different C (64 | 128: the grid covers the larger) and
    different slot counts == the two single launches bit for bit, in either order, and the oracle."""
    cases = [CONV_CASES[1], CONV_CASES[0]]  # K = 64, M = 320, 3 slots | K = 128, M = 75, 1 slot
    torch.manual_seed(12)
    bns, refs = [], []
    for (geom, split_k, _, _), regime in zip(cases, ("bias", "randn")):
        y, st = _run_conv(geom, split_k, regime, cuda)
        G, K, M = geom.G, geom.K, geom.N * geom.P * geom.Q
        gamma, beta = torch.rand(G, K, device=cuda) + 0.5, torch.randn(G, K, device=cuda) * 0.1
        rm0, rv0 = torch.randn(G, K, device=cuda) * 0.2, torch.rand(G, K, device=cuda) + 0.5
        bns.append((st, gamma, beta, rm0, rv0, M))
        refs.append(O.bn_train(y.cpu().reshape(G, M, K), gamma.cpu(), beta.cpu(), rm0.cpu(), rv0.cpu()))
    assert bns[0][0].t.shape[-1] == 64 and bns[1][0].t.shape[-1] == 128
    assert bns[0][0].t.shape[1] != bns[1][0].t.shape[1]

    def fresh(bn):
        st, gamma, beta, rm0, rv0, M = bn
        return (st, gamma, beta, rm0.clone(), rv0.clone(), M)
    single = []
    for bn in bns:
        a = fresh(bn)
        single.append((*Fn.bn_finalize(*a), a[3], a[4]))
    for order in ((0, 1), (1, 0)):
        a, b = fresh(bns[order[0]]), fresh(bns[order[1]])
        outs = Fn.bn_finalize2(a, b)
        for i, args, out in zip(order, (a, b), outs):
            got = (*out, args[3], args[4])
            for name, t, s in zip(("scale", "shift", "mean", "rstd", "running_mean", "running_var"), got, single[i]):
                assert torch.equal(t, s), (order, i, name)
                _close(f"A2/{name}", t, refs[i][name])


# ============================================================================ B. streaming passes
def _tpr(C):
    return min(C // 4, 256)


def _rpi(C):
    return 256 // _tpr(C)


CS = (4, 24, 64, 96, 1024, 2048)
SHAPES = [(G, M, C) for C in CS for M in (1, 7, 777) for G in (1, 3)]
# one M per C above the streaming grid cap (2048 blocks x RPI rows x 4) — hence above the reduce
# passes' 256 slots x RPI x 16 rows too — and the benchmark's M = 102400 at C = 64 (reduce slots
# capped at 256, streaming grid not). Largest tensor: 8200 x 2048 fp32 = 67 MB.
BIG = [(1, 2048 * _rpi(C) * 4 + (8 if C >= 1024 else 7), C) for C in CS] + [(1, 102400, 64)]
ALL_SHAPES = SHAPES + BIG
SHAPE_IDS = [f"g{G}_m{M}_c{C}" for G, M, C in ALL_SHAPES]


def _slots_formula(M, C, G):
    return max(1, min(-(-M // (_rpi(C) * 16)), min(256, -(-2048 // G))))


def test_shapes_cross_the_grid_caps():
    assert (1, 8200, 1024) in BIG and (1, 8200, 2048) in BIG
    for G, M, C in BIG:
        assert _slots_formula(M, C, G) == 256 and M * C * 4 < 70e6
        assert (M > 2048 * _rpi(C) * 4) == ((G, M, C) != (1, 102400, 64))


def _activations(G, M, C, dev, seed=0):
    """c with mean 0.5, std 2 per channel. M == 1 draws multiples of 1/64 (|c| < 32), whose squares
    are exact in fp32: one row per channel is the limit |mean| / std = inf of the sum / sum-of-squares
    statistics, which keep the variance only as exactly as they keep c^2 (F32.bn_stats); with exact
    squares the count == 1 branch gives variance 0, as defined."""
    torch.manual_seed(100 + seed)
    c = torch.randn(G, M, C, device=dev) * 2 + 0.5
    if M == 1:
        c = (c * 64).round().clamp(-2047, 2047) / 64
    return c


def _params(G, C, dev):
    gamma, beta = torch.rand(G, C, device=dev) + 0.5, torch.randn(G, C, device=dev) * 0.1
    rm0, rv0 = torch.randn(G, C, device=dev) * 0.2, torch.rand(G, C, device=dev) + 0.5
    return gamma, beta, rm0, rv0


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_stats_finalize_train_and_eval(cuda, shape):
    """Fn.bn_stats (sum / sum-of-squares slots, tile_rows == 0) -> bn_finalize, training and eval."""
    G, M, C = shape
    c = _activations(G, M, C, cuda)
    gamma, beta, rm0, rv0 = _params(G, C, cuda)
    st = Fn.bn_stats(c)
    assert st.rows == 0 and st.t.shape == (G, _slots_formula(M, C, G), 2, C)
    assert st.t.shape[1] == F32.reduce_slots(M, C, G)
    cr, ga, be, rm_r, rv_r = (t if c.numel() > HOST_NUMEL else t.cpu() for t in (c, gamma, beta, rm0, rv0))
    ref = O.bn_train(cr, ga, be, rm_r, rv_r)
    raw = st.t.double().sum(1)
    _close("B/stats/sum", raw[:, 0], O.f64(cr).sum(1), rel=2e-5)
    _close("B/stats/sumsq", raw[:, 1], (O.f64(cr) ** 2).sum(1), rel=2e-5)
    flats = [_strided(t) for t in (gamma, beta, rm0, rv0)]
    (_, gv), (_, bv), (_, rm), (_, rv) = flats
    sc, sh, mu, rs = Fn.bn_finalize(st, gv, bv, rm, rv, M)
    for name, t in (("mean", mu), ("rstd", rs), ("scale", sc), ("shift", sh), ("running_mean", rm), ("running_var", rv)):
        _close(f"B/train/{name}", t, ref[name])
    assert all(_pad_intact(f) for f, _ in flats)
    # eval: the running statistics normalise and stay as they are (with or without a slot buffer)
    ev = O.bn_eval(ga, be, rm_r, rv_r)
    for stats in (F32.SlotStats(), st):
        rme, rve = rm0.clone(), rv0.clone()
        out = Fn.bn_finalize(stats, gv, bv, rme, rve, M, training=False)
        for name, t in zip(("scale", "shift", "mean", "rstd"), out):
            _close(f"B/eval/{name}", t, ev[name])
        assert torch.equal(rme, rm0) and torch.equal(rve, rv0)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_apply_acts_and_residuals(cuda, shape):
    G, M, C = shape
    c = _activations(G, M, C, cuda)
    r = torch.randn(G, M, C, device=cuda)
    sc, sh = torch.randn(G, C, device=cuda), torch.randn(G, C, device=cuda)
    rsc, rsh = torch.rand(G, C, device=cuda) + 0.5, torch.randn(G, C, device=cuda) * 0.3
    side = lambda *ts: tuple(t if c.numel() > HOST_NUMEL else t.cpu() for t in ts)  # noqa: E731
    cr, rr, scr, shr, rscr, rshr = side(c, r, sc, sh, rsc, rsh)
    for kind in (0, 1, 2, 3):
        _close(f"B/apply/act{kind}", Fn.bn_apply(c, sc, sh, act=kind), O.bn_apply(cr, scr, shr, kind=kind))
    for kind in (1, 3):
        _close(f"B/apply/r/act{kind}", Fn.bn_apply(c, sc, sh, r=r, act=kind), O.bn_apply(cr, scr, shr, r=rr, kind=kind))
    for kind in (0, 1, 2):
        out = torch.full_like(c, float("nan"))
        got = Fn.bn_apply(c, sc, sh, r=r, rscale=rsc, rshift=rsh, act=kind, out=out)
        assert got is out
        _close(f"B/apply/rs/act{kind}", out, O.bn_apply(cr, scr, shr, rr, rscr, rshr, kind))


FOLDS = (("one_level", False, True), ("two_level_two_launches", True, False), ("two_level_one_launch", True, True))


def _chunk_part(dy, x, mean, rstd, S):
    """A BN backward's partial sums as a producer with S slots would leave them: slot j holds
    (sum dy, sum dy xhat) of the j-th of S consecutive row chunks (float64 sums, stored in fp32)."""
    G, M, C = x.shape
    d = dy.double()
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    ids = (torch.arange(M, device=x.device) * S) // M
    p0 = torch.zeros(G, S, C, dtype=torch.float64, device=x.device).index_add_(1, ids, d)
    p1 = torch.zeros(G, S, C, dtype=torch.float64, device=x.device).index_add_(1, ids, d * xh)
    return torch.stack([p0, p1], 2).float().contiguous()


def _moments(c):
    mean = c.mean(1)
    var = c.var(1, unbiased=False) if c.shape[1] > 1 else torch.zeros_like(mean)
    return mean, 1 / torch.sqrt(var + EPS)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_backward_under_every_fold(cuda, shape, monkeypatch):
    """bn_backward (masked | plain | emit_dym | accumulating into strided pre-filled views),
    bn_backward_coef + coef_apply, and bn_backward2 with parts of different slot counts, each under
    the three fold variants, against one float64 reference. M == 1: dx is identically 0 (dy_m - s0 with
    s0 = dy_m), so its error is taken relative to max |A dy_m|, the terms that cancel."""
    G, M, C = shape
    c = _activations(G, M, C, cuda)
    c2 = _activations(G, M, C, cuda, seed=1)
    gamma, _, _, _ = _params(G, C, cuda)
    gamma2 = torch.rand(G, C, device=cuda) + 0.5
    dy = torch.randn(G, M, C, device=cuda)
    ymask = torch.relu(torch.randn(G, M, C, device=cuda))  # a ReLU output: exact zeros where masked
    mean, rstd = _moments(c)
    mean2, rstd2 = _moments(c2)
    side = lambda *ts: tuple(t if c.numel() > HOST_NUMEL else t.cpu() for t in ts)  # noqa: E731
    cr, c2r, dyr, ymr, mr, rr, m2r, r2r, gr, g2r = side(c, c2, dy, ymask, mean, rstd, mean2, rstd2, gamma, gamma2)
    bm = O.bn_backward(dyr, cr, mr, rr, gr, ymask=ymr)
    bp = O.bn_backward(dyr, cr, mr, rr, gr)
    bp2 = O.bn_backward(dyr, c2r, m2r, r2r, g2r)
    dym_dev = torch.where(ymask > 0, dy, torch.zeros_like(dy))

    def dx_scale(b):
        return (b["A"][:, None] * O.f64(b["dym"])).abs().max().item() if M == 1 else None
    Sa = F32.reduce_slots(M, C, G)
    # 130 slots against the reduce pass's 4 at M = 777, C = 64; the benchmark's 800 conv tiles against
    # its 256 on the large shapes (13 level-1 blocks: the level-2 loop's 8 in flight plus a tail)
    Sb = Sa + 126 if M < 8192 else 800
    part_b = _chunk_part(dy, c2, mean2, rstd2, Sb)
    gflat, gv = _strided(gamma)
    g2flat, g2v = _strided(gamma2)
    for name, fold2, fold1l in FOLDS:
        monkeypatch.setattr(F32, "FOLD2", [fold2])
        monkeypatch.setattr(F32, "FOLD1L", [fold1l])
        tag = f"B/bwd/{name}/"
        # masked, accumulating into pre-filled group-strided views
        dgflat, dg = _strided(torch.full((G, C), 0.25, device=cuda))
        dbflat, db = _strided(torch.full((G, C), -0.5, device=cuda))
        dx = Fn.bn_backward(dy, ymask, c, mean, rstd, gv, dg, db)
        _close(tag + "masked/dx", dx, bm["dx"], scale=dx_scale(bm))
        _close(tag + "masked/dgamma", dg, bm["dgamma"] + 0.25, rel=2e-5)
        _close(tag + "masked/dbeta", db, bm["dbeta"] - 0.5, rel=2e-5)
        assert _pad_intact(dgflat) and _pad_intact(dbflat) and _pad_intact(gflat)
        # emit_dym: the masked gradient itself, and the same dx
        dx2, dym = Fn.bn_backward(dy, ymask, c, mean, rstd, gv, emit_dym=True)
        assert torch.equal(dym, dym_dev) and torch.equal(dx2, dx)
        # plain, and its coefficient form: coef_apply(bn_backward_coef) == bn_backward, bit for bit
        dg1, db1 = torch.zeros(G, C, device=cuda), torch.zeros(G, C, device=cuda)
        dxp = Fn.bn_backward(dy, None, c, mean, rstd, gamma, dg1, db1)
        _close(tag + "plain/dx", dxp, bp["dx"], scale=dx_scale(bp))
        _close(tag + "plain/dgamma", dg1, bp["dgamma"], rel=2e-5)
        _close(tag + "plain/dbeta", db1, bp["dbeta"], rel=2e-5)
        dg2, db2 = torch.zeros(G, C, device=cuda), torch.zeros(G, C, device=cuda)
        coef = F32.bn_backward_coef(dy, c, mean, rstd, gamma, dg2, db2)
        assert torch.equal(dg2, dg1) and torch.equal(db2, db1)
        for i, k in enumerate("ABC"):
            _close(tag + f"coef/{k}", coef[:, i], bp[k], rel=2e-5)
        assert torch.equal(F32.coef_apply(dy, c, coef), dxp)
        # two BNs sharing dy: a's part from the reduce pass (Sa slots), b's from a producer with more
        part_a = Fn.bn_bwd_reduce_part(dy, None, c, mean, rstd)
        assert part_a.shape[1] == Sa < part_b.shape[1]
        raw = part_a.double().sum(1)
        _close(tag + "part/s0", raw[:, 0], bp["s0"], rel=2e-5)
        _close(tag + "part/s1", raw[:, 1], bp["s1"], rel=2e-5)
        outs = {}
        for order in ("ab", "ba"):
            za = [torch.zeros(G, C, device=cuda) for _ in range(4)]
            bn_a = (c, mean, rstd, gamma, za[0], za[1], part_a)
            bn_b = (c2, mean2, rstd2, g2v, *(v for _, v in (_strided(za[2]), _strided(za[3]))), part_b)
            if order == "ab":
                dxa, dxb = Fn.bn_backward2(dy, bn_a, bn_b)
            else:
                dxb, dxa = Fn.bn_backward2(dy, bn_b, bn_a)
            outs[order] = (dxa, dxb, za[0], za[1], bn_b[4], bn_b[5])
            _close(tag + f"two/{order}/dx_a", dxa, bp["dx"], scale=dx_scale(bp))
            _close(tag + f"two/{order}/dx_b", dxb, bp2["dx"], scale=dx_scale(bp2))
            _close(tag + f"two/{order}/dgamma_a", za[0], bp["dgamma"], rel=2e-5)
            _close(tag + f"two/{order}/dbeta_a", za[1], bp["dbeta"], rel=2e-5)
            _close(tag + f"two/{order}/dgamma_b", bn_b[4], bp2["dgamma"], rel=2e-5)
            _close(tag + f"two/{order}/dbeta_b", bn_b[5], bp2["dbeta"], rel=2e-5)
        assert torch.equal(outs["ab"][0], dxp)  # a's part is the reduce pass's own: the single backward's dx
        for u, v in zip(outs["ab"], outs["ba"]):
            assert torch.equal(u, v)
        assert _pad_intact(g2flat)
        assert F32.fold_tickets_clean()


def _pool_shape(M):
    """M rows as N samples x HW pixels, HW the largest divisor of M up to 64."""
    hw = max(d for d in range(1, 65) if M % d == 0)
    return M // hw, hw


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_avgpool_bwd_bn_and_channel_sum(cuda, shape):
    G, M, C = shape
    N, HW = _pool_shape(M)
    c = _activations(G, M, C, cuda).reshape(G, N, HW, 1, C)
    x = torch.relu(c * 0.7 + torch.randn_like(c))
    dy = torch.randn(G, N, C, device=cuda)
    mean, rstd = torch.randn(G, C, device=cuda) * 0.1 + 0.5, torch.rand(G, C, device=cuda) + 0.5
    dx, part = Fn.avgpool_bwd_bn(dy, x, (c, mean, rstd))
    assert part.shape == (G, F32.reduce_slots(M, C, G), 2, C)
    side = lambda *ts: tuple(t if c.numel() > HOST_NUMEL else t.cpu() for t in ts)  # noqa: E731
    ref = O.avgpool_bwd_bn(*side(dy, x, c, mean, rstd))
    _close("B/pool/dx", dx, ref["dx"])
    raw = part.double().sum(1)
    _close("B/pool/s0", raw[:, 0], ref["s0"], rel=2e-5)
    _close("B/pool/s1", raw[:, 1], ref["s1"], rel=2e-5)
    # the per-channel sum (bias gradients), accumulated into a pre-filled group-strided view
    flat, out = _strided(torch.full((G, C), 0.75, device=cuda))
    assert Fn.channel_sum(c, out) is out
    cr, = side(c)
    _close("B/channel_sum", out, O.f64(cr).reshape(G, M, C).sum(1) + 0.75, rel=2e-5)
    assert _pad_intact(flat)


@pytest.mark.parametrize("C", [6, 1028])
def test_unsupported_channel_counts_raise_before_any_launch(cuda, C):
    """C % 4 != 0, or C / 4 neither <= 256 nor a multiple of 256: every streaming entry point refuses
    on the host. Outputs the caller provides stay as they were."""
    G, M = 2, 5
    assert F32.reduce_slots(M, C, G) == -1
    c, dy = torch.randn(G, M, C, device=cuda), torch.randn(G, M, C, device=cuda)
    v = torch.rand(G, C, device=cuda) + 0.5
    part = torch.randn(G, 1, 2, C, device=cuda)
    out = torch.full_like(c, 3.0)
    acc = torch.full((G, C), 3.0, device=cuda)
    dg, db = torch.full((G, C), 3.0, device=cuda), torch.full((G, C), 3.0, device=cuda)
    with pytest.raises(RuntimeError):
        Fn.bn_stats(c)
    with pytest.raises(RuntimeError):
        Fn.bn_apply(c, v, v, out=out)
    with pytest.raises(RuntimeError):
        Fn.bn_bwd_reduce_part(dy, None, c, v, v)
    with pytest.raises(RuntimeError):
        Fn.bn_backward(dy, None, c, v, v, v, dg, db)
    with pytest.raises(RuntimeError):
        Fn.bn_backward(dy, None, c, v, v, v, dg, db, part=part)
    with pytest.raises(RuntimeError):
        F32.bn_backward_coef(dy, c, v, v, v, dg, db, part=part)
    with pytest.raises(RuntimeError):
        Fn.bn_backward2(dy, (c, v, v, v, dg, db, part), (c, v, v, v, dg, db, part))
    with pytest.raises(RuntimeError):
        Fn.avgpool_bwd_bn(torch.randn(G, M, C, device=cuda), c.reshape(G, M, 1, 1, C), (c.reshape(G, M, 1, 1, C), v, v))
    with pytest.raises(RuntimeError):
        Fn.channel_sum(c, acc)
    torch.cuda.synchronize()
    for t in (out, acc, dg, db):
        assert bool((t == 3.0).all())
    assert F32.fold_tickets_clean()
    coef = torch.randn(G, 3, C, device=cuda)
    if C % 4:
        with pytest.raises(RuntimeError):
            F32.coef_apply(dy, c, coef, out=out)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    else:  # coef_apply walks float4 chunks of any C % 4 == 0
        b = lambda i: coef[:, i].double().cpu()[:, None]  # noqa: E731
        _close("B/coef_apply/1028", F32.coef_apply(dy, c, coef), b(0) * dy.double().cpu() + b(1) * c.double().cpu() + b(2))


def test_bn_stats_single_pass_error_at_shifted_mean(cuda):
    """F32.bn_stats keeps (sum, sum of squares) in fp32 slots, so at |mean| / std = 100 its variance
    carries the rounding of sums 1e4 times larger than itself (by design: the conv epilogues'
    two-pass slots are the accurate path). Measured and bounded, not held to 1e-5: each slot value
    is at most 16 + RPI sequential fp32 additions per lane plus the rounding of x^2, so
    |d var| <= (17 + RPI) 2^-24 (mean^2 + var), and rstd moves by half of that relatively."""
    G, M, C = 2, 4096, 64
    torch.manual_seed(13)
    sign = torch.where(torch.rand(G, 1, C, device=cuda) < 0.5, -1.0, 1.0)
    c = 100.0 * sign + torch.randn(G, M, C, device=cuda)
    ref = O.bn_train(c.cpu())
    ones, zeros = torch.ones(G, C, device=cuda), torch.zeros(G, C, device=cuda)
    _, _, mu, rs = Fn.bn_finalize(Fn.bn_stats(c), ones, zeros, zeros.clone(), ones.clone(), M)
    e = _err(rs, ref["rstd"])
    bound = 0.5 * (17 + _rpi(C)) * 2.0 ** -24 * (1 + 100.0 ** 2) * 1.1
    print(f"BNF32 stats/single_pass/rstd err={e:.3g} bound={bound:.3g}")
    _close("stats/single_pass/mean", mu, ref["mean"])
    assert e <= bound
