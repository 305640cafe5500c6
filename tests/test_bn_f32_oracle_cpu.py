"""The float64 BatchNorm oracle (tests/bn_f32_oracle.py) against torch's own float64 batch_norm and
autograd, and the proof that the shifted-mean inputs of the GPU test discriminate: on them a
single-pass fp32 sum / sum-of-squares estimate misses the float64 rstd by more than ten times the
tolerance the GPU test allows the kernels (tests/test_bn_f32_oracle_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import bn_f32_oracle as O
from ddl25spring_amd.ops.functional import ConvGeom

GPU_TOL = 1e-5  # the project's max-abs-relative bound of test_bn_f32_oracle_gpu.py


def _err(a, b):
    a, b = a.double(), b.double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.mark.parametrize("G,M,C", [(1, 1, 4), (2, 7, 24), (3, 300, 64)])
@pytest.mark.parametrize("masked", [False, True])
def test_oracle_matches_torch_float64(G, M, C, masked):
    torch.manual_seed(0)
    x = (torch.randn(G, M, C, dtype=torch.float64) * 2 + 0.5)
    gamma = torch.rand(G, C, dtype=torch.float64) + 0.5
    beta = torch.randn(G, C, dtype=torch.float64) * 0.1
    rm0, rv0 = torch.randn(G, C, dtype=torch.float64), torch.rand(G, C, dtype=torch.float64) + 0.5
    dy = torch.randn(G, M, C, dtype=torch.float64)
    r = torch.randn(G, M, C, dtype=torch.float64)
    fwd = O.bn_train(x, gamma, beta, rm0, rv0)
    y = O.bn_apply(x, fwd["scale"], fwd["shift"], r=r, kind=1 if masked else 0)
    bwd = O.bn_backward(dy, x, fwd["mean"], fwd["rstd"], gamma, ymask=y if masked else None)
    for g in range(G):
        xg = x[g].clone().requires_grad_(True)
        gg, bg = gamma[g].clone().requires_grad_(True), beta[g].clone().requires_grad_(True)
        rm, rv = rm0[g].clone(), rv0[g].clone()
        if M > 1:
            # [M, C] is batch_norm's (N, C) layout: statistics over the rows
            yt = F.batch_norm(xg, rm, rv, gg, bg, True, O.MOMENTUM, O.EPS)
            assert _err(fwd["running_mean"][g], rm) <= 1e-12
            assert _err(fwd["running_var"][g], rv) <= 1e-12
        else:  # torch refuses one value per channel in training mode: the definition itself
            yt = (xg - xg.mean(0)) / torch.sqrt(xg.var(0, unbiased=False) + O.EPS) * gg + bg
            assert _err(fwd["running_mean"][g], 0.9 * rm0[g] + 0.1 * x[g, 0]) <= 1e-12
            assert _err(fwd["running_var"][g], 0.9 * rv0[g]) <= 1e-12  # count == 1: biased variance (0)
        yt = yt + r[g]
        if masked:
            yt = yt.clamp_min(0)
        assert _err(y[g], yt.detach()) <= 1e-12
        yt.backward(dy[g])
        scale = xg.grad.abs().max().item() + (fwd["scale"][g] * dy[g]).abs().max().item()
        assert (bwd["dx"][g] - xg.grad).abs().max().item() <= 1e-12 * scale
        assert _err(bwd["dgamma"][g], gg.grad) <= 1e-12
        assert _err(bwd["dbeta"][g], bg.grad) <= 1e-12
    ev = O.bn_eval(gamma, beta, rm0, rv0)
    for g in range(G):
        ye = F.batch_norm(x[g], rm0[g].clone(), rv0[g].clone(), gamma[g], beta[g], False, O.MOMENTUM, O.EPS)
        assert _err(O.bn_apply(x, ev["scale"], ev["shift"])[g], ye) <= 1e-12


def test_oracle_apply_variants_and_pool_backward():
    torch.manual_seed(1)
    G, N, H, W, C = 2, 3, 2, 5, 8
    x = torch.randn(G, N, H, W, C, dtype=torch.float64)
    r = torch.randn_like(x)
    sc, sh, rsc, rsh = (torch.randn(G, C, dtype=torch.float64) for _ in range(4))
    b = lambda t: t[:, None, None, None]  # noqa: E731
    for kind, slope in ((2, 0.01), (3, 0.2)):
        want = F.leaky_relu(x * b(sc) + b(sh) + r * b(rsc) + b(rsh), slope)
        assert _err(O.bn_apply(x, sc, sh, r, rsc, rsh, kind), want) <= 1e-12
    # pool backward: autograd of mean over (H, W) of relu(x), masked the same way
    c = torch.randn_like(x)
    xr = x.clone().requires_grad_(True)
    dy = torch.randn(G, N, C, dtype=torch.float64)
    xr.clamp_min(0).mean((2, 3)).backward(dy)
    mean, rstd = torch.randn(G, C, dtype=torch.float64), torch.rand(G, C, dtype=torch.float64) + 0.5
    got = O.avgpool_bwd_bn(dy, x, c, mean, rstd)
    assert _err(got["dx"], xr.grad) <= 1e-12
    xh = (c - b(mean)) * b(rstd)
    assert _err(got["s0"], xr.grad.sum((1, 2, 3))) <= 1e-12
    assert _err(got["s1"], (xr.grad * xh).sum((1, 2, 3))) <= 1e-12


# the conv geometries of the GPU test small enough for a float64 host convolution; which regimes
# must discriminate on them: "bias" everywhere, "data" on the unpadded 1x1 convs (a zero-padded 3x3
# conv's border pixels spread y by themselves, see bn_f32_oracle.conv_inputs)
SHIFT_CASES = [
    (ConvGeom(G=2, N=3, H=9, W=9, C=64, K=128, R=3, S=3, stride=2, pad=1), ("bias",)),
    (ConvGeom(G=2, N=5, H=8, W=8, C=64, K=64, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=1, N=3, H=14, W=14, C=32, K=48, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=1, N=5, H=7, W=7, C=32, K=32, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=1, N=2, H=28, W=28, C=32, K=48, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=1, N=5, H=8, W=7, C=32, K=32, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=2, N=3, H=20, W=20, C=48, K=64, R=1, S=1, stride=1, pad=0), ("bias", "data")),
    (ConvGeom(G=1, N=3, H=4, W=4, C=512, K=512, R=3, S=3, stride=1, pad=1), ("bias",)),
    (ConvGeom(G=1, N=30, H=32, W=32, C=32, K=64, R=1, S=1, stride=1, pad=0), ("bias", "data")),
]


@pytest.mark.parametrize("geom,regimes", SHIFT_CASES, ids=[f"{g.C}x{g.K}_{g.H}x{g.W}_{g.R}s{g.stride}"
                                                            for g, _ in SHIFT_CASES])
def test_shifted_inputs_expose_a_single_pass_epilogue(geom, regimes):
    assert set(O.SHIFTED) >= set(regimes)
    for regime in regimes:
        y = O.conv_epilogue(O.conv_inputs(regime, geom), geom, geom.stride, geom.pad).float()  # the fp32 output
        ref = O.bn_train(y)
        ratio = (ref["mean"].abs() / torch.sqrt(ref["var"])).min().item()
        _, var = O.naive_single_pass_fp32(y)
        e = _err(1.0 / torch.sqrt(var + O.EPS), ref["rstd"])
        print(f"{regime}: min |mean|/std = {ratio:.1f}, naive fp32 rstd error = {e:.3g}")
        assert ratio >= 100, (regime, ratio)
        assert e > 10 * GPU_TOL, (regime, e)


def test_every_shifted_generator_is_proven():
    assert {r for _, rs in SHIFT_CASES for r in rs} == set(O.SHIFTED)
