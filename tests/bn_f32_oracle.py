"""Float64 oracle of the fp32 BatchNorm passes (csrc/kernels/bn_f32.hip) and of the statistics the
fp32 conv epilogues hand them.

Plain torch, written from the definitions of nn.BatchNorm2d (training semantics:
momentum 0.1, eps 1e-5, biased variance for the normalisation, unbiased for the running variance):
it shares no code with the kernels or with ``ddl25spring_amd.ops.reference``. Activations are
[G, M, C] (G independent BatchNorms, M rows, C channels; any [G, ..., C] is flattened). Every
function takes tensors of any dtype and returns float64 tensors on the device of its inputs: the
tests hand it host copies, or, for the few shapes of tens of millions of elements, device tensors
(float64 torch arithmetic either way; nothing of the library under test runs in here).

* training: mean = sum x / M, var = sum (x - mean)^2 / M, rstd = 1 / sqrt(var + eps),
  scale = gamma rstd, shift = beta - mean scale, running_mean' = (1 - m) running_mean + m mean,
  running_var' = (1 - m) running_var + m var M / (M - 1)  (M == 1: the biased variance, as the kernel);
* eval: mean / var are the running statistics, which stay as they are;
* apply: act(x scale + shift [+ r rscale + rshift | + r]), act 0 none, 1 ReLU, 2 / 3 leaky ReLU
  with slopes 0.01 / 0.2;
* backward, given (x, mean, rstd) of the forward: dy_m = dy [ymask > 0], s0 = sum dy_m,
  s1 = sum dy_m xhat, dbeta = s0, dgamma = s1, A = gamma rstd, B = -A rstd s1 / M,
  C = -A s0 / M - B mean, dx = A dy_m + B x + C  (= gamma rstd (dy_m - s0 / M - xhat s1 / M));
* global-average-pool backward of x = relu(bn(c) ...): dx = dy / HW [x > 0] with s0, s1 of that dx
  against c's BatchNorm.

``naive_single_pass_fp32`` is NOT part of the oracle: it is the estimate a sum / sum-of-squares
epilogue accumulating in fp32 would give, used to prove that the shifted-mean inputs of the GPU
test would expose such an epilogue (tests/test_bn_f32_oracle_cpu.py).
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
SLOPES = {2: 0.01, 3: 0.2}


def f64(t):
    return None if t is None else t.detach().double()


def _gmc(t):
    t = f64(t)
    return t.reshape(t.shape[0], -1, t.shape[-1])


def _row(v):
    return f64(v)[:, None, :]


def bn_train(x, gamma=None, beta=None, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM):
    """-> dict(mean, var, rstd, scale, shift[, running_mean, running_var]) of [G, C] each."""
    x = _gmc(x)
    G, M, C = x.shape
    mean = x.sum(1) / M
    var = ((x - mean[:, None]) ** 2).sum(1) / M
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = f64(gamma) if gamma is not None else torch.ones_like(mean)
    be = f64(beta) if beta is not None else torch.zeros_like(mean)
    out = dict(mean=mean, var=var, rstd=rstd, scale=ga * rstd, shift=be - mean * ga * rstd)
    if running_mean is not None:
        unbiased = var * M / (M - 1) if M > 1 else var
        out["running_mean"] = (1 - momentum) * f64(running_mean) + momentum * mean
        out["running_var"] = (1 - momentum) * f64(running_var) + momentum * unbiased
    return out


def bn_eval(gamma, beta, running_mean, running_var, eps=EPS):
    """Eval mode: the running statistics normalise (and are left alone)."""
    mean, var = f64(running_mean), f64(running_var)
    rstd = 1.0 / torch.sqrt(var + eps)
    ga = f64(gamma) if gamma is not None else torch.ones_like(mean)
    be = f64(beta) if beta is not None else torch.zeros_like(mean)
    return dict(mean=mean, var=var, rstd=rstd, scale=ga * rstd, shift=be - mean * ga * rstd,
                running_mean=mean, running_var=var)


def act(v, kind):
    if kind == 0:
        return v
    if kind == 1:
        return v.clamp_min(0)
    return torch.where(v > 0, v, SLOPES[kind] * v)


def bn_apply(x, scale, shift, r=None, rscale=None, rshift=None, kind=0):
    shape = x.shape
    v = _gmc(x) * _row(scale) + _row(shift)
    if r is not None:
        t = _gmc(r)
        if rscale is not None:
            t = t * _row(rscale) + _row(rshift)
        v = v + t
    return act(v, kind).reshape(shape)


def bn_backward(dy, x, mean, rstd, gamma=None, ymask=None):
    """-> dict(dym, s0, s1, dbeta, dgamma, A, B, C, dx); dym / dx shaped like x."""
    shape = x.shape
    x, dym = _gmc(x), _gmc(dy)
    G, M, C = x.shape
    if ymask is not None:
        dym = dym * (_gmc(ymask) > 0)
    mean, rstd = f64(mean), f64(rstd)
    ga = f64(gamma) if gamma is not None else torch.ones_like(mean)
    xhat = (x - mean[:, None]) * rstd[:, None]
    s0, s1 = dym.sum(1), (dym * xhat).sum(1)
    A = ga * rstd
    B = -A * rstd * s1 / M
    Cc = -A * s0 / M - B * mean
    dx = A[:, None] * dym + B[:, None] * x + Cc[:, None]
    return dict(dym=dym.reshape(shape), s0=s0, s1=s1, dbeta=s0, dgamma=s1, A=A, B=B, C=Cc, dx=dx.reshape(shape))


def avgpool_bwd_bn(dy, x, c, mean, rstd):
    """dy [G, N, C], x = the pooled activation [G, N, H, W, C], c = the input of its BatchNorm
    -> dict(dx [G, N, H, W, C], s0, s1)."""
    G, N, H, W, C = x.shape
    dx = f64(dy).reshape(G, N, 1, 1, C) / (H * W) * (f64(x) > 0)
    xhat = (_gmc(c) - _row(mean)) * _row(rstd)
    d = dx.reshape(G, -1, C)
    return dict(dx=dx, s0=d.sum(1), s1=(d * xhat).sum(1))


def naive_single_pass_fp32(y):
    """(mean, var) [G, C] as a single-pass fp32 epilogue would produce them: sum and sum of squares
    accumulated in fp32, var = sumsq / M - mean^2 in fp32. Returned as float64."""
    y = y.detach().float()
    y = y.reshape(y.shape[0], -1, y.shape[-1])
    M = y.shape[1]
    mean = y.sum(1) / M
    var = ((y * y).sum(1) / M - mean * mean).clamp_min(0)
    return mean.double(), var.double()


# ----------------------------------------------------------------------------- conv statistics inputs
# The data regimes of the conv -> statistics -> finalize test (tests/test_bn_f32_oracle_gpu.py A),
# generated on the host so that the CPU test can prove they discriminate:
#   randn    zero-mean data (what every other test uses);
#   bias     |mean| / std ~ 140 induced by the epilogue: bias_k = +-100, a residual of std 0.5 and
#            a conv output of std ~0.5 (weights scaled by 0.5 / sqrt(R S C));
#   data     mean induced by the data: x = 3 + 0.03 randn, w = 0.1 |randn|. A 1x1 conv (no padding)
#            gives |mean| / std of several hundred; a zero-padded 3x3 conv's border pixels see
#            fewer taps, so there the spread of y is set by the border (|mean| / std ~ 5);
#   fused    bias + residual + ReLU: the statistics are those of the final output;
#   zerovar  one output channel with all-zero weights and bias 40 (variance exactly 0).
REGIMES = ("randn", "bias", "data", "fused", "zerovar")
SHIFTED = ("bias", "data")


def zero_channel(K):
    return K // 2 + 1


def conv_inputs(regime, g, seed=0):
    """-> dict(x [G,N,H,W,C], w [G,K,R,S,C], bias [G,K] | None, residual [G,N,P,Q,K] | None, relu)
    of fp32 host tensors for a conv geometry g (fields G N H W C K R S P Q)."""
    gen = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + seed)

    def rn(*shape):
        return torch.randn(*shape, generator=gen)
    x = rn(g.G, g.N, g.H, g.W, g.C)
    w = rn(g.G, g.K, g.R, g.S, g.C) * 0.1
    bias = residual = None
    relu = False
    if regime == "bias":
        w = rn(g.G, g.K, g.R, g.S, g.C) * (0.5 / math.sqrt(g.R * g.S * g.C))
        sign = torch.where(torch.rand(g.G, g.K, generator=gen) < 0.5, -1.0, 1.0)
        bias = 100.0 * sign
        residual = 0.5 * rn(g.G, g.N, g.P, g.Q, g.K)
    elif regime == "data":
        x = 3.0 + 0.03 * x
        w = w.abs()
    elif regime == "fused":
        bias = rn(g.G, g.K)
        residual = rn(g.G, g.N, g.P, g.Q, g.K)
        relu = True
    elif regime == "zerovar":
        bias = 0.3 * rn(g.G, g.K)
        k0 = zero_channel(g.K)
        w[:, k0] = 0
        bias[:, k0] = 40.0
    return dict(x=x, w=w, bias=bias, residual=residual, relu=relu)


def conv_epilogue(inp, g, stride, pad):
    """float64 [relu](conv(x, w) + bias + residual) as [G, N, P, Q, K]: the tensor whose statistics the
    epilogue takes (host stand-in for the device output, for the CPU discrimination proof)."""
    ys = []
    for i in range(g.G):
        y = F.conv2d(inp["x"][i].double().permute(0, 3, 1, 2), inp["w"][i].double().permute(0, 3, 1, 2), None,
                     stride, pad).permute(0, 2, 3, 1)
        if inp["bias"] is not None:
            y = y + inp["bias"][i].double()
        if inp["residual"] is not None:
            y = y + inp["residual"][i].double()
        ys.append(y.clamp_min(0) if inp["relu"] else y)
    return torch.stack(ys)
