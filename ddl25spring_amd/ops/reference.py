"""Pure-PyTorch reference implementations of every native op (fp32 math on bf16 storage).

Used (a) as the CPU execution path so the whole framework runs in GPU-less CI, and (b) as the
numerics oracle for the HIP kernels in ``tests/test_kernels_gpu.py``. They follow the same
layout contract as the kernels: NHWC activations with a leading client-group dimension
``[G, N, H, W, C]``, bf16 storage, fp32 accumulation.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F

# activation storage dtype of the CPU path: bf16 (mirrors the device numerics) or fp32 (a net in
# the fp32 precision mode runs its CPU ops inside ``storage(torch.float32)``)
_STORAGE = [torch.bfloat16]


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(_STORAGE[-1])


@contextlib.contextmanager
def storage(dtype):
    _STORAGE.append(dtype)
    try:
        yield
    finally:
        _STORAGE.pop()


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1)


def _is_gemm(geom) -> bool:
    """1x1 / stride 1 / no padding (every Linear layer): the conv is a plain GEMM over pixels."""
    return geom.R == 1 and geom.S == 1 and geom.stride == 1 and geom.pad == 0


def conv_fwd(x, w, geom, bias=None, relu=False, stats=None):
    G = geom.G
    if _is_gemm(geom):  # one batched matmul over the client groups (the CPU MLP path)
        y = torch.bmm(x.float().reshape(G, -1, geom.C), w.float().reshape(G, geom.K, geom.C).transpose(1, 2))
        if bias is not None:
            y = y + bias.float().reshape(G, 1, geom.K)
        if relu:
            y = y.clamp_min(0)
        if stats is not None:
            st = stats[:, 0] if stats.dim() == 4 else stats
            st[:, 0] += y.sum(1)
            st[:, 1] += (y * y).sum(1)
        return _bf(y).reshape(G, geom.N, geom.P, geom.Q, geom.K)
    outs = []
    for g in range(G):
        xi = nhwc_to_nchw(x[g].float())
        wi = w[g].float().permute(0, 3, 1, 2)  # [K, C, R, S]
        y = F.conv2d(xi, wi, None, geom.stride, geom.pad)
        y = nchw_to_nhwc(y)
        if bias is not None:
            y = y + bias[g].float()
        if relu:
            y = y.clamp_min(0)
        if stats is not None:
            flat = y.reshape(-1, geom.K)
            st = stats[g, 0] if stats.dim() == 4 else stats[g]
            st[0] += flat.sum(0)
            st[1] += (flat * flat).sum(0)
        outs.append(y)
    return _bf(torch.stack(outs)).contiguous()


def conv_dgrad(dy, w, geom, residual=None, mask=None):
    if _is_gemm(geom):
        G = geom.G
        dx = torch.bmm(dy.float().reshape(G, -1, geom.K), w.float().reshape(G, geom.K, geom.C))
        dx = dx.reshape(G, geom.N, geom.H, geom.W, geom.C)
        if residual is not None:
            dx = dx + residual.float()
        if mask is not None:
            dx = dx * (mask.float() > 0)
        return _bf(dx).contiguous()
    outs = []
    for g in range(geom.G):
        dyi = nhwc_to_nchw(dy[g].float())
        wi = w[g].float().permute(0, 3, 1, 2)
        dx = torch.nn.grad.conv2d_input((geom.N, geom.C, geom.H, geom.W), wi, dyi, geom.stride,
                                        geom.pad)
        dx = nchw_to_nhwc(dx)
        if residual is not None:
            dx = dx + residual[g].float()
        if mask is not None:
            dx = dx * (mask[g].float() > 0)
        outs.append(dx)
    return _bf(torch.stack(outs)).contiguous()


def conv_wgrad(dy, x, geom, dw, accumulate=True, scale=1.0):
    if _is_gemm(geom):
        G = geom.G
        gw = torch.bmm(dy.float().reshape(G, -1, geom.K).transpose(1, 2), x.float().reshape(G, -1, geom.C))
        gw = gw.reshape(G, geom.K, 1, 1, geom.C)
        if scale != 1.0:
            gw = gw * scale
        if accumulate:
            dw += gw
        else:
            dw.copy_(gw)
        return
    for g in range(geom.G):
        dyi = nhwc_to_nchw(dy[g].float())
        xi = nhwc_to_nchw(x[g].float())
        gw = torch.nn.grad.conv2d_weight(xi, (geom.K, geom.C, geom.R, geom.S), dyi, geom.stride,
                                         geom.pad)
        gw = gw.permute(0, 2, 3, 1)  # [K, R, S, C]
        if scale != 1.0:
            gw = gw * scale
        if accumulate:
            dw[g] += gw
        else:
            dw[g].copy_(gw)


def bn_finalize(stats, gamma, beta, running_mean, running_var, count, eps, momentum, training):
    if stats.dim() == 4:  # striped [G, S, 2, C]
        stats = stats.sum(1)
    if training:
        mean = stats[:, 0] / count
        var = (stats[:, 1] / count - mean * mean).clamp_min(0)
        if running_mean is not None:
            unb = var * count / max(count - 1, 1)
            running_mean.mul_(1 - momentum).add_(momentum * mean)
            running_var.mul_(1 - momentum).add_(momentum * unb)
    else:
        mean = running_mean.clone()
        var = running_var.clone()
    rstd = torch.rsqrt(var + eps)
    ga = gamma if gamma is not None else torch.ones_like(mean)
    be = beta if beta is not None else torch.zeros_like(mean)
    scale = ga * rstd
    shift = be - mean * scale
    return scale.contiguous(), shift.contiguous(), mean.contiguous(), rstd.contiguous()


def _act(y, act, slope=0.01):
    if act == 1:
        return y.clamp_min(0)
    if act == 2:
        return torch.where(y > 0, y, slope * y)
    if act == 3:
        return torch.tanh(y)
    if act == 4:
        return torch.sigmoid(y)
    return y


def _bn_act(y, act):
    # bn_apply's act code 3 is leaky(0.2) (act_fwd's 3 is tanh)
    return torch.where(y > 0, y, 0.2 * y) if act == 3 else _act(y, act)


def _bcast(v, x):
    # v [G, C] -> broadcast over x [G, ..., C]
    shape = [v.shape[0]] + [1] * (x.dim() - 2) + [v.shape[1]]
    return v.reshape(shape)


def bn_apply(x, scale, shift, r=None, rscale=None, rshift=None, act=0):
    y = x.float() * _bcast(scale, x) + _bcast(shift, x)
    if r is not None:
        rv = r.float()
        if rscale is not None:
            rv = rv * _bcast(rscale, x) + _bcast(rshift, x)
        y = y + rv
    return _bf(_bn_act(y, act)).contiguous()


def bn_bwd_reduce(dy, ymask, x, mean, rstd, dgamma=None, dbeta=None):
    d = dy.float()
    if ymask is not None:
        d = d * (ymask.float() > 0)
    xh = (x.float() - _bcast(mean, x)) * _bcast(rstd, x)
    dims = tuple(range(1, x.dim() - 1))
    s0 = d.sum(dims)
    s1 = (d * xh).sum(dims)
    if dbeta is not None:
        dbeta += s0
    if dgamma is not None:
        dgamma += s1
    return torch.stack([s0, s1], 1)


def bn_bwd_apply(dy, ymask, x, mean, rstd, gamma, sums, emit_dym=False):
    d = dy.float()
    if ymask is not None:
        d = d * (ymask.float() > 0)
    M = x[0].numel() // x.shape[-1]
    xh = (x.float() - _bcast(mean, x)) * _bcast(rstd, x)
    ga = gamma if gamma is not None else torch.ones_like(mean)
    dx = _bcast(ga * rstd, x) * (d - _bcast(sums[:, 0], x) / M - xh * _bcast(sums[:, 1], x) / M)
    dxb = _bf(dx).contiguous()
    if emit_dym:
        return dxb, _bf(d).contiguous()
    return dxb


def maxpool2_fwd(x):
    G, N, H, W, C = x.shape
    xi = x.float().reshape(G * N, H, W, C).permute(0, 3, 1, 2)
    y = F.max_pool2d(xi, 2)
    return _bf(y.permute(0, 2, 3, 1).reshape(G, N, H // 2, W // 2, C)).contiguous()


def maxpool2_bwd(x, dy):
    G, N, H, W, C = x.shape
    with torch.enable_grad():  # may be called from inside an autograd backward
        xi = x.float().reshape(G * N, H, W, C).permute(0, 3, 1, 2).detach().requires_grad_(True)
        y = F.max_pool2d(xi, 2)
        g = dy.float().reshape(G * N, H // 2, W // 2, C).permute(0, 3, 1, 2)
        (dx,) = torch.autograd.grad(y, xi, g)
    return _bf(dx.permute(0, 2, 3, 1).reshape(G, N, H, W, C)).contiguous()


def avgpool_fwd(x):
    G, N, H, W, C = x.shape
    return _bf(x.float().mean((2, 3))).contiguous()


def avgpool_bwd(dy, H, W):
    G, N, C = dy.shape
    return _bf((dy.float() / (H * W)).reshape(G, N, 1, 1, C).expand(G, N, H, W, C)).contiguous()


def dropout_mask(shape, p, seed, offset, device):
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 1000003 + int(offset)) % (2 ** 63))
    return (torch.rand(shape, generator=g) > p).to(device)


def dropout(x, p, seed, offset):
    if p <= 0:
        return x.clone()
    m = dropout_mask(x.shape, p, seed, offset, x.device)
    return _bf(x.float() * m / (1 - p)).contiguous()


def act_fwd(x, act, slope=0.01):
    return _bf(_act(x.float(), act, slope)).contiguous()


def act_bwd(y, dy, act, slope=0.01):
    yf = y.float()
    d = dy.float()
    if act == 1:
        d = d * (yf > 0)
    elif act == 3:
        d = d * (1 - yf * yf)
    elif act == 4:
        d = d * yf * (1 - yf)
    else:
        d = torch.where(yf > 0, d, slope * d)
    return _bf(d).contiguous()


def bn_stats(x, stats):
    C = x.shape[-1]
    xf = x.float().reshape(x.shape[0], -1, C)
    st = stats[:, 0] if stats.dim() == 4 else stats
    st[:, 0] += xf.sum(1)
    st[:, 1] += (xf * xf).sum(1)


def bce_logits(l, t):
    """-> (sum loss, dloss/dl)."""
    loss = (l.clamp_min(0) - l * t + torch.log1p(torch.exp(-l.abs()))).sum()
    return loss, torch.sigmoid(l) - t


def channel_sum(x, out):
    C = x.shape[-1]
    out += x.float().reshape(x.shape[0], -1, C).sum(1)


def ce_fwd_bwd(logits, labels, targets, ncls, scale, loss=None, correct=None, want_grad=True):
    # logits [G, N, ld]
    z = logits.float()[..., :ncls]
    logp = F.log_softmax(z, -1)  # (z - max) - log(sum): z - logsumexp(z) rounds at the logits' magnitude
    if targets is not None:
        t = targets.float()
        lrow = -(t * logp).sum(-1)
        tsum = t.sum(-1, keepdim=True)
        grad = torch.exp(logp) * tsum - t
        ytrue = t.argmax(-1)
    else:
        lrow = -logp.gather(-1, labels.long().unsqueeze(-1)).squeeze(-1)
        grad = torch.exp(logp)
        grad.scatter_add_(-1, labels.long().unsqueeze(-1), -torch.ones_like(lrow).unsqueeze(-1))
        ytrue = labels.long()
    if loss is not None:
        loss += lrow.sum(-1) * scale
    if correct is not None:
        correct += (z.argmax(-1) == ytrue).sum(-1).to(correct.dtype)
    if not want_grad:
        return None
    full = torch.zeros_like(logits, dtype=torch.float32)
    full[..., :ncls] = grad * scale
    return _bf(full).contiguous()


def sgd(p, g, mom, shadow, lr, wd, momentum, dampening, nesterov, first_step, grad_scale=1.0):
    d = g * grad_scale + wd * p
    if momentum != 0:
        if first_step:
            mom.copy_(d)
        else:
            mom.mul_(momentum).add_((1 - dampening) * d)
        d = d + momentum * mom if nesterov else mom
    p.sub_(lr * d)
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def sgd_direct(p, g, shadow, dmap, lr, grad_scale=1.0):
    """Columns marked in ``dmap`` (per 16) were updated inside the backward: shadow refresh only;
    the rest take a plain SGD step and have their gradient zeroed (optim.hip sgd_direct_kernel)."""
    rest = (dmap == 0).repeat_interleave(16).to(p.device)
    p[:, rest] -= lr * grad_scale * g[:, rest]
    g[:, rest] = 0
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def adam(p, g, m, v, shadow, lr, beta1, beta2, eps, wd, step, decoupled, grad_scale=1.0):
    g = g * grad_scale
    if decoupled:
        p.mul_(1 - lr * wd)
    else:
        g = g + wd * p
    m.mul_(beta1).add_((1 - beta1) * g)
    v.mul_(beta2).add_((1 - beta2) * g * g)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    p.sub_((lr / bc1) * m / denom)
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


def weighted_sum(src, coeff, out, accumulate=False):
    r = (coeff.reshape(-1, 1).to(src.dtype) * src).sum(0)
    if accumulate:
        out += r
    else:
        out.copy_(r)


def broadcast_rows(src, dst, shadow=None):
    dst.copy_(src.unsqueeze(0).expand_as(dst))
    if shadow is not None:
        shadow.copy_(dst.to(shadow.dtype))


def gram(X, center=None):
    Xc = X - center if center is not None else X
    return Xc @ Xc.t()


def coord_select(X, mode, trim=0):
    s, _ = torch.sort(X, 0)
    K = X.shape[0]
    if mode == 0:
        return 0.5 * (s[(K - 1) // 2] + s[K // 2])
    return s[trim:K - trim].mean(0)


def bulyan_select(gram, f, keys):
    """bulyan_select_kernel's twin in fp32 -> (the winners' scores [theta], sel as a list): the
    kernel's distances, the nb_t smallest among the clients still in R added in ascending order,
    the least (score, key) picked and removed, theta = K - 2f times."""
    K = gram.shape[0]
    inf = float("inf")
    sq = torch.diagonal(gram)
    d2 = sq[:, None] + sq[None, :] - 2 * gram
    d2 = torch.where(torch.isfinite(d2), d2.clamp_min(0), torch.full_like(d2, inf))
    d2.fill_diagonal_(inf)
    left, sel, win = list(range(K)), [], []
    for t in range(K - 2 * f):
        n1 = K - t
        nb = min(max(n1 - f - 2, 1), n1 - 1)
        idx = torch.tensor(left)
        near = torch.sort(d2[idx][:, idx], 1).values
        score = torch.zeros(n1, dtype=gram.dtype)
        for j in range(nb):
            score = score + near[:, j]
        sc = score.tolist()  # in [0, +inf], never NaN
        w = min(range(n1), key=lambda a: (sc[a], int(keys[left[a]])))
        sel.append(left.pop(w))
        win.append(sc[w])
    return torch.tensor(win, dtype=gram.dtype), sel


def bulyan_coord(X, sel, beta):
    """bulyan_coord_kernel's twin: the window compared in double, its fp32 sum in ascending order."""
    s = X.index_select(0, sel.long())
    s = torch.sort(torch.where(torch.isnan(s), torch.full_like(s, float("inf")), s), 0).values
    theta = s.shape[0]
    span = theta - beta
    mid = s[(theta - 1) // 2].double() + s[theta // 2].double()
    lo = ((s[:span].double() + s[beta:].double()) < mid).sum(0)
    acc = torch.zeros(s.shape[1], dtype=s.dtype)
    for j in range(beta):
        acc = acc + s.gather(0, (lo + j)[None])[0]
    return acc / beta


# ------------------------------------------------- clipped aggregation (clip_agg.hip), torch twins
def update_sqnorm(rows, center=None):
    d = rows if center is None else rows - center  # rounded to fp32, then squared in double
    return d.double().square().sum(1)


def clip_scales(sq, coeff, clip):
    nrm = sq.double().sqrt()
    one = torch.ones_like(nrm)
    s = torch.where(nrm <= clip, one, clip / nrm).float()
    cs = coeff.float() * s
    cs = torch.where(torch.isfinite(sq), cs, torch.zeros_like(cs))  # NaN / Inf row: skipped
    return nrm.float(), cs


def gm_scales(sq, coeff, nu, init, total=None):
    """gm_scales_kernel's twin, in double: -> (norms fp32, cs fp32, beta_sum float64 [1])."""
    q = sq.double()
    nrm = q.sqrt()
    beta = coeff.double() if init else coeff.double() / nrm.clamp_min(nu)
    beta = torch.where(q < float("inf"), beta, torch.zeros_like(beta))  # NaN / Inf row: weight 0
    S = 0.0
    for b in beta.tolist():  # index order
        S += b
    T = S if total is None else float(total)
    cs = torch.zeros_like(beta) if T == 0.0 else beta / T
    return nrm.float(), cs.float(), torch.tensor([S], dtype=torch.float64)


def root_dots(rows, root, center=None):
    """FLTrust's dot products and squared norms against the root update, from the definition: the
    differences rounded to fp32, their products in double -> (dots, sq) float64 [G + 1]."""
    d = (rows if center is None else rows - center).double()
    d0 = (root if center is None else root - center).double()
    sq0 = (d0 * d0).sum().reshape(1)
    return torch.cat([(d * d0).sum(1), sq0]), torch.cat([(d * d).sum(1), sq0])


def trust_scales(dots, sq, coeff, total=None):
    """FLTrust's trust scores and row scales from the definition, in double:
    -> (cos fp32, norms fp32, cs fp32, beta_sum float64 [1])."""
    G = coeff.numel()
    dots, sq = dots.double(), sq.double()
    nrm, n0 = sq[:G].sqrt(), sq[G].sqrt()
    live = torch.isfinite(sq[:G]) & torch.isfinite(dots[:G]) & (nrm > 0) & torch.isfinite(sq[G]) & (n0 > 0)
    zero = torch.zeros_like(nrm)
    cos = torch.where(live, (dots[:G] / (nrm * n0)).clamp(-1.0, 1.0), torch.full_like(nrm, float("nan")))
    beta = torch.where(live, coeff.double() * cos.clamp_min(0.0), zero)
    S = 0.0
    for b in beta.tolist():  # index order
        S += b
    T = S if total is None else float(total)
    cs = zero if T == 0.0 else torch.where(live, beta * (n0 / nrm) / T, zero)
    return cos.float(), nrm.float(), cs.float(), torch.tensor([S], dtype=torch.float64)


def clipped_sum(rows, center, cs, out, accumulate=False):
    acc = out.clone() if accumulate else torch.zeros_like(out)
    for k, c in enumerate(cs.tolist()):
        if c == 0.0:
            continue  # not read: 0 * NaN would be NaN
        d = rows[k] if center is None else rows[k] - center
        acc = acc + cs[k] * d  # product rounded, then added, in row order
    out.copy_(acc)


def rlr_flip(delta, votes, theta):
    th = torch.tensor(theta, dtype=torch.float32)  # the kernel compares in fp32
    delta.copy_(torch.where(votes.abs() < th, -delta, delta))


def rlr_sum(rows, center, cs, delta, votes=None, theta=None):
    """rlr_sum_kernel's twin: clipped_sum's loop, the signs of the same differences counted beside it."""
    acc = torch.zeros_like(delta)
    s = torch.zeros_like(delta)
    for k, c in enumerate(cs.tolist()):
        if c == 0.0:
            continue  # not read, no vote
        d = rows[k] if center is None else rows[k] - center
        acc = acc + cs[k] * d
        s = s + ((d > 0).float() - (d < 0).float())  # both false for +-0 and NaN
    delta.copy_(acc)
    if theta is not None:
        rlr_flip(delta, s, theta)
    if votes is not None:
        votes.copy_(s)


def cc_step(rows, center, ctr_in, v_in, cs, v_out, ctr_out, want_norms=True):
    """cc_step_kernel's twin: the sum starts from v_in and adds the rows in order."""
    acc = v_in.clone()
    live = [k for k, c in enumerate(cs.tolist()) if c != 0.0]
    for k in live:
        acc = acc + cs[k] * (rows[k] - ctr_in)
    ctr = acc if center is None else center + acc
    v_out.copy_(acc)
    ctr_out.copy_(ctr)
    if not want_norms:
        return None
    sq = torch.full((rows.shape[0],), float("inf"), dtype=torch.float64)
    for k in live:
        sq[k] = (rows[k] - ctr).double().square().sum()
    return sq


# ------------------------------------------------- colluding attacks (collude.hip), float64 twin
def collude_rows(src, src_rows, center, dst, dst_rows, mode, coef):
    """collude_kernel's definition in torch float64: one pass over the source rows in table order,
    moments of the finite d = fl32(src - center) shifted by each coordinate's first finite d."""
    n = dst.shape[1]
    shift = torch.zeros(n, dtype=torch.float64)
    s1, s2, m = torch.zeros_like(shift), torch.zeros_like(shift), torch.zeros_like(shift)
    for j in src_rows.tolist():
        d = src[j] if center is None else src[j] - center  # rounded to fp32
        ok = torch.isfinite(d)
        d = torch.where(ok, d, torch.zeros_like(d)).double()
        shift = torch.where(ok & (m == 0), d, shift)
        t = torch.where(ok, d - shift, torch.zeros_like(d))
        s1, s2, m = s1 + t, s2 + t * t, m + ok.double()
    cnt = m.clamp_min(1.0)
    mu = shift + s1 / cnt
    if mode == 0:
        p = mu - coef * ((s2 - s1 * s1 / cnt) / cnt).clamp_min(0.0).sqrt()
    else:
        p = -coef * mu
    p = torch.where(m > 0, p, torch.zeros_like(p)).float()
    row = p if center is None else center + p
    for t in dst_rows.tolist():
        dst[t].copy_(row)


# ------------------------------------------------ FedProx / FedOpt (fedopt.hip), fp32 torch twins
def _s32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def sgd_corrected(p, g, mom, shadow, term, lr, wd, momentum, dampening, nesterov, first_step, grad_scale=1.0):
    """Rows p/g/mom/shadow [G, P] and the correction term (broadcastable to them: FedProx's
    ``mu * (p - anchor)``, SCAFFOLD's ``c - bank[slot_client]``): every operation a separate fp32
    rounding, in sgd_corrected_kernel's order."""
    lr, wd, mo, gs = (_s32(v) for v in (lr, wd, momentum, grad_scale))
    d = g * gs + wd * p
    d = d + term
    if momentum != 0:
        if first_step:
            mom.copy_(d)
        else:
            mom.copy_(mo * mom + (_s32(1.0) - _s32(dampening)) * d)
        d = d + mo * mom if nesterov else mom
    p.copy_(p - lr * d)
    if shadow is not None:
        shadow.copy_(p.to(shadow.dtype))


SERVER_OPT_KINDS = {"sgdm": 0, "adagrad": 1, "adam": 2, "yogi": 3}


def server_opt(w, x, m, v, kind, x_is_delta, lr, beta1, beta2, tau):
    """In place on w, m, v [n] (fedopt.hip server_opt_kernel, the same operation order); a
    coordinate whose delta is NaN / Inf keeps its w, m, v."""
    lr, b1, b2, tau = (_s32(s) for s in (lr, beta1, beta2, tau))
    d = x if x_is_delta else x - w
    ok = torch.isfinite(d)
    d = torch.where(ok, d, torch.zeros_like(d))
    if kind == "sgdm":
        m1 = b1 * m + d
        w1 = w + lr * m1
    else:
        omb1, omb2 = _s32(1.0) - b1, _s32(1.0) - b2
        m1 = b1 * m + omb1 * d
        if kind == "adagrad":
            v1 = v + d * d
        elif kind == "adam":
            v1 = b2 * v + omb2 * d * d
        else:
            d2 = d * d
            v1 = v - omb2 * d2 * torch.sign(v - d2)
        w1 = w + lr * m1 / (v1.sqrt() + tau)
        v.copy_(torch.where(ok, v1, v))
    m.copy_(torch.where(ok, m1, m))
    w.copy_(torch.where(ok, w1, w))


def server_opt_rows(rows, coeff, w, m, v, kind, x_is_delta, lr, beta1, beta2, tau):
    x = torch.empty_like(w)
    weighted_sum(rows, coeff, x)
    server_opt(w, x, m, v, kind, x_is_delta, lr, beta1, beta2, tau)


# ------------------------------------------------------- SCAFFOLD (scaffold.hip), fp32 torch twins
def scaffold_finish(rows, x, c, bank, slot_client, inv_klr, inv_n, dc, apply_c):
    """scaffold_finish_kernel's order: the slots from 0 upward, acc from 0; a NaN / Inf delta
    leaves its bank entry untouched and adds nothing."""
    inv_n = _s32(inv_n)
    acc = torch.zeros_like(x)
    for g, cl in enumerate(slot_client.tolist()):
        t = (x - rows[g]) * inv_klr[g]
        delta = t - c
        ok = torch.isfinite(delta)
        delta = torch.where(ok, delta, torch.zeros_like(delta))
        bank[cl].copy_(torch.where(ok, bank[cl] + delta, bank[cl]))
        acc = torch.where(ok, acc + delta * inv_n, acc)
    dc.copy_(acc)
    if apply_c:
        c.copy_(c + acc)


CLIP_NOISE_TAG = 0x3C6EF372
_M32 = 0xFFFFFFFF


def _mulhilo_t(a: int, b):
    """(hi, lo) 32-bit words of a * b for a 32-bit constant a and an int64 tensor b < 2**32, in
    int64 arithmetic (16-bit limbs of b: no product reaches 2**63)."""
    p0, p1 = a * (b & 0xFFFF), a * (b >> 16)
    t = p0 + ((p1 & 0xFFFF) << 16)
    return (p1 >> 16) + (t >> 32), t & _M32


def philox4x32_t(c0, c1, c2, c3, k0: int, k1: int):
    """Philox-4x32-10 (csrc/include/ddl_common.h) on int64 tensors holding 32-bit words."""
    for _ in range(10):
        hi0, lo0 = _mulhilo_t(0xD2511F53, c0)
        hi1, lo1 = _mulhilo_t(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def update_noise(n: int, seed: int, round: int, offset: int = 0):
    """z[offset : offset + n] of the N(0, 1) stream of (seed, round): apply_update_kernel's draws."""
    q0 = offset >> 2
    q = torch.arange(q0, ((offset + n + 3) >> 2), dtype=torch.int64)
    zero = torch.zeros_like(q)
    r = philox4x32_t(q & _M32, q >> 32, zero + CLIP_NOISE_TAG, zero + (round & _M32),
                     seed & _M32, (seed >> 32) & _M32)
    u = [((x >> 8).float() + 1.0) * (1.0 / 16777216.0) for x in r]  # (0, 1], fp32 exactly
    two_pi = torch.tensor(6.2831853071795864769, dtype=torch.float32)
    r0, r1 = torch.sqrt(-2.0 * torch.log(u[0])), torch.sqrt(-2.0 * torch.log(u[2]))
    a0, a1 = two_pi * u[1], two_pi * u[3]
    z = torch.stack([r0 * torch.cos(a0), r0 * torch.sin(a0), r1 * torch.cos(a1), r1 * torch.sin(a1)], 1)
    lo = offset - 4 * q0
    return z.reshape(-1)[lo:lo + n]


def apply_update(out, center, delta, std=0.0, seed=0, round=0, offset=0):
    o = delta if center is None else center + delta
    if std != 0.0:
        o = o + torch.tensor(std, dtype=torch.float32) * update_noise(out.numel(), seed, round, offset)
    out.copy_(o)


# ------------------------------------------- compressed uploads (compress.hip), fp32 torch twins
QUANT_TAG = 0x510E527F
_EXP_MASK = 0x7F800000


def _corrected_update(rows, x, bank, ids, g):
    """-> (u, e, magnitude bits, finite): u = (y - x) + e, or y - x without a bank."""
    e = None if bank is None else bank[ids[g]]
    d = rows[g] - x
    u = (d if e is None else d + e).contiguous()
    key = u.view(torch.int32) & 0x7FFFFFFF
    return u, e, key, key < _EXP_MASK


def topk_compress(rows, x, bank, slot_client, k, nnz):
    """compress.hip's top-k, bit for bit: tau is the k-th largest magnitude bit pattern among the
    finite non-zero ones (the smallest when there are fewer), every entry that reaches it is kept."""
    ids = None if slot_client is None else slot_client.tolist()
    for g in range(rows.shape[0]):
        u, e, key, finite = _corrected_update(rows, x, bank, ids, g)
        counts = finite & (key != 0)
        n = int(counts.sum())
        keep = torch.zeros_like(counts)
        if n:
            tau = torch.sort(key[counts], descending=True).values[min(int(k), n) - 1]
            keep = counts & (key >= tau)
        rows[g].copy_(torch.where(keep | ~finite, x + u, x))
        if e is not None:
            e.copy_(torch.where(finite, torch.where(keep, torch.zeros_like(u), u), e))
        nnz[g] = int(keep.sum())


def quantize_draws(P: int, client: int, seed: int, round: int):
    """r [P] in (0, 1]: word j & 3 of philox4x32(counter (j >> 2, client, QUANT_TAG, round), key seed)."""
    q = torch.arange((P + 3) >> 2, dtype=torch.int64)
    zero = torch.zeros_like(q)
    r = philox4x32_t(q & _M32, zero + (int(client) & _M32), zero + QUANT_TAG, zero + (round & _M32),
                     seed & _M32, (seed >> 32) & _M32)
    w = torch.stack(r, 1).reshape(-1)[:P]
    return ((w >> 8).float() + 1.0) * (1.0 / 16777216.0)


def quantize_compress(rows, x, bank, slot_client, bits, seed, round, levels=None, scales=None):
    """quantize_kernel's operations in its order, in fp32 torch."""
    G, P = rows.shape
    L = (1 << (bits - 1)) - 1
    fL = _s32(float(L))
    nb = (P + 255) // 256
    ids = slot_client.tolist()
    for g in range(G):
        u, e, key, finite = _corrected_update(rows, x, bank, ids, g)
        mag = torch.where(finite, key, torch.zeros_like(key)).view(torch.float32)
        pad = torch.zeros(nb * 256)
        pad[:P] = mag
        s = pad.reshape(nb, 256).max(1).values
        sj = s.repeat_interleave(256)[:P]
        live = finite & (sj > 0)
        a = (mag / torch.where(live, sj, torch.ones_like(sj))) * fL
        fl = torch.floor(a)
        up = (a - fl) >= quantize_draws(P, ids[g], seed, round)
        lv = torch.clamp(fl + up.float(), max=float(L))
        lv = torch.where(live, lv, torch.zeros_like(lv))
        q = sj * (lv / fL)
        neg = u.view(torch.int32) < 0
        q = torch.where(neg, -q, q)
        rows[g].copy_(torch.where(finite, x + q, x + u))
        if e is not None:
            e.copy_(torch.where(finite, u - q, e))
        if levels is not None:
            levels[g].copy_(torch.where(neg, -lv, lv).to(torch.int8))
        if scales is not None:
            scales[g].copy_(s)


# ----------------------------------------- secure aggregation (secagg.hip), int64 torch twins
SECAGG_TAG = 0x9B05688C
SECAGG_MAX_CLIENTS = 65536


def secagg_pair_mask(P: int, a: int, b: int, seed: int, round: int):
    """m(a, b, e) for e in [0, P), a <= b, as int64 holding 32-bit words: word e & 3 of
    philox4x32(counter (Q_lo, Q_hi, (a << 16) | b, round), key (seed_lo ^ SECAGG_TAG, seed_hi))."""
    q = torch.arange((P + 3) >> 2, dtype=torch.int64)
    zero = torch.zeros_like(q)
    r = philox4x32_t(q & _M32, q >> 32, zero + (((a << 16) | b) & _M32), zero + (round & _M32),
                     (seed & _M32) ^ SECAGG_TAG, (seed >> 32) & _M32)
    return torch.stack(r, 1).reshape(-1)[:P]


def _secagg_signed_pair(P, i, j, seed, round):
    """s_ij m(min, max, .) for i != j: +m for i < j, -m for i > j."""
    m = secagg_pair_mask(P, min(i, j), max(i, j), seed, round)
    return m if i < j else -m


def _to_i32(t):
    """int64 holding any integer -> its residue mod 2^32 as int32 bits."""
    t = t & _M32
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


def secagg_encode(rows, center, cs, n: int, frac_bits: int):
    """-> (q [G, P] int64, sat [G] int64): the fixed-point updates of secagg_mask_kernel."""
    G, P = rows.shape
    lim = (2 ** 31 - 1) // n
    q = torch.zeros(G, P, dtype=torch.int64)
    sat = torch.zeros(G, dtype=torch.int64)
    for g, k in enumerate(cs.tolist()):
        if k == 0.0:
            continue  # not read
        d = rows[g] if center is None else rows[g] - center
        p = cs[g] * d  # each rounded to fp32
        r = torch.round(p.double() * float(1 << frac_bits))  # ties to even
        nan = torch.isnan(r)
        over = nan | (r.abs() > lim)
        r = torch.where(nan, torch.zeros_like(r), r.clamp(-lim, lim))
        q[g] = r.to(torch.int64)
        sat[g] = int(over.sum())
    return q, sat


def secagg_mask(rows, center, cs, slot_client, cohort, frac_bits, seed, round, words, sat):
    G, P = rows.shape
    ids, U = slot_client.tolist(), cohort.tolist()
    q, over = secagg_encode(rows, center, cs, len(U), frac_bits)
    for g, i in enumerate(ids):
        y = q[g] + secagg_pair_mask(P, i, i, seed, round)
        for j in U:
            if j != i:
                y = y + _secagg_signed_pair(P, i, j, seed, round)
        words[g].copy_(_to_i32(y))
    sat.copy_(over.to(torch.int32))


def secagg_sum(words, out):
    out.copy_(_to_i32(words.to(torch.int64).sum(0)))


def secagg_open(words, survivors, dropped, frac_bits, seed, round, delta):
    P = words.shape[1]
    T = words.to(torch.int64).sum(0)
    D = [] if dropped is None else dropped.tolist()
    for i in survivors.tolist():
        T = T - secagg_pair_mask(P, i, i, seed, round)
        for d in D:
            T = T - _secagg_signed_pair(P, i, d, seed, round)
    # int32 -> fp32 rounds to nearest even; the power of two is exact
    delta.copy_(_to_i32(T).to(torch.float32) * (1.0 / float(1 << frac_bits)))


def mse_kl(xr, x, mu, lv, kl_w=1.0):
    mse = ((xr - x) ** 2).sum()
    kl = -0.5 * (1 + lv - mu * mu - lv.exp()).sum()
    return mse + kl_w * kl


# ------------------------------------------------------------------------- Philox (numpy twin)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint32 arrays (csrc/include/ddl_common.h philox4x32)."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    for _ in range(10):
        p0 = _M0 * c0.astype(np.uint64)
        p1 = _M1 * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = np.uint32((int(k0) + int(_W0)) & 0xFFFFFFFF)
        k1 = np.uint32((int(k1) + int(_W1)) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def _unit(x):  # (0, 1], u32_to_unit
    return ((x >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)


def gan_inputs(desc, steps: int, B: int, nz: int):
    """nn_ops.hip gan_inputs_kernel on the host: desc [(seed, n, off), ...] per slot ->
    (idx int64 [steps, G*B], z fp32 [steps, G, B, nz])."""
    G = len(desc)
    idx = np.empty((steps, G * B), dtype=np.int64)
    z = np.empty((steps, G, B, nz), dtype=np.float32)
    for g, (seed, n, off) in enumerate(desc):
        k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        e = np.arange(steps * B, dtype=np.uint64)
        zeros = np.zeros_like(e, dtype=np.uint32)
        r = philox4x32(e.astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32), zeros + np.uint32(0x1d872b41),
                       zeros, k0, k1)
        u = (r[0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)
        idx[:, g * B:(g + 1) * B] = (u.astype(np.int64) + int(off)).reshape(steps, B)
        e = np.arange(steps * B * nz, dtype=np.uint64)
        zeros = np.zeros_like(e, dtype=np.uint32)
        r = philox4x32(e.astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32), zeros + np.uint32(0x6a09e667),
                       zeros, k0, k1)
        u1 = np.maximum(_unit(r[0]), np.float32(1e-12))
        u2 = _unit(r[1])
        zz = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.28318530717958648) * u2)
        z[:, g] = zz.astype(np.float32).reshape(steps, B, nz)
    return torch.from_numpy(idx), torch.from_numpy(z)
