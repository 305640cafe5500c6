"""float64 oracle of the generation path (ops/llama_decode.py, LLama.generate): single-query
attention with absolute-position RoPE over a cache, the prologue-aware skinny linear, the top-k /
inverse-CDF sampler, and last-position logits of a float64 LLama. Plain PyTorch on the CPU, written
from the definitions, sharing no code with the ops under test (the Philox uniforms excepted: they
are an input of the sampler, taken from ``sample_uniforms``)."""
import math

import torch

F64 = torch.float64


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------- RoPE
def rope64(x, pos, base=10000.0):
    """x [..., hd] (interleaved pairs) rotated at absolute positions ``pos`` (broadcast over the
    leading dims: a scalar, or a tensor shaped like x without its last dim)."""
    hd = x.shape[-1]
    inv = base ** (-torch.arange(0, hd, 2, dtype=F64) / hd)
    ang = torch.as_tensor(pos, dtype=F64)[..., None] * inv
    c, s = torch.cos(ang), torch.sin(ang)
    x = x.double()
    out = torch.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


def causal_attention64(qkv, H, hd):
    """qkv [B, S, 3*H*hd] -> [B, S, H*hd]: the training attention (RoPE at positions 0..S-1)."""
    B, S, _ = qkv.shape
    q, k, v = qkv.double().view(B, S, 3, H, hd).unbind(2)
    pos = torch.arange(S)[None, :, None].expand(B, S, H)
    q, k = rope64(q, pos), rope64(k, pos)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(hd)
    s = s.masked_fill(torch.ones(S, S).triu(1).bool(), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v).reshape(B, S, H * hd)


def attn_decode64(qkv, kc, vc, lens):
    """qkv [B, 3*H*hd], kc / vc [B, H, Smax, hd] (K rotated), lens [B] ->
    (out [B, H*hd], new K row [B, H, hd] rotated, new V row [B, H, hd]); a sequence with lens
    outside [0, Smax) gives zeros."""
    B, H, Smax, hd = kc.shape
    q, k, v = qkv.double().view(B, 3, H, hd).unbind(1)
    out = torch.zeros(B, H * hd, dtype=F64)
    kn, vn = torch.zeros(B, H, hd, dtype=F64), v.clone()
    for b in range(B):
        L = int(lens[b])
        if L < 0 or L >= Smax:
            continue
        qb, kb = rope64(q[b], L), rope64(k[b], L)
        kn[b] = kb
        keys = torch.cat([kc[b, :, :L].double(), kb[:, None]], 1)
        vals = torch.cat([vc[b, :, :L].double(), v[b][:, None]], 1)
        p = torch.softmax(torch.einsum("hd,hsd->hs", qb, keys) / math.sqrt(hd), -1)
        out[b] = torch.einsum("hs,hsd->hd", p, vals).reshape(-1)
    return out, kn, vn


# ----------------------------------------------------------------------------------- linear
def lin_rows64(x, w, residual=None, pro="none", gain=None, eps=1e-6):
    x = x.double()
    if pro == "rmsnorm":
        x = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * gain.double()
    elif pro == "swiglu":
        a, b = x[:, :x.shape[1] // 2], x[:, x.shape[1] // 2:]
        x = a / (1 + torch.exp(-a)) * b
    y = x @ w.double().t()
    return y if residual is None else y + residual.double()


# ---------------------------------------------------------------------------------- sampler
def kept64(row, top_k):
    """[V] bool: the top_k largest logits; among equals at the threshold the lowest indices."""
    V = row.numel()
    if top_k <= 0 or top_k >= V:
        return torch.ones(V, dtype=torch.bool)
    idx = torch.sort(row.double() + 0.0, descending=True, stable=True).indices[:top_k]  # stable: ties by index
    keep = torch.zeros(V, dtype=torch.bool)
    keep[idx] = True
    return keep


def cdf64(row, temperature, top_k):
    """(kept [V], normalised CDF [V] in vocabulary order over the kept set)."""
    keep = kept64(row, top_k)
    z = row.double() / temperature
    w = torch.where(keep, torch.exp(z - z[keep].max()), torch.zeros_like(z))
    c = torch.cumsum(w, 0)
    return keep, c / c[-1]


def sample64(row, temperature, top_k, u):
    """The first kept index whose CDF reaches u (greedy, lowest index on ties, at temperature 0)."""
    if temperature == 0:
        return int((row == row.max()).nonzero()[0])
    keep, c = cdf64(row, temperature, top_k)
    hit = (keep & (c >= u)).nonzero()
    return int(hit[0]) if len(hit) else int(keep.nonzero()[-1])


# ------------------------------------------------------------------------------------ model
def last_logits64(m64, seq):
    """Logits of the last position only (the head on one row: cheap at a 32000 vocabulary)."""
    with torch.no_grad():
        h = m64.last.run_layers(m64.first.embed(torch.tensor([seq])))[0, -1:]
        h = h / torch.sqrt((h * h).mean(-1, keepdim=True) + 1e-6) * m64.last.norm
        return (h @ m64.last.head.t())[0]


def greedy64(m64, prompts, steps):
    """Greedy continuation of each prompt (token lists) by ``steps`` tokens under ``m64`` ->
    (tokens [B][steps], logits [B][steps + 1][V]: entry i is the distribution token i is drawn
    from, the last one follows the final token)."""
    toks, logs = [], []
    for p in prompts:
        s, t, lg = list(p), [], []
        for _ in range(steps):
            lo = last_logits64(m64, s)
            lg.append(lo)
            t.append(int(lo.argmax()))
            s.append(t[-1])
        lg.append(last_logits64(m64, s))
        toks.append(t)
        logs.append(torch.stack(lg))
    return toks, logs


def exempt64(logits_row, frac=1e-3):
    """Is the float64 top-2 gap of this row below ``frac`` x its max-abs logit (a near-tie: an
    fp32 path may legitimately pick the other token)?"""
    top = torch.topk(logits_row, 2).values
    return float(top[0] - top[1]) < frac * float(logits_row.abs().max())
