"""Ops of the fp32 LLaMA's generation path (csrc/kernels/llama_decode.hip): a skinny-row linear with
fused prologues, single-query attention over a KV cache with the step's row appended in the same
launch, the prefill's cache append, and a sampler that also carries the step's state.

Every function writes into caller-provided buffers (nothing is allocated inside a step, so a step
can be captured into one HIP graph) and returns its output buffer. CPU tensors run the PyTorch fp32
references below, with the same semantics — frozen sequences, tie rules, Philox uniforms — so
``LLama.generate`` works and is tested without a GPU.

Sequence state (all int32, on the tensors' device): ``lens[b]`` = rows of sequence b in the cache;
a sequence with ``lens[b]`` outside ``[0, Smax)`` is frozen (the attention stores nothing and
returns zeros, the sampler leaves its ``lens``); ``finished[b]`` is set once ``eos_id`` is drawn,
after which the sequence emits ``eos_id`` and keeps its ``lens``; ``step[b]`` is the row's Philox
counter and output column (one counter per row: each row's workgroup advances its own).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import reference as ref
from ._lib import check, ptr, stream
from .llama_f32 import ATTN_HD

vp, i32, f32, u64 = _lib.vp, _lib.i32, _lib.f32, _lib.u64
_lib.register_signatures({
    "ddl_lin_rows_f32": [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "ddl_attnf_decode": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp],
    "ddl_kv_append": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "ddl_sample_f32": [vp, i32, i32, f32, i32, u64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp],
})

LIN_ROWS_MAX_T = 16
TOP_K_MAX = 1024
PROLOGUES = {"none": 0, "rmsnorm": 1, "swiglu": 2}
ATTN_REC_EXTRA = 2  # floats of a split record beside its HD accumulators: max, sum


def K():
    return _lib.kernels()


# --------------------------------------------------------------------------------- lin_rows
def lin_rows_launch(x, w, out, residual=None, pro="none", gain=None, eps=1e-6, T=None, C=None) -> int:
    """The raw launcher's return code (0, or hipErrorInvalidValue without a launch)."""
    Kout = w.shape[0]
    T = x.shape[0] if T is None else T
    C = w.shape[1] if C is None else C
    return int(K().ddl_lin_rows_f32(ptr(x), ptr(w), ptr(residual), ptr(gain), ptr(out), T, C, Kout,
                                    PROLOGUES[pro], float(eps), stream()))


def lin_rows_ref(x, w, residual=None, pro="none", gain=None, eps=1e-6):
    if pro == "rmsnorm":
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gain
    elif pro == "swiglu":
        a, b = x.chunk(2, -1)
        x = torch.nn.functional.silu(a) * b
    y = x @ w.t()
    return y if residual is None else y + residual


def lin_rows(x, w, out, residual=None, pro="none", gain=None, eps=1e-6):
    """out[T, K] = pro(x)[T, C] @ w[K, C]^T (+ residual[T, K]), 1 <= T <= 16, C % 4 == 0.
    ``pro``: "none"; "rmsnorm" (``gain`` [C], ``eps``); "swiglu" (x is [T, 2C] = [a | b])."""
    if pro not in PROLOGUES:
        raise ValueError(f"lin_rows: prologue {pro!r} not in {tuple(PROLOGUES)}")
    if not x.is_cuda:
        out.copy_(lin_rows_ref(x, w, residual, pro, gain, eps))
        return out
    T, Cx = x.shape
    Kout, C = w.shape
    if Cx != (2 * C if pro == "swiglu" else C) or out.shape != (T, Kout):
        raise ValueError(f"lin_rows: x {tuple(x.shape)}, w {tuple(w.shape)}, out {tuple(out.shape)} ({pro})")
    for t in (x, w, out, residual, gain):
        if t is not None and not (t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError("lin_rows: contiguous fp32 tensors only")
    check(lin_rows_launch(x, w, out, residual, pro, gain, eps), "lin_rows_f32")
    return out


# --------------------------------------------------------------------------- decode attention
def attn_splits(max_len: int) -> int:
    """Key splits of the decode attention, from the cache capacity alone (never from ``lens``: the
    launch is captured into a graph): one workgroup covers 64 keys per sweep, a split about 512."""
    return max(1, min(16, (max_len + 511) // 512))


def attn_workspace(B: int, H: int, hd: int, splits: int, device):
    """Per-split records of ``attn_decode`` (``None`` for a single split)."""
    if splits <= 1:
        return None
    return torch.empty(B, H, splits, hd + ATTN_REC_EXTRA, dtype=torch.float32, device=device)


def _rope_at(x, cos, sin, pos):
    """x [B, H, hd] rotated at per-sequence positions ``pos`` [B] (interleaved pairs)."""
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    out = torch.empty_like(x)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    out[..., 0::2] = x0 * c - x1 * s
    out[..., 1::2] = x0 * s + x1 * c
    return out


def attn_decode_ref(qkv, kc, vc, lens, cos, sin, out):
    B, H, Smax, hd = kc.shape
    q, k, v = qkv.view(B, 3, H, hd).unbind(1)
    scale = 1.0 / math.sqrt(hd)
    for b in range(B):
        L = int(lens[b])
        if L < 0 or L >= Smax:
            out[b].zero_()
            continue
        pos = torch.tensor([L])
        qb, kb = _rope_at(q[b:b + 1], cos, sin, pos)[0], _rope_at(k[b:b + 1], cos, sin, pos)[0]
        kc[b, :, L], vc[b, :, L] = kb, v[b]
        s = torch.einsum("hd,hsd->hs", qb, kc[b, :, :L + 1]) * scale
        out[b] = torch.einsum("hs,hsd->hd", torch.softmax(s, -1), vc[b, :, :L + 1]).reshape(H * hd)
    return out


def attn_decode(qkv, kc, vc, lens, cos, sin, out, splits: int = 1, ws=None):
    """One query per sequence: rotate q, k at position ``lens[b]``, store k, v into cache row
    ``lens[b]``, attend over rows ``0..lens[b]``. qkv [B, 3*H*hd], kc / vc [B, H, Smax, hd] (K
    rotated), cos / sin with Smax rows, out [B, H*hd]. ``lens`` is not modified."""
    B, H, Smax, hd = kc.shape
    if hd not in ATTN_HD:
        raise ValueError(f"attn_decode: head_dim {hd} not in {ATTN_HD}")
    if cos.shape[0] < Smax or qkv.shape != (B, 3 * H * hd) or out.shape != (B, H * hd):
        raise ValueError("attn_decode: shapes do not match the cache")
    if not qkv.is_cuda:
        return attn_decode_ref(qkv, kc, vc, lens, cos, sin, out)
    if splits > 1 and (ws is None or ws.numel() < B * H * splits * (hd + ATTN_REC_EXTRA)):
        raise ValueError("attn_decode: splits > 1 needs the attn_workspace records")
    for t in (qkv, kc, vc, lens, cos, sin, out):
        if not t.is_contiguous():
            raise ValueError("attn_decode: contiguous tensors only")
    if lens.dtype != torch.int32:
        raise ValueError("attn_decode: lens must be int32")
    check(K().ddl_attnf_decode(ptr(qkv), ptr(kc), ptr(vc), ptr(lens), ptr(cos), ptr(sin), ptr(out), ptr(ws), B, H,
                               hd, Smax, int(splits), 1.0 / math.sqrt(hd), stream()), "attnf_decode")
    return out


# ------------------------------------------------------------------------------ prefill append
def kv_append(qkv, kc, vc, cos, sin, pos0: int = 0):
    """Prompt qkv [B, T, 3*H*hd]: K rotated at positions pos0 + t, K and V written to cache rows
    pos0 .. pos0 + T - 1 (rows at or past Smax are dropped)."""
    B, H, Smax, hd = kc.shape
    T = qkv.shape[1]
    if hd not in ATTN_HD:
        raise ValueError(f"kv_append: head_dim {hd} not in {ATTN_HD}")
    if qkv.shape != (B, T, 3 * H * hd) or cos.shape[0] < Smax or pos0 < 0:
        raise ValueError("kv_append: shapes do not match the cache")
    if not qkv.is_cuda:
        n = max(0, min(T, Smax - pos0))
        if n:
            _, k, v = qkv.view(B, T, 3, H, hd)[:, :n].unbind(2)
            c, s = cos[pos0:pos0 + n][None, :, None, :], sin[pos0:pos0 + n][None, :, None, :]
            kr = torch.empty_like(k)
            kr[..., 0::2] = k[..., 0::2] * c - k[..., 1::2] * s
            kr[..., 1::2] = k[..., 0::2] * s + k[..., 1::2] * c
            kc[:, :, pos0:pos0 + n] = kr.transpose(1, 2)
            vc[:, :, pos0:pos0 + n] = v.transpose(1, 2)
        return
    qc = qkv.contiguous()
    check(K().ddl_kv_append(ptr(qc), ptr(kc), ptr(vc), ptr(cos), ptr(sin), B, T, H, hd, Smax, int(pos0), stream()),
          "kv_append")


# ------------------------------------------------------------------------------------ sampler
def sample_uniforms(seed: int, step, B: int) -> np.ndarray:
    """u [B] in (0, 1] (fp32): row b's draw at step counter ``step`` (an int, or one per row):
    ``u32_to_unit(philox4x32(counter (step, b, 0, 0), key seed).x)``."""
    st = np.broadcast_to(np.asarray(step, dtype=np.int64), (B,)).astype(np.uint32)
    z = np.zeros(B, dtype=np.uint32)
    r = ref.philox4x32(st, np.arange(B, dtype=np.uint32), z, z, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return ref._unit(r[0])


def kept_mask(x, top_k: int):
    """[V] bool: the top_k largest logits, ties at the threshold kept by lowest index (0: all)."""
    V = x.numel()
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        order = torch.sort(x + 0.0, descending=True, stable=True).indices  # equal values: lowest index first
        keep = torch.zeros(V, dtype=torch.bool)
        keep[order[:top_k]] = True
    return keep


def sample_ref(logits, next_tok, out, lens, finished, step, max_len, temperature, top_k, seed, eos_id, advance):
    B, V = logits.shape
    u = sample_uniforms(seed, step.numpy(), B)
    for b in range(B):
        st = int(step[b])
        if int(finished[b]):
            tok = eos_id
        else:
            x = logits[b]
            tok = int(torch.argmax(x))
            if temperature > 0:
                keep = kept_mask(x, top_k)
                z = x / temperature
                wgt = torch.where(keep, torch.exp(z - z[tok]), torch.zeros_like(z))
                cdf = torch.cumsum(wgt, 0)
                hit = keep & (cdf >= torch.tensor(u[b]) * cdf[-1])
                tok = int(torch.argmax(hit.to(torch.int8))) if bool(hit.any()) else int(keep.nonzero()[-1])
            L = int(lens[b])
            if advance and 0 <= L < max_len:
                lens[b] = L + 1
            if eos_id >= 0 and tok == eos_id:
                finished[b] = 1
        next_tok[b] = tok
        if out is not None and 0 <= st < out.shape[1]:
            out[b, st] = tok
        step[b] = st + 1


def sample(logits, next_tok, out, lens, finished, step, max_len: int, temperature: float = 0.0, top_k: int = 0,
           seed: int = 0, eos_id: int = -1, advance: bool = True):
    """One token per row of logits [B, V] into ``next_tok[b]`` and ``out[b, step[b]]`` (``out``
    may be None). ``temperature == 0``: argmax, lowest index on ties; else softmax of
    logits / temperature over the ``top_k`` largest (0: all), drawn by inverse CDF in vocabulary
    order with ``sample_uniforms(seed, step, B)``. Then the state: ``lens[b] += 1`` (if ``advance``
    — the decode step before this call appended a row — and the sequence is neither frozen nor
    finished), ``finished[b]`` set on ``eos_id`` (-1: none), ``step[b] += 1``."""
    B, V = logits.shape
    eos_id = -1 if eos_id is None else int(eos_id)
    if not (temperature >= 0 and math.isfinite(temperature)) or not 0 <= top_k <= TOP_K_MAX or eos_id >= V:
        raise ValueError(f"sample: temperature {temperature}, top_k {top_k} (0..{TOP_K_MAX}), eos_id {eos_id}")
    for t in (next_tok, lens, finished, step) + (() if out is None else (out,)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("sample: contiguous int32 state tensors only")
    if not logits.is_cuda:
        sample_ref(logits, next_tok, out, lens, finished, step, max_len, temperature, top_k, seed, eos_id, advance)
        return next_tok
    if not logits.is_contiguous() or logits.dtype != torch.float32:
        raise ValueError("sample: contiguous fp32 logits only")
    check(K().ddl_sample_f32(ptr(logits), B, V, float(temperature), int(top_k), int(seed) & (2 ** 64 - 1), eos_id,
                             int(max_len), int(bool(advance)), ptr(next_tok), ptr(out),
                             0 if out is None else out.shape[1], ptr(lens), ptr(finished), ptr(step), stream()),
          "sample_f32")
    return next_tok
