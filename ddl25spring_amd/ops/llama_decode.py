"""Ops of the fp32 LLaMA's generation path (csrc/kernels/llama_decode.hip): a skinny-row linear with
fused prologues, single-query attention over a KV cache with the step's row appended in the same
launch, the prefill's cache append, and a sampler that also carries the step's state. Per-sequence
LoRA adapters (row t of the batch runs adapter ``ids[t]``): the shrink ``lora_rows_u`` and the expand
fused into ``lin_rows(lora=...)``.

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

vp, i32, i64, f32, u64 = _lib.vp, _lib.i32, _lib.i64, _lib.f32, _lib.u64
_lib.register_signatures({
    "ddl_lin_rows_f32": [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "ddl_lin_rows_lora_f32": [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, i32, i64, i32, f32, vp],
    "ddl_lora_rows_u": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, i32, f32, vp],
    "ddl_attnf_decode": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp],
    "ddl_kv_append": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "ddl_sample_f32": [vp, i32, i32, f32, i32, u64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp],
})

LIN_ROWS_MAX_T = 16
LORA_RANKS = (4, 8, 16)  # ranks of the per-sequence adapters (ops/lora.py: RANKS)
TOP_K_MAX = 1024
PROLOGUES = {"none": 0, "rmsnorm": 1, "swiglu": 2}
ATTN_REC_EXTRA = 2  # floats of a split record beside its HD accumulators: max, sum


def K():
    return _lib.kernels()


# --------------------------------------------------------------------------------- lin_rows
def _slot_stride(t) -> int:
    """Slot stride in floats of an adapter view [R, a, b] (0: one shared slot)."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1] * t.shape[2])


def lin_rows_launch(x, w, out, residual=None, pro="none", gain=None, eps=1e-6, T=None, C=None, lora=None,
                    rank=None) -> int:
    """The raw launcher's return code (0, or hipErrorInvalidValue without a launch)."""
    Kout = w.shape[0]
    T = x.shape[0] if T is None else T
    C = w.shape[1] if C is None else C
    if lora is not None:
        u, B, ids, scale = lora
        return int(K().ddl_lin_rows_lora_f32(ptr(x), ptr(w), ptr(residual), ptr(gain), ptr(out), T, C, Kout,
                                             PROLOGUES[pro], float(eps), ptr(u), ptr(B), ptr(ids), B.shape[0],
                                             _slot_stride(B), B.shape[2] if rank is None else rank, float(scale),
                                             stream()))
    return int(K().ddl_lin_rows_f32(ptr(x), ptr(w), ptr(residual), ptr(gain), ptr(out), T, C, Kout,
                                    PROLOGUES[pro], float(eps), stream()))


def _prologue_ref(x, pro, gain, eps):
    if pro == "rmsnorm":
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gain
    elif pro == "swiglu":
        a, b = x.chunk(2, -1)
        x = torch.nn.functional.silu(a) * b
    return x


def _valid_ids(ids, R):
    """(bool [T]: the row has an adapter, int64 [T]: its slot, 0 where it has none)."""
    ok = (ids >= 0) & (ids < R)
    return ok, torch.where(ok, ids, torch.zeros_like(ids)).long()


def lin_rows_ref(x, w, residual=None, pro="none", gain=None, eps=1e-6, lora=None):
    y = _prologue_ref(x, pro, gain, eps) @ w.t()
    if lora is not None:
        u, B, ids, scale = lora
        ok, slot = _valid_ids(ids, B.shape[0])
        d = torch.einsum("tj,tkj->tk", u, B[slot])
        y = torch.where(ok[:, None], y + float(scale) * d, y)
    return y if residual is None else y + residual


def _check_ids(name, ids, T):
    if ids.dtype != torch.int32 or tuple(ids.shape) != (T,) or not ids.is_contiguous():
        raise ValueError(f"{name}: ids must be a contiguous int32 [{T}] tensor")


def _check_slots(name, what, t, shape, shared_ok):
    """An adapter view [R, a, b]: fp32, packed inside a slot, slots 16-byte aligned (stride 0 = one
    shared slot where ``shared_ok``)."""
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} must be float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    R, a, b = shape
    if t.stride(2) != 1 or t.stride(1) != b:
        raise ValueError(f"{name}: {what} must be packed inside a slot (strides {t.stride()})")
    ss = _slot_stride(t)
    if ss % 4 or t.data_ptr() % 16 or not (ss >= a * b or (shared_ok and ss == 0)):
        raise ValueError(f"{name}: {what} slots must be 16-byte aligned and not overlap (slot stride {ss})")


def _check_lora(name, T, Kout, lora, like):
    u, B, ids, _ = lora
    if not 1 <= T <= LIN_ROWS_MAX_T:
        raise ValueError(f"{name}: {T} rows (1 <= T <= {LIN_ROWS_MAX_T})")
    if B.dim() != 3 or B.shape[2] not in LORA_RANKS:
        raise ValueError(f"{name}: B must be [R, K, r] with r in {LORA_RANKS}")
    r = B.shape[2]
    _check_slots(name, "B", B, (B.shape[0], Kout, r), False)
    _check_ids(name, ids, T)
    if u.dtype != torch.float32 or tuple(u.shape) != (T, r) or not u.is_contiguous() or u.data_ptr() % 16:
        raise ValueError(f"{name}: u must be a contiguous 16-byte aligned fp32 [{T}, {r}] tensor")
    if len({like.device, u.device, B.device, ids.device}) != 1:
        raise ValueError(f"{name}: operands on different devices")


def lin_rows(x, w, out, residual=None, pro="none", gain=None, eps=1e-6, lora=None):
    """out[T, K] = pro(x)[T, C] @ w[K, C]^T (+ residual[T, K]), 1 <= T <= 16, C % 4 == 0.
    ``pro``: "none"; "rmsnorm" (``gain`` [C], ``eps``); "swiglu" (x is [T, 2C] = [a | b]).
    ``lora = (u, B, ids, scale)``: row t also gets ``scale * u[t] @ B[ids[t]]^T`` before the residual
    (u [T, r] from ``lora_rows_u``, B [R, K, r] with any slot stride, ids int32 [T]); a row whose id
    is outside ``[0, R)`` is the plain row, bit for bit."""
    if pro not in PROLOGUES:
        raise ValueError(f"lin_rows: prologue {pro!r} not in {tuple(PROLOGUES)}")
    if lora is not None:
        _check_lora("lin_rows", x.shape[0], w.shape[0], lora, x)
    if not x.is_cuda:
        out.copy_(lin_rows_ref(x, w, residual, pro, gain, eps, lora))
        return out
    T, Cx = x.shape
    Kout, C = w.shape
    if Cx != (2 * C if pro == "swiglu" else C) or out.shape != (T, Kout):
        raise ValueError(f"lin_rows: x {tuple(x.shape)}, w {tuple(w.shape)}, out {tuple(out.shape)} ({pro})")
    for t in (x, w, out, residual, gain):
        if t is not None and not (t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError("lin_rows: contiguous fp32 tensors only")
    check(lin_rows_launch(x, w, out, residual, pro, gain, eps, lora=lora), "lin_rows_f32")
    return out


# ----------------------------------------------------------------- per-sequence adapters: shrink
def lora_rows_u_launch(x, A, ids, u, pro="none", gain=None, eps=1e-6, T=None, rank=None) -> int:
    """The raw launcher's return code (0, or hipErrorInvalidValue without a launch)."""
    R, r, C = A.shape
    return int(K().ddl_lora_rows_u(ptr(x), ptr(A), ptr(ids), ptr(gain), ptr(u), x.shape[0] if T is None else T, C, R,
                                   r if rank is None else rank, _slot_stride(A) if A.stride(0) else 0,
                                   PROLOGUES[pro], float(eps), stream()))


def lora_rows_u_ref(x, A, ids, pro="none", gain=None, eps=1e-6):
    ok, slot = _valid_ids(ids, A.shape[0])
    u = torch.einsum("tc,tjc->tj", _prologue_ref(x, pro, gain, eps), A[slot])
    return torch.where(ok[:, None], u, torch.zeros_like(u))


def lora_rows_u(x, A, ids, u, pro="none", gain=None, eps=1e-6):
    """u[T, r] = pro(x)[T, C] @ A[ids[t]]^T: the adapters' shrink on the rows ``lin_rows`` stages
    (the same prologues, the same staged bits). A [R, r, C] with any slot stride (a view into
    optimizer rows; stride 0 = one shared A), ids int32 [T]; an id outside ``[0, R)`` means no
    adapter and gives a zero row. r in (4, 8, 16), 1 <= T <= 16, C % 4 == 0."""
    if pro not in PROLOGUES:
        raise ValueError(f"lora_rows_u: prologue {pro!r} not in {tuple(PROLOGUES)}")
    if A.dim() != 3 or A.shape[1] not in LORA_RANKS or x.dim() != 2:
        raise ValueError(f"lora_rows_u: A must be [R, r, C] with r in {LORA_RANKS}, x [T, C]")
    R, r, C = A.shape
    T, Cx = x.shape
    if not 1 <= T <= LIN_ROWS_MAX_T or C < 4 or C % 4 or Cx != (2 * C if pro == "swiglu" else C):
        raise ValueError(f"lora_rows_u: x {tuple(x.shape)}, A {tuple(A.shape)} ({pro}); 1 <= T <= {LIN_ROWS_MAX_T}")
    _check_slots("lora_rows_u", "A", A, (R, r, C), True)
    _check_ids("lora_rows_u", ids, T)
    if u.dtype != torch.float32 or tuple(u.shape) != (T, r) or not u.is_contiguous() or u.data_ptr() % 16:
        raise ValueError(f"lora_rows_u: u must be a contiguous 16-byte aligned fp32 [{T}, {r}] tensor")
    for t in (x, gain):
        if t is not None and not (t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0):
            raise ValueError("lora_rows_u: contiguous 16-byte aligned fp32 tensors only")
    if pro == "rmsnorm" and (gain is None or gain.numel() != C):
        raise ValueError("lora_rows_u: the rmsnorm prologue needs gain [C]")
    if len({x.device, A.device, ids.device, u.device}) != 1:
        raise ValueError("lora_rows_u: operands on different devices")
    if not x.is_cuda:
        u.copy_(lora_rows_u_ref(x, A, ids, pro, gain, eps))
        return u
    check(lora_rows_u_launch(x, A, ids, u, pro, gain, eps), "lora_rows_u")
    return u


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
