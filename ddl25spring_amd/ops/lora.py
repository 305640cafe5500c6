"""Client-batched LoRA product on a shared frozen linear (csrc/kernels/lora.hip).

Slot s is one client: ``x [S, T, D]`` are its T tokens entering the base linear D -> N, ``y [S, T, N]``
the base linear's output, ``A [S, r, D]`` / ``B [S, N, r]`` its adapter pair. A and B (and dA, dB) may
be views into the rows of ``optim.SlotAdam`` (``data[:, off:off + k].view(S, ...)``): only the slot
stride differs from a contiguous tensor, and the kernels take it as an argument.

  lora_fwd(x, A, B, y, scale)                 -> u = x A^T [S, T, r];  y += scale (u B^T)   in place
  lora_bwd_x(dy, A, B, scale, dx, accumulate) -> v = scale (dy B) [S, T, r];  dx (+)= v A   (dx optional)
  lora_bwd_w(x, dy, u, v, dA, dB, scale)      dA += v^T x,  dB += scale (dy^T u)   (dA None: A frozen)

Device tensors run the HIP kernels (exact-fp32 MFMA, deterministic: the reductions over T go through
per-chunk partials folded in chunk order); CPU tensors the same formulas in torch fp32. Unsupported
shapes raise ``ValueError`` before anything is launched.

``LoRAF32`` is the autograd Function the model uses: applied to the output of ``A.linear`` it adds
the adapter product in place (``LinearF32`` does not save its output) and hands ``dy`` through to the
base linear; the LoRA branch's ``dx`` is a separate tensor that autograd adds to the base DGRAD's.
"""
from __future__ import annotations

import torch

from . import _lib
from . import workspace
from ._lib import check, ptr, stream

vp, i32, i64, f32 = _lib.vp, _lib.i32, _lib.i64, _lib.f32
_lib.register_signatures({
    "ddl_lora_chunk": [],
    "ddl_lora_workspace": [i32, i32, i32, i32],
    "ddl_lora_fwd": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, f32, vp],
    "ddl_lora_bwd_x": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, f32, i32, vp],
    "ddl_lora_bwd_w": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, f32, vp],
})
_lib._RESTYPES["ddl_lora_workspace"] = _lib.ctypes.c_longlong

RANKS = (4, 8, 16)
CHUNK = 64  # tokens per reduction chunk of lora_bwd_w (LORA_CHUNK in lora.hip; checked on first use)
_chunk_checked = [False]


def K():
    lib = _lib.kernels()
    if not _chunk_checked[0]:
        if int(lib.ddl_lora_chunk()) != CHUNK:
            raise RuntimeError(f"lora: kernel chunk {int(lib.ddl_lora_chunk())} != ops.lora.CHUNK {CHUNK}")
        _chunk_checked[0] = True
    return lib


def _dense(name, t, shape):
    if t.dtype != torch.float32:
        raise ValueError(f"lora: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lora: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"lora: {name} must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"lora: {name} must be 16-byte aligned")


def _slot_view(name, t, shape):
    """[S, a, b] with rows packed inside a slot and any slot stride (a SlotAdam row view): -> the
    slot stride in floats."""
    if t.dtype != torch.float32:
        raise ValueError(f"lora: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lora: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    S, a, b = shape
    if t.stride(2) != 1 or t.stride(1) != b:
        raise ValueError(f"lora: {name} must be packed inside a slot (strides {t.stride()})")
    ss = t.stride(0) if S > 1 else a * b
    if ss < a * b or ss % 4 or t.data_ptr() % 16:
        raise ValueError(f"lora: {name} slots must be 16-byte aligned and not overlap (slot stride {ss})")
    return ss


def _check(S, T, D, N, r):
    if r not in RANKS:
        raise ValueError(f"lora: rank {r} not in {RANKS}")
    if D < 16 or N < 16 or D % 16 or N % 16:
        raise ValueError(f"lora: D = {D} and N = {N} must be positive multiples of 16")
    if T < 1 or S < 1 or S > 65535:
        raise ValueError(f"lora: S = {S}, T = {T} must be at least 1 (S at most 65535)")


def _shapes(big, A, B):
    if big.dim() != 3 or A.dim() != 3 or B.dim() != 3:
        raise ValueError("lora: expected [S, T, .] activations, A [S, r, D] and B [S, N, r]")
    S, T = int(big.shape[0]), int(big.shape[1])
    r, D, N = int(A.shape[1]), int(A.shape[2]), int(B.shape[1])
    _check(S, T, D, N, r)
    devs = {big.device, A.device, B.device}
    if len(devs) != 1:
        raise ValueError(f"lora: operands on different devices {devs}")
    return S, T, D, N, r


def lora_fwd(x, A, B, y, scale: float):
    """y += scale ((x A^T) B^T) in place; returns u = x A^T [S, T, r]."""
    S, T, D, N, r = _shapes(x, A, B)
    _dense("x", x, (S, T, D))
    _dense("y", y, (S, T, N))
    a_ss, b_ss = _slot_view("A", A, (S, r, D)), _slot_view("B", B, (S, N, r))
    if not x.is_cuda:
        u = torch.bmm(x, A.transpose(1, 2))
        y.add_(torch.bmm(u, B.transpose(1, 2)), alpha=float(scale))
        return u
    u = torch.empty(S, T, r, dtype=torch.float32, device=x.device)
    lora_fwd_out(x, A, B, y, u, scale, (S, T, D, N, r, a_ss, b_ss))
    return u


def lora_fwd_out(x, A, B, y, u, scale, dims=None):
    """``lora_fwd`` into a caller's ``u`` (device only)."""
    if dims is None:
        S, T, D, N, r = _shapes(x, A, B)
        _dense("x", x, (S, T, D))
        _dense("y", y, (S, T, N))
        dims = (S, T, D, N, r, _slot_view("A", A, (S, r, D)), _slot_view("B", B, (S, N, r)))
    S, T, D, N, r, a_ss, b_ss = dims
    _dense("u", u, (S, T, r))
    check(K().ddl_lora_fwd(ptr(x), ptr(A), ptr(B), ptr(y), ptr(u), S, T, D, N, r, a_ss, b_ss, float(scale),
                           stream()), "lora_fwd")
    return u


def lora_bwd_x(dy, A, B, scale: float, dx=None, accumulate: bool = False, v=None):
    """v = scale (dy B) [S, T, r] (returned); with ``dx`` [S, T, D]: dx = v A, or dx += v A."""
    S, T, D, N, r = _shapes(dy, A, B)
    _dense("dy", dy, (S, T, N))
    if dx is not None:
        _dense("dx", dx, (S, T, D))
    a_ss, b_ss = _slot_view("A", A, (S, r, D)), _slot_view("B", B, (S, N, r))
    if not dy.is_cuda:
        vv = torch.bmm(dy, B).mul_(float(scale))
        if v is not None:
            v.copy_(vv)
            vv = v
        if dx is not None:
            p = torch.bmm(vv, A)
            dx.add_(p) if accumulate else dx.copy_(p)
        return vv
    if v is None:
        v = torch.empty(S, T, r, dtype=torch.float32, device=dy.device)
    _dense("v", v, (S, T, r))
    check(K().ddl_lora_bwd_x(ptr(dy), ptr(A), ptr(B), ptr(v), ptr(dx), S, T, D, N, r, a_ss, b_ss, float(scale),
                             int(bool(accumulate)), stream()), "lora_bwd_x")
    return v


def lora_bwd_w(x, dy, u, v, dA, dB, scale: float):
    """dA += v^T x (skipped when ``dA`` is None: A frozen), dB += scale (dy^T u)."""
    if dy.dim() != 3 or u.dim() != 3 or dB.dim() != 3:
        raise ValueError("lora: expected dy [S, T, N], u [S, T, r] and dB [S, N, r]")
    S, T, N = (int(v_) for v_ in dy.shape)
    r = int(u.shape[2])
    D = int(x.shape[2]) if dA is None else int(dA.shape[2])
    _check(S, T, D, N, r)
    _dense("dy", dy, (S, T, N))
    _dense("u", u, (S, T, r))
    db_ss = _slot_view("dB", dB, (S, N, r))
    da_ss = 0
    if dA is not None:
        _dense("x", x, (S, T, D))
        _dense("v", v, (S, T, r))
        da_ss = _slot_view("dA", dA, (S, r, D))
    if not dy.is_cuda:
        if dA is not None:
            dA.add_(torch.bmm(v.transpose(1, 2), x))
        dB.add_(torch.bmm(dy.transpose(1, 2), u), alpha=float(scale))
        return
    lib = K()
    ws = workspace.scratch_uninit((S * int(lib.ddl_lora_workspace(T, D, N, r)),), dy.device)
    check(lib.ddl_lora_bwd_w(ptr(x) if dA is not None else None, ptr(dy), ptr(u), ptr(v) if dA is not None else None,
                             ptr(dA), ptr(dB), ptr(ws), S, T, D, N, r, da_ss, db_ss, float(scale), stream()),
          "lora_bwd_w")


class LoRAF32(torch.autograd.Function):
    """y_base [S b, ctx, N] (the output of the base linear on x [S b, ctx, D], slot-major) -> the
    same tensor with scale (x A^T) B^T of each slot's adapter added in place. A and B get their
    gradients straight into their ``.grad`` rows when the optimizer fuses them (SlotAdam), else
    through autograd; ``A.requires_grad == False`` skips dA."""

    @staticmethod
    def forward(ctx, y, x, A, B, scale):
        S, r, D = A.shape
        N = B.shape[1]
        x3 = x.reshape(S, -1, D)
        if not x3.is_contiguous():
            x3 = x3.contiguous()
        if not y.is_contiguous():
            raise ValueError("lora: the base linear's output must be contiguous")
        Ad, Bd = A.detach(), B.detach()
        # the result lives in y's memory (no second [T, N] tensor, no copy). It is handed back as a
        # tensor of its own rather than as a dirtied input: LinearF32's output is a view made inside
        # its forward, which autograd refuses to see modified in place. Nothing saved y, and the
        # caller drops it.
        out = y.detach()
        u = lora_fwd(x3, Ad, Bd, out.view(S, -1, N), scale)
        ctx.save_for_backward(x3, u, Ad, Bd)
        ctx.scale, ctx.xshape, ctx.A, ctx.B = float(scale), x.shape, A, B
        return out

    @staticmethod
    def backward(ctx, dy):
        from .autograd_ops import _grad_ready
        x3, u, Ad, Bd = ctx.saved_tensors
        S, T, D = x3.shape
        N = Bd.shape[1]
        d3 = dy.reshape(S, T, N)
        if not d3.is_contiguous():
            d3 = d3.contiguous()
        want_dx, want_a, want_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dx = torch.empty(S, T, D, dtype=torch.float32, device=dy.device) if want_dx else None
        v = lora_bwd_x(d3, Ad, Bd, ctx.scale, dx=dx, accumulate=False)
        dA = dB = None
        if want_b:
            # the row views of SlotAdam.grad are not contiguous tensors, which _grad_sink refuses
            ga = _row_sink(ctx.A) if want_a else None
            gb = _row_sink(ctx.B)
            if want_a and ga is None:
                dA = ga = torch.zeros(Ad.shape, dtype=torch.float32, device=dy.device)
            if gb is None:
                dB = gb = torch.zeros(Bd.shape, dtype=torch.float32, device=dy.device)
            lora_bwd_w(x3, d3, u, v, ga if want_a else None, gb, ctx.scale)
            if want_a and dA is None:
                _grad_ready(ctx.A)
            if dB is None:
                _grad_ready(ctx.B)
        return dy, (dx.view(ctx.xshape) if want_dx else None), dA, dB, None


def _row_sink(p):
    """``p.grad`` when it is a slot-row view the kernels can accumulate into in place."""
    if not getattr(p, "_ddl_fuse_grad", False):
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or g.device != p.device or g.dim() != 3:
        return None
    if g.stride(2) != 1 or g.stride(1) != g.shape[2] or g.stride(0) % 4 or g.data_ptr() % 16:
        return None
    return g


def lora_linear(y, x, A, B, scale: float):
    """The adapter product added to ``y = A.linear(x, W, ...)`` (all devices, differentiable)."""
    return LoRAF32.apply(y, x, A, B, float(scale))
