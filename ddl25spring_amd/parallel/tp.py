"""Tensor (intra-layer) parallelism of the fp32 LLaMA, Megatron style (Shoeybi et al. 2019).

A block's two GEMM pairs are cut so that each needs one all-reduce per pass: ``wqkv`` and ``w13``
by output rows (column-parallel: every rank keeps ``H / tp`` heads and ``F / tp`` SwiGLU columns),
``wo`` and ``w2`` by input columns (row-parallel: each rank's product is a partial sum). The LM
head is cut over the vocabulary and the loss is ``ops.cross_entropy_vocab_parallel``, so no rank
ever holds a full logit row. RMSNorm gains and the embedding stay replicated; their gradients are
identical on every rank of a group because ``copy_to_tp``'s backward all-reduce hands every rank
the same bits.

  copy_to_tp      identity forward, all-reduce of the gradient backward  (before a column-parallel linear)
  reduce_from_tp  all-reduce forward, identity backward                  (after a row-parallel linear)
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class TPHandle:
    """What a sharded module needs to talk to its tensor-parallel peers."""
    ctx: object            # runtime.dist.DistContext
    group: object          # the tp process group (None: the context's whole world)
    degree: int
    rank: int              # this rank's index t within the group

    def copy(self, x):
        return copy_to_tp(x, self.ctx, self.group)

    def reduce(self, x):
        return reduce_from_tp(x, self.ctx, self.group)


class _CopyToTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dctx, group):
        ctx.dctx, ctx.group = dctx, group
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        g = dy.contiguous().clone()
        ctx.dctx.all_reduce(g, group=ctx.group)
        return g, None, None


class _ReduceFromTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dctx, group):
        y = x.detach().contiguous().clone()
        dctx.all_reduce(y, group=group)
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None


def copy_to_tp(x, ctx, group=None):
    """x on every rank; in the backward the ranks' gradients of x are summed."""
    return _CopyToTP.apply(x, ctx, group)


def reduce_from_tp(x, ctx, group=None):
    """The sum over the group of every rank's partial x; the gradient passes through."""
    return _ReduceFromTP.apply(x, ctx, group)


def vocab_range(V: int, tp: int, t: int) -> tuple[int, int]:
    """Vocabulary rows [v0, v1) of rank t: shards of ceil(V / tp / 16) * 16 rows (whole 64-byte
    lines of a logit row), the last one shorter. Raises if a shard would be empty."""
    if tp < 1 or not 0 <= t < tp:
        raise ValueError(f"vocab_range: rank {t} outside a tensor-parallel group of {tp}")
    vs = -(-V // (tp * 16)) * 16
    if (tp - 1) * vs >= V:
        raise ValueError(f"vocabulary {V} over tp={tp}: shards of {vs} rows leave rank {tp - 1} without any")
    return t * vs, min(V, (t + 1) * vs)


def _kind(name: str) -> str:
    leaf = name.rsplit(".", 1)[-1]
    return leaf if leaf in ("wqkv", "wo", "w13", "w2", "head") else "replicated"


def _blocks(module):
    from ..models.llama import Block
    return [m for m in module.modules() if isinstance(m, Block)]


def check_shardable(num_heads: int, ffn_hidden: int, vocab_size: int | None, tp: int) -> None:
    """ValueError unless heads and FFN columns divide by tp and no vocabulary shard is empty."""
    if tp < 1:
        raise ValueError(f"tp must be >= 1, got {tp}")
    if num_heads % tp:
        raise ValueError(f"tensor parallelism: num_heads {num_heads} is not a multiple of tp={tp}")
    if ffn_hidden % tp:
        raise ValueError(f"tensor parallelism: FFN hidden size {ffn_hidden} is not a multiple of tp={tp}")
    if vocab_size is not None:
        vocab_range(vocab_size, tp, tp - 1)


def shard_slices(kind: str, shape, tp: int, t: int):
    """(dim, [index ranges]) of rank t's part of a full parameter of this kind, None if replicated."""
    if kind == "wqkv":
        d = shape[0] // 3
        return 0, [(p * d + t * d // tp, p * d + (t + 1) * d // tp) for p in range(3)]
    if kind == "w13":
        f = shape[0] // 2
        return 0, [(p * f + t * f // tp, p * f + (t + 1) * f // tp) for p in range(2)]
    if kind in ("wo", "w2"):
        n = shape[1]
        return 1, [(t * n // tp, (t + 1) * n // tp)]
    if kind == "head":
        return 0, [vocab_range(shape[0], tp, t)]
    return None


def _cut(full: torch.Tensor, kind: str, tp: int, t: int) -> torch.Tensor:
    sl = shard_slices(kind, full.shape, tp, t)
    if sl is None:
        return full
    dim, ranges = sl
    return torch.cat([full.narrow(dim, a, b - a) for a, b in ranges], dim=dim).contiguous()


def shard_llama(model, tp: int, t: int, handle: TPHandle | None = None):
    """Turn a full (seeded) LLama, or one of its stages, into rank t's shard IN PLACE: the sharded
    parameters are replaced by their slices, every block keeps ``num_heads / tp`` heads, and the
    blocks / last stage get ``handle`` (their collectives). Returns the model."""
    blocks = _blocks(model)
    if not 0 <= t < tp:
        raise ValueError(f"shard_llama: rank {t} outside a tensor-parallel group of {tp}")
    head = model_head(model)
    for blk in blocks[:1]:
        check_shardable(blk.h, blk.w2.shape[1], None if head is None else head.shape[0], tp)
    with torch.no_grad():
        for blk in blocks:
            for name in ("wqkv", "wo", "w13", "w2"):
                setattr(blk, name, torch.nn.Parameter(_cut(getattr(blk, name).data, name, tp, t)))
            blk.h //= tp
            blk.tp = handle
        for m in model.modules():
            if isinstance(getattr(m, "head", None), torch.nn.Parameter):
                m.head = torch.nn.Parameter(_cut(m.head.data, "head", tp, t))
                m.tp = handle
    return model


def model_head(model):
    for m in model.modules():
        if isinstance(getattr(m, "head", None), torch.nn.Parameter):
            return m.head
    return None


def gather_llama(shards: list[dict], full_shapes: dict | None = None) -> dict:
    """Inverse of ``shard_llama`` on named tensors: ``shards[t]`` maps parameter names to rank t's
    tensors (weights, or their gradients); returns the full tensors. Replicated entries are taken
    from rank 0."""
    tp = len(shards)
    out = {}
    for name, first in shards[0].items():
        kind = _kind(name)
        parts = [s[name] for s in shards]
        if kind == "replicated":
            out[name] = first.clone()
        elif kind in ("wo", "w2"):
            out[name] = torch.cat(parts, dim=1)
        elif kind == "head":
            out[name] = torch.cat(parts, dim=0)
        else:  # wqkv / w13: each of the 3 / 2 row blocks is cut separately
            nb = 3 if kind == "wqkv" else 2
            per = first.shape[0] // nb
            out[name] = torch.cat([p[b * per:(b + 1) * per] for b in range(nb) for p in parts], dim=0)
        if full_shapes is not None and tuple(out[name].shape) != tuple(full_shapes[name]):
            raise ValueError(f"gather_llama: {name} reassembles to {tuple(out[name].shape)}, "
                             f"expected {tuple(full_shapes[name])} (tp={tp})")
    return out
