"""Low-rank adapters (LoRA, Hu et al. 2021) for the fp32 LLaMA, client-batched: one frozen base
model on the device, S slots (clients) each with its own ``A [r, D]``, ``B [N, r]`` on the targeted
linears, trained together as one launch per product (ops/lora.py, csrc/kernels/lora.hip).

    cfg = LoRAConfig(rank=8, alpha=16.0)
    ad = attach_lora(model, slots=8, cfg=cfg, seed=0)   # freezes the base, hands adapters to the blocks
    opt = ad.make_optimizer(lr=1e-3)                    # SlotAdam: row s = client s's whole adapter
    loss = causalLLMLoss(model(tokens), tokens)         # tokens [S * b, ctx], slot-major

The adapter parameters are ``[S, r, D]`` / ``[S, N, r]`` tensors and, once the optimizer exists,
strided views of its ``data [S, P]`` rows: row s is what client s uploads, and ``fl/aggregate.py``
aggregates the rows in place. ``freeze_a`` (FFA-LoRA, Sun et al. 2024) keeps A at its shared seed
initialisation and out of the rows, which makes averaging the rows exact: mean(B_k) A = mean(B_k A).

Generation with several adapters at once, nothing merged (``rows`` is any ``[R, P]`` stack of rows):

    bank = adapter_bank(model, rows)
    model.generate(prompts, adapters=bank, adapter_ids=[0, 2, -1, 1])   # -1: the base model

Only the whole fp32 model in one process is supported; the embedding, the RMSNorm gains and the
LM head stay frozen and unadapted.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass

import torch
import torch.nn as nn

from ..ops import autograd_ops as A_ops
from ..ops import lora as L

TARGETS = ("wqkv", "wo", "w13", "w2")
ROUTES = ("native", "composed")
# the product's route: "native" = the fused kernels of ops/lora.py; "composed" = the same adapters
# from torch.bmm and autograd (benchmarks/bench_fedlora.py times one against the other)
DEFAULT_ROUTE = "native"


@dataclass
class LoRAConfig:
    rank: int = 8
    alpha: float = 16.0
    targets: tuple = TARGETS
    freeze_a: bool = False

    @property
    def scale(self) -> float:
        return float(self.alpha) / float(self.rank)


class BlockLoRA:
    """What a ``Block`` holds: its targets' (A, B) pairs. ``active`` is False while the adapter is
    merged into the base weights (the block then takes the plain path)."""

    def __init__(self, pairs: dict, scale: float, slots: int, owner: "LoRAAdapters"):
        self.pairs, self.scale, self.slots, self.owner = pairs, scale, slots, owner

    @property
    def active(self) -> bool:
        return not self.owner.merged

    def add(self, name, y, x):
        """y = linear(x, W[name], ...) -> y with slot s's scale (x A_s^T) B_s^T added."""
        pair = self.pairs.get(name)
        if pair is None:
            return y
        A, B = pair
        S = self.slots
        if x.shape[0] % S:
            raise ValueError(f"lora: a batch of {x.shape[0]} sequences is not slot-major over {S} slots")
        if x.dtype != torch.float32:
            raise NotImplementedError("lora: fp32 activations only")
        if self.owner.route == "composed":
            x3 = x.reshape(S, -1, x.shape[-1])
            d = torch.bmm(torch.bmm(x3, A.transpose(1, 2)), B.transpose(1, 2))
            return y + (self.scale * d).view(y.shape)
        return L.lora_linear(y, x, A, B, self.scale)


class LoRAAdapters:
    """Every adapter parameter of a model, by name (``"<block>.<target>.A"`` / ``".B"``)."""

    def __init__(self, model, slots: int, cfg: LoRAConfig):
        self.model, self.slots, self.cfg = model, slots, cfg
        self.named: "OrderedDict[str, nn.Parameter]" = OrderedDict()
        self.opt = None
        self.route = DEFAULT_ROUTE
        self._saved = None  # base weights while merged

    @property
    def merged(self) -> bool:
        return self._saved is not None

    def parameters(self):
        return list(self.named.values())

    def trainable(self):
        """(name, parameter) of the parameters in the optimizer's rows, in row order."""
        return [(n, p) for n, p in self.named.items() if p.requires_grad]

    def make_optimizer(self, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        from ..optim import SlotAdam
        if self.opt is not None:
            raise RuntimeError("lora: the adapters already have an optimizer")
        self.opt = SlotAdam([p for _, p in self.trainable()], self.slots, lr=lr, betas=betas, eps=eps)
        return self.opt

    @property
    def P(self) -> int:
        return self._opt().P

    def _opt(self):
        if self.opt is None:
            raise RuntimeError("lora: call make_optimizer() first (the rows are its buffer)")
        return self.opt

    def row_views(self, row):
        """The trainable parameters of one row [P] as views of it, by name."""
        opt = self._opt()
        out = OrderedDict()
        for (n, p), off in zip(self.trainable(), opt.offsets):
            out[n] = row[off:off + p[0].numel()].view(p.shape[1:])
        return out

    def pair(self, row, block: int, target: str):
        """(A [r, D], B [N, r]) of one row; a frozen A is the shared one."""
        if row is None:
            return self.named[f"{block}.{target}.A"].detach()[0], self.named[f"{block}.{target}.B"].detach()[0]
        views = self.row_views(row)
        a = views.get(f"{block}.{target}.A")
        if a is None:
            a = self.named[f"{block}.{target}.A"].detach()[0]
        return a, views[f"{block}.{target}.B"]

    @torch.no_grad()
    def broadcast(self, row, rows: int | None = None):
        """The global row into the first ``rows`` slots."""
        opt = self._opt()
        opt.data[:opt.S if rows is None else rows].copy_(row.unsqueeze(0))


def _check_model(model):
    from .llama import LLama
    if not isinstance(model, LLama):
        raise NotImplementedError("lora: only a whole LLama in one process is supported (no pipeline stages)")
    if model.precision != "fp32":
        raise NotImplementedError(f"lora: the adapters run the fp32 kernels only (precision={model.precision!r})")
    if any(getattr(m, "tp", None) is not None for m in (model.first, model.last, *model.blocks())):
        raise NotImplementedError("lora: a tensor-parallel (sharded) model is not supported")


def attach_lora(model, slots: int, cfg: LoRAConfig | None = None, seed: int = 0) -> LoRAAdapters:
    """Freeze every base parameter and give each block's targeted linears S adapter pairs:
    A ~ N(0, 1 / D) from ``seed`` (the same in every slot), B = 0, so the model computes exactly
    what the base does until B moves. -> the ``LoRAAdapters`` (also ``model.lora``)."""
    cfg = cfg or LoRAConfig()
    _check_model(model)
    if getattr(model, "lora", None) is not None:
        raise RuntimeError("lora: the model already has adapters")
    if cfg.rank not in L.RANKS:
        raise ValueError(f"lora: rank {cfg.rank} not in {L.RANKS}")
    if slots < 1:
        raise ValueError("lora: at least one slot")
    bad = [t for t in cfg.targets if t not in TARGETS]
    if bad or not cfg.targets:
        raise ValueError(f"lora: targets {tuple(cfg.targets)} must be a non-empty subset of {TARGETS}")
    for p in model.parameters():
        p.requires_grad_(False)
    ad = LoRAAdapters(model, slots, cfg)
    gen = torch.Generator().manual_seed(int(seed))
    for i, blk in enumerate(model.blocks()):
        pairs = {}
        for t in cfg.targets:
            w = getattr(blk, t)
            N, D = w.shape
            if D % 16 or N % 16:
                raise ValueError(f"lora: {t} of shape {N} x {D} is not a multiple of 16 in both extents")
            a0 = torch.randn(cfg.rank, D, generator=gen) * (1.0 / math.sqrt(D))
            Ap = nn.Parameter(a0.unsqueeze(0).repeat(slots, 1, 1).to(w.device), requires_grad=not cfg.freeze_a)
            Bp = nn.Parameter(torch.zeros(slots, N, cfg.rank, device=w.device))
            ad.named[f"{i}.{t}.A"], ad.named[f"{i}.{t}.B"] = Ap, Bp
            pairs[t] = (Ap, Bp)
        blk.lora = BlockLoRA(pairs, cfg.scale, slots, ad)
    model.lora = ad
    return ad


def detach_lora(model) -> None:
    """Take the adapters off again (the base stays frozen)."""
    if getattr(model, "lora", None) is not None and model.lora.merged:
        unmerge_lora(model)
    for blk in model.blocks():
        blk.lora = None
    model.lora = None


def _adapters(model) -> LoRAAdapters:
    ad = getattr(model, "lora", None)
    if ad is None:
        raise RuntimeError("lora: the model has no adapters (attach_lora)")
    return ad


class AdapterBank:
    """R adapters for generation (``LLama.generate(adapters=bank, adapter_ids=...)``): per
    (block, target) the strided views ``A [R, r, D]`` and ``B [R, N, r]`` into ``rows [R, P]``. The
    views alias ``rows``: writing a row in place changes what the next step computes."""

    def __init__(self, owner: LoRAAdapters, rows, pairs: dict):
        self.owner, self.rows, self.pairs = owner, rows, pairs
        self.R, self.rank, self.scale = int(rows.shape[0]), owner.cfg.rank, owner.cfg.scale
        self.targets = tuple(owner.cfg.targets)

    def pair(self, block: int, target: str):
        """(A, B) of one targeted linear, or None where the target has no adapter."""
        return self.pairs.get((block, target))

    @property
    def key(self):
        """What a captured decode step depends on beside the ids (which it reads on the device)."""
        return (self.rows.data_ptr(), self.R, int(self.rows.stride(0)), self.rank, self.targets)

    def check(self, model, device):
        if self.owner is not getattr(model, "lora", None):
            raise ValueError("lora: the adapter bank belongs to another model")
        if self.owner.merged:
            raise RuntimeError("lora: an adapter is merged into the base weights (unmerge_lora first)")
        if self.rows.device != device:
            raise ValueError(f"lora: the adapter bank is on {self.rows.device}, the model on {device}")


@torch.no_grad()
def adapter_bank(model, rows) -> AdapterBank:
    """Any stack ``rows [R, P]`` of ``SlotAdam`` rows (``opt.data``, ``global_row[None]``, a
    ``torch.cat`` of them) on the model's device as per-sequence adapters of ``LLama.generate``. A
    frozen A (FFA-LoRA) is the model's one shared copy, with slot stride 0."""
    ad = _adapters(model)
    if ad.merged:
        raise RuntimeError("lora: an adapter is merged into the base weights (unmerge_lora first)")
    opt = ad._opt()
    dev = ad.parameters()[0].device
    if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[0] < 1 or rows.shape[1] != opt.P:
        raise ValueError(f"lora: adapter rows must be [R, {opt.P}]")
    if rows.dtype != torch.float32 or rows.device != dev:
        raise ValueError(f"lora: adapter rows must be float32 on {dev}")
    if rows.stride(1) != 1 or rows.stride(0) % 4 or rows.data_ptr() % 16 or \
            (rows.shape[0] > 1 and rows.stride(0) < opt.P):
        raise ValueError(f"lora: adapter rows must be packed, 16-byte aligned rows (strides {rows.stride()})")
    R = rows.shape[0]
    views = {n: rows[:, off:off + p[0].numel()].view(R, *p.shape[1:])
             for (n, p), off in zip(ad.trainable(), opt.offsets)}
    pairs = {}
    for i in range(len(model.blocks())):
        for t in ad.cfg.targets:
            a = views.get(f"{i}.{t}.A")
            if a is None:
                a0 = ad.named[f"{i}.{t}.A"].detach()[0]
                a = a0.unsqueeze(0).expand(R, *a0.shape)
            pairs[(i, t)] = (a, views[f"{i}.{t}.B"])
    return AdapterBank(ad, rows, pairs)


@torch.no_grad()
def merged_weight(w, a, b, scale: float):
    """W + scale B A with the product on the project's linear op (off the hot path)."""
    delta = A_ops.linear(b.contiguous(), a.t().contiguous())  # [N, r] x [D, r]^T
    return w + scale * delta.to(w.dtype)


@torch.no_grad()
def merge_lora(model, row=None) -> None:
    """Add ``scale B A`` of one adapter row [P] (default: slot 0's) into the targeted weights, so
    that ``model.generate`` and plain forwards run the fine-tuned model. The base bits are kept and
    ``unmerge_lora`` copies them back."""
    ad = _adapters(model)
    if ad.merged:
        raise RuntimeError("lora: already merged (unmerge_lora first)")
    saved = {}
    for i, blk in enumerate(model.blocks()):
        for t in ad.cfg.targets:
            w = getattr(blk, t)
            a, b = ad.pair(row, i, t)
            saved[(i, t)] = w.detach().clone()
            w.data.copy_(merged_weight(w.detach(), a, b, ad.cfg.scale))
    ad._saved = saved


@torch.no_grad()
def unmerge_lora(model) -> None:
    """Restore the saved base bits (a copy, not a subtraction)."""
    ad = _adapters(model)
    if not ad.merged:
        raise RuntimeError("lora: nothing is merged")
    blocks = model.blocks()
    for (i, t), w0 in ad._saved.items():
        getattr(blocks[i], t).data.copy_(w0)
    ad._saved = None


@torch.no_grad()
def lora_state_dict(model, row=None) -> dict:
    """One adapter row (default: slot 0's) by parameter name, frozen A included, on the CPU."""
    ad = _adapters(model)
    views = ad.row_views(row) if row is not None else {}
    out = OrderedDict()
    for n, p in ad.named.items():
        out[n] = (views[n] if n in views else p.detach()[0]).detach().cpu().clone()
    return out


@torch.no_grad()
def load_lora_state_dict(model, sd: dict, row=None) -> None:
    """Write a ``lora_state_dict`` into ``row`` [P] (default: every slot). Names and shapes must
    match; a frozen A must equal the model's own (it is not part of a row)."""
    ad = _adapters(model)
    if set(sd) != set(ad.named):
        missing, extra = sorted(set(ad.named) - set(sd)), sorted(set(sd) - set(ad.named))
        raise KeyError(f"lora state dict: missing {missing[:3]}, unexpected {extra[:3]}")
    for n, p in ad.named.items():
        if tuple(sd[n].shape) != tuple(p.shape[1:]):
            raise ValueError(f"lora state dict: {n} has shape {tuple(sd[n].shape)}, expected {tuple(p.shape[1:])}")
    views = ad.row_views(row) if row is not None else None
    for n, p in ad.named.items():
        t = sd[n].to(p.device, torch.float32)
        if not p.requires_grad:
            if row is None:
                p.data.copy_(t.unsqueeze(0).expand_as(p))
            elif not torch.equal(p.detach()[0], t):
                raise ValueError(f"lora state dict: frozen {n} differs from the model's")
        elif row is None:
            p.data.copy_(t.unsqueeze(0).expand_as(p))
        else:
            views[n].copy_(t)
