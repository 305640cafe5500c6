"""Tiny LLaMA for the data/pipeline-parallel tutorials, with the reference's stage API.

The reference imports these from the external ``simplellm`` package (not vendored, not
installable here): ``LLama(CausalLLama, vocab, dmodel, num_heads, device, n_layers,
ctx_size, padding_idx)``, ``LLamaFirstStage(...).embed(x)``, ``LLamaStage``, ``LLamaLastStage``,
``causalLLMLoss`` (call sites lab/tutorial_1b/primer/intro.py:17-18,
PP/1F1B/intro_PP_1F1B.py:29-39,53,78-79). simplellm's internals are unverified, so the
architecture is the standard pre-norm LLaMA block: RMSNorm -> fused QKV -> causal attention with
interleaved RoPE -> out-proj (+residual, fused in the GEMM epilogue) -> RMSNorm -> fused [w1|w3]
SwiGLU FFN (hidden = 8/3 d rounded to 32) -> w2 (+residual) ; final RMSNorm and an untied LM head.
Loss-curve comparisons with the reference are therefore trend-level.

Precision (extension): ``precision="fp32"`` (default: the reference trains this model in fp32,
lab/tutorial_1b/PP/1F1B/intro_PP_1F1B_MB.py:16-46) makes the embedding emit fp32 activations, so
every op downstream runs the reference-precision kernels (ops/llama_f32.py: linears on the X6 /
exact-fp32 conv engine, fp32 attention / RMSNorm / SwiGLU / CE, all deterministic);
``precision="bf16"`` is the bf16-MFMA fast path. On CPU everything is fp32 either way.

Stage 0's ``embed`` runs the embedding AND the stage's blocks (the reference's rank 0 only calls
``embed``, so whether its blocks ran was simplellm-dependent).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..ops import autograd_ops as A


def _ffn_hidden(d: int) -> int:
    return int(math.ceil(8 * d / 3 / 32) * 32)


class Block(nn.Module):
    def __init__(self, dmodel: int, num_heads: int, ffn_hidden: int | None = None, tp=None):
        super().__init__()
        assert dmodel % num_heads == 0
        self.h, self.hd = num_heads, dmodel // num_heads
        # tensor-parallel handle (parallel/tp.py: ctx, group, degree); the weights are built whole
        # from the seed and cut by ``shard_llama``, which also sets the local head count
        self.tp = tp
        F = ffn_hidden or _ffn_hidden(dmodel)
        self.norm1 = nn.Parameter(torch.ones(dmodel))
        self.norm2 = nn.Parameter(torch.ones(dmodel))
        self.wqkv = nn.Parameter(torch.empty(3 * dmodel, dmodel))
        self.wo = nn.Parameter(torch.empty(dmodel, dmodel))
        self.w13 = nn.Parameter(torch.empty(2 * F, dmodel))
        self.w2 = nn.Parameter(torch.empty(dmodel, F))
        for w in (self.wqkv, self.wo, self.w13, self.w2):
            nn.init.normal_(w, std=0.02)
        with torch.no_grad():
            self.wo.mul_(1 / math.sqrt(2))
            self.w2.mul_(1 / math.sqrt(2))

    # low-rank adapters of the targeted linears (models/lora.py: attach_lora); None = the plain block
    lora = None

    def forward(self, x):  # x [B, S, D]
        if self.tp is not None:
            return self.forward_tp(x)
        if self.lora is not None and self.lora.active:
            return self.forward_lora(x)
        h, x = A.rmsnorm_fork(x, self.norm1)
        qkv = A.linear(h, self.wqkv)
        att = A.causal_attention(qkv, self.h, self.hd)
        x = A.linear(att, self.wo, residual=x)
        h, x = A.rmsnorm_fork(x, self.norm2)
        return A.linear(A.swiglu(A.linear(h, self.w13)), self.w2, residual=x)

    def forward_lora(self, x):
        """The block on a frozen base with per-slot adapters: x [S b, ctx, D] is slot-major, and each
        targeted linear's output gets scale (x A_s^T) B_s^T of its slot added in place."""
        lo = self.lora
        h, x = A.rmsnorm_fork(x, self.norm1)
        qkv = lo.add("wqkv", A.linear(h, self.wqkv), h)
        att = A.causal_attention(qkv, self.h, self.hd)
        x = lo.add("wo", A.linear(att, self.wo, residual=x), att)
        h, x = A.rmsnorm_fork(x, self.norm2)
        g = A.swiglu(lo.add("w13", A.linear(h, self.w13), h))
        return lo.add("w2", A.linear(g, self.w2, residual=x), g)

    def forward_tp(self, x):
        """The sharded block: wqkv / w13 hold this rank's heads / SwiGLU columns (column-parallel,
        the normed input's gradient summed over the group), wo / w2 the matching input columns
        (row-parallel: partial products summed over the group, then the residual added once)."""
        tp = self.tp
        h, x = A.rmsnorm_fork(x, self.norm1)
        att = A.causal_attention(A.linear(tp.copy(h), self.wqkv), self.h, self.hd)
        x = A.residual_add(x, tp.reduce(A.linear(att, self.wo)))
        h, x = A.rmsnorm_fork(x, self.norm2)
        return A.residual_add(x, tp.reduce(A.linear(A.swiglu(A.linear(tp.copy(h), self.w13)), self.w2)))


class CausalLLama:
    """Marker type, as passed to ``LLama(CausalLLama, ...)`` in the reference."""


PRECISIONS = ("fp32", "bf16")


def _act_dtype(precision: str):
    if precision not in PRECISIONS:
        raise ValueError(f"LLaMA precision must be one of {PRECISIONS}, got {precision!r}")
    return torch.float32 if precision == "fp32" else torch.bfloat16


class _Base(nn.Module):
    def __init__(self, dmodel, num_heads, n_layers, ctx_size, device=None, ffn_hidden=None, precision="fp32",
                 tp=None):
        super().__init__()
        self.dmodel, self.ctx_size = dmodel, ctx_size
        self.precision = precision
        self.act_dtype = _act_dtype(precision)
        self.tp = tp
        self.layers = nn.ModuleList(Block(dmodel, num_heads, ffn_hidden, tp) for _ in range(n_layers))
        if device is not None:
            self.to(device)

    def run_layers(self, x):
        for blk in self.layers:
            x = blk(x)
        return x


class LLamaFirstStage(_Base):
    def __init__(self, vocab_size, dmodel=288, num_heads=6, device=None, n_layers=2, ctx_size=256,
                 padding_idx=None, ffn_hidden=None, precision="fp32", tp=None):
        super().__init__(dmodel, num_heads, n_layers, ctx_size, None, ffn_hidden, precision, tp)
        self.vocab_size, self.padding_idx = vocab_size, padding_idx
        self.emb = nn.Parameter(torch.randn(vocab_size, dmodel) * 0.02)
        if device is not None:
            self.to(device)

    def embed(self, x):
        return self.run_layers(A.embedding(x, self.emb, self.padding_idx, dtype=self.act_dtype))

    forward = embed


class LLamaStage(_Base):
    def __init__(self, dmodel=288, num_heads=6, device=None, n_layers=2, ctx_size=256, ffn_hidden=None,
                 precision="fp32", tp=None):
        super().__init__(dmodel, num_heads, n_layers, ctx_size, device, ffn_hidden, precision, tp)

    def forward(self, x):
        return self.run_layers(x)


class LLamaLastStage(_Base):
    def __init__(self, vocab_size, dmodel=288, num_heads=6, device=None, n_layers=2, ctx_size=256,
                 ffn_hidden=None, precision="fp32", tp=None):
        super().__init__(dmodel, num_heads, n_layers, ctx_size, None, ffn_hidden, precision, tp)
        self.vocab_size = vocab_size
        self.norm = nn.Parameter(torch.ones(dmodel))
        self.head = nn.Parameter(torch.randn(vocab_size, dmodel) * 0.02)
        if device is not None:
            self.to(device)

    def forward(self, x):
        h = A.rmsnorm(self.run_layers(x), self.norm)
        if getattr(self, "tp", None) is not None:  # head cut over the vocabulary: the local logit shard
            return A.linear(self.tp.copy(h), self.head)
        return A.linear(h, self.head)


class LLama(nn.Module):
    """Whole model (reference primer/intro.py:17-18): first stage + last stage, n_layers total."""

    def __init__(self, kind=CausalLLama, vocab_size=32000, dmodel=288, num_heads=6, device=None,
                 n_layers=6, ctx_size=256, padding_idx=None, ffn_hidden=None, precision="fp32"):
        super().__init__()
        n0 = n_layers // 2
        self.precision = precision
        self.first = LLamaFirstStage(vocab_size, dmodel, num_heads, None, n0, ctx_size, padding_idx,
                                     ffn_hidden, precision)
        self.last = LLamaLastStage(vocab_size, dmodel, num_heads, None, n_layers - n0, ctx_size, ffn_hidden,
                                   precision)
        if device is not None:
            self.to(device)

    lora = None  # the model's LoRAAdapters once models/lora.py: attach_lora has run

    def forward(self, x):
        return self.last(self.first.embed(x))

    # ------------------------------------------------------------------ generation (extension)
    def blocks(self):
        return list(self.first.layers) + list(self.last.layers)

    def _check_generation(self):
        if self.precision != "fp32":
            raise NotImplementedError(f"generation runs the fp32 kernels only (precision={self.precision!r})")
        if any(getattr(m, "tp", None) is not None for m in (self.first, self.last, *self.blocks())):
            raise NotImplementedError("generation from a tensor-parallel (sharded) model is not supported")

    @torch.no_grad()
    def _adapter_args(self, cache, adapters, adapter_ids):
        """Validate ``adapters`` / ``adapter_ids`` (host side) and put the ids into ``cache.aid``;
        with ids of None the cache keeps the ids it has."""
        if adapters is None:
            if adapter_ids is not None:
                raise ValueError("generation: adapter_ids without adapters")
            return
        adapters.check(self, cache.device)
        if adapter_ids is not None:
            cache.set_adapter_ids(adapter_ids, adapters.R)

    @torch.no_grad()
    def prefill(self, prompt_ids, prompt_lens, cache, adapters=None, adapter_ids=None):
        """Right-padded prompts [B, T] (real lengths ``prompt_lens`` [B]) through the blocks once:
        every layer's K (rotated) and V go into ``cache``, ``cache.lens = prompt_lens``; returns
        the logits of each sequence's last real position, [B, V] (``cache.logits``). ``adapters``
        (an ``AdapterBank``): sequence b runs adapter ``adapter_ids[b]`` (-1: the base model)."""
        from ..ops import llama_decode as D
        self._check_generation()
        self._adapter_args(cache, adapters, adapter_ids)
        B, T = prompt_ids.shape
        if B != cache.batch or T > cache.max_len:
            raise ValueError(f"prefill: prompts {B} x {T} do not fit the cache ({cache.batch} x {cache.max_len})")
        dev = cache.device
        lens = torch.as_tensor(prompt_lens, dtype=torch.int32).to(dev)
        x = A.embedding(prompt_ids.to(dev), self.first.emb, self.first.padding_idx, dtype=torch.float32)
        cache._gathered = None  # the bank's rows may have changed in place since the last prompts
        lo = cache.gathered(adapters)  # per-sequence (A, B) pairs, gathered once (identity without adapters)
        for i, blk in enumerate(self.blocks()):
            h, x = A.rmsnorm_fork(x, blk.norm1)
            qkv = lo(i, "wqkv", A.linear(h, blk.wqkv), h)
            D.kv_append(qkv, cache.k(i), cache.v(i), cache.cos, cache.sin, 0)
            att = A.causal_attention(qkv, blk.h, blk.hd)
            x = lo(i, "wo", A.linear(att, blk.wo, residual=x), att)
            h, x = A.rmsnorm_fork(x, blk.norm2)
            g = A.swiglu(lo(i, "w13", A.linear(h, blk.w13), h))
            x = lo(i, "w2", A.linear(g, blk.w2, residual=x), g)
        last = x[torch.arange(B, device=dev), (lens - 1).long()].contiguous()  # [B, D], no host sync
        if B <= D.LIN_ROWS_MAX_T:
            D.lin_rows(last, self.last.head.detach(), cache.logits, pro="rmsnorm", gain=self.last.norm.detach())
        else:
            cache.logits.copy_(A.linear(A.rmsnorm(last, self.last.norm), self.last.head))
        cache.lens.copy_(lens)
        cache.finished.zero_()
        cache.step.zero_()
        return cache.logits

    @torch.no_grad()
    def decode_step(self, cache, tokens=None, fused: bool = True, advance=None, adapters=None, adapter_ids=None):
        """One token per sequence through the cached model: ``tokens`` [B] (forced decoding) or
        ``cache.next_tok``. Launches: the embedding; per layer norm+qkv, attention with the cache
        append, wo+residual, norm+w13, swiglu+w2+residual; norm+head. ``fused=False`` runs the
        existing rmsnorm / swiglu kernels before plain skinny linears (A/B and cross-check).
        Returns the static [B, V] logits buffer. ``advance`` (default: when ``tokens`` are given)
        adds the appended row to ``cache.lens`` here; in ``generate`` the sampler does.
        ``adapters`` (an ``AdapterBank``): row b runs adapter ``cache.aid[b]`` (set from
        ``adapter_ids`` when given; -1: the base row, bit for bit) — one more launch per adapted
        linear, the shrink ``lora_rows_u``; the expand rides in the linear's epilogue."""
        from ..ops import llama_decode as D
        self._check_generation()
        c = cache
        self._adapter_args(c, adapters, adapter_ids)
        if tokens is not None:
            if not tokens.is_cuda and (int(tokens.min()) < 0 or int(tokens.max()) >= self.first.vocab_size):
                raise ValueError(f"decode_step: token outside [0, {self.first.vocab_size})")
            c.next_tok.copy_(tokens.to(torch.int32))
        c.embed(self.first.emb.detach())
        if c.batch > D.LIN_ROWS_MAX_T:
            self._decode_wide(c, adapters)
        else:
            xa, xb = c.xa, c.xb
            u = None if adapters is None else c.u_rows(adapters.rank)

            def lin(i, name, x, w, out, residual=None, pro="none", gain=None):
                pair = None if adapters is None else adapters.pair(i, name)
                lora = None
                if pair is not None:  # the shrink on the rows the linear stages, then the fused expand
                    D.lora_rows_u(x, pair[0], c.aid, u, pro, gain)
                    lora = (u, pair[1], c.aid, adapters.scale)
                D.lin_rows(x, w.detach(), out, residual, pro, gain, lora=lora)

            for i, blk in enumerate(self.blocks()):
                n1, n2 = blk.norm1.detach(), blk.norm2.detach()
                if fused:
                    lin(i, "wqkv", xa, blk.wqkv, c.qkv, pro="rmsnorm", gain=n1)
                else:
                    lin(i, "wqkv", c.rmsnorm(xa, n1), blk.wqkv, c.qkv)
                D.attn_decode(c.qkv, c.k(i), c.v(i), c.lens, c.cos, c.sin, c.att, c.splits, c.ws)
                lin(i, "wo", c.att, blk.wo, xb, residual=xa)
                if fused:
                    lin(i, "w13", xb, blk.w13, c.h13, pro="rmsnorm", gain=n2)
                    lin(i, "w2", c.h13, blk.w2, xa, residual=xb, pro="swiglu")
                else:
                    lin(i, "w13", c.rmsnorm(xb, n2), blk.w13, c.h13)
                    lin(i, "w2", c.swiglu(c.h13), blk.w2, xa, residual=xb)
            if fused:
                D.lin_rows(xa, self.last.head.detach(), c.logits, pro="rmsnorm", gain=self.last.norm.detach())
            else:
                D.lin_rows(c.rmsnorm(xa, self.last.norm.detach()), self.last.head.detach(), c.logits)
        if tokens is not None if advance is None else advance:
            c.lens.add_((c.lens < c.max_len).to(torch.int32))
        return c.logits

    def _decode_wide(self, c, adapters=None):
        """More than 16 sequences: the linears on the training engine (``A.linear``), the adapters
        through the training product (``lora_fwd``) on per-sequence gathered pairs; the decode
        attention and the sampler have no such limit."""
        from ..ops import llama_decode as D
        x = c.xa
        lo = c.gathered(adapters)
        for i, blk in enumerate(self.blocks()):
            h = A.rmsnorm(x, blk.norm1)
            c.qkv.copy_(lo(i, "wqkv", A.linear(h, blk.wqkv), h))
            D.attn_decode(c.qkv, c.k(i), c.v(i), c.lens, c.cos, c.sin, c.att, c.splits, c.ws)
            x = lo(i, "wo", A.linear(c.att, blk.wo, residual=x), c.att)
            h = A.rmsnorm(x, blk.norm2)
            g = A.swiglu(lo(i, "w13", A.linear(h, blk.w13), h))
            x = lo(i, "w2", A.linear(g, blk.w2, residual=x), g)
        c.logits.copy_(A.linear(A.rmsnorm(x, self.last.norm), self.last.head))

    @torch.no_grad()
    def generate(self, prompt_ids, prompt_lens=None, max_new_tokens: int = 32, temperature: float = 0.0,
                 top_k: int = 0, seed: int = 0, eos_id=None, graph=None, fused=None, return_logits: bool = False,
                 cache=None, adapters=None, adapter_ids=None):
        """Continue right-padded prompts [B, T] by ``max_new_tokens`` tokens -> int64 [B, N]
        (``return_logits``: also the fp32 [B, N, V] logits each token was drawn from).
        ``temperature == 0`` is greedy; else temperature / ``top_k`` sampling, a pure function of
        ``seed``. After ``eos_id`` a sequence emits ``eos_id``. One prefill, then N - 1 cached
        steps whose state (token, lengths, finished flags, Philox counter) stays on the device:
        the loop never waits for the GPU, and with ``graph`` every step is one HIP-graph replay.
        ``cache``: a ``KVCache`` to reuse (its captured step included). Unset ``graph`` /
        ``fused`` take ``GENERATE_DEFAULTS``. ``adapters`` (models/lora.py: ``adapter_bank``) with
        ``adapter_ids`` [B] (a list or int tensor; -1 = the base model): sequence b is continued
        under LoRA adapter ``adapter_ids[b]`` without merging anything. The captured step reads
        the ids from the device, so one capture serves any later assignment and any in-place
        change of the bank's rows. Without ``adapters`` the base model generates, adapters
        attached or not."""
        from ..ops import llama_decode as D
        self._check_generation()
        if prompt_ids.dim() != 2 or prompt_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError("generate: prompt_ids must be an integer tensor [B, T]")
        B, T = prompt_ids.shape
        N = int(max_new_tokens)
        V = self.first.vocab_size
        if prompt_lens is None:
            plens = [T] * B
        else:
            plens = [int(v) for v in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        if len(plens) != B or min(plens) < 1 or max(plens) > T:
            raise ValueError(f"generate: prompt_lens {plens} for prompts of shape {B} x {T}")
        if N < 1:
            raise ValueError("generate: max_new_tokens must be at least 1")
        ctx = self.first.ctx_size
        if max(plens) + N > ctx:
            raise ValueError(f"generate: prompt of {max(plens)} + {N} new tokens exceeds ctx_size {ctx}")
        lo, hi = (int(prompt_ids.min()), int(prompt_ids.max())) if not prompt_ids.is_cuda else \
            torch.stack([prompt_ids.min(), prompt_ids.max()]).tolist()  # the one read before the loop
        if lo < 0 or hi >= V:
            raise ValueError(f"generate: prompt token outside [0, {V})")
        eos = -1 if eos_id is None else int(eos_id)
        if eos >= V:
            raise ValueError(f"generate: eos_id {eos} outside the vocabulary")
        need = max(plens) + N
        if cache is None:
            cache = KVCache(self, B, need)
        elif cache.batch != B or cache.max_len < need:
            raise ValueError(f"generate: the cache ({cache.batch} x {cache.max_len}) does not fit {B} x {need}")
        if adapters is not None and adapter_ids is None:
            raise ValueError("generate: adapters need adapter_ids [B] (-1: the base model)")
        self._adapter_args(cache, adapters, adapter_ids)
        dev = cache.device
        on_gpu = dev.type == "cuda"
        fused = GENERATE_DEFAULTS["fused"] if fused is None else bool(fused)
        graph = (GENERATE_DEFAULTS["graph"] if graph is None else bool(graph)) and on_gpu \
            and B <= D.LIN_ROWS_MAX_T
        out = torch.zeros(B, N, dtype=torch.int32, device=dev)
        cache.out = out

        def one_step():
            self.decode_step(cache, fused=fused, adapters=adapters)
            D.sample(cache.logits, cache.next_tok, cache.out, cache.lens, cache.finished, cache.step,
                     cache.max_len, temperature, top_k, seed, eos, advance=True)

        step = one_step
        if graph:  # a captured step writes the token buffer it was recorded with, kept beside the graph
            key = (float(temperature), int(top_k), int(seed), eos, fused, N)
            step = cache.captured_step(key if adapters is None else key + adapters.key, one_step, N)
            out = cache.out
            out.zero_()
        logits = self.prefill(prompt_ids, plens, cache, adapters)
        all_logits = torch.empty(B, N, V, dtype=torch.float32, device=dev) if return_logits else None
        if return_logits:
            all_logits[:, 0].copy_(logits)
        D.sample(logits, cache.next_tok, out, cache.lens, cache.finished, cache.step, cache.max_len, temperature,
                 top_k, seed, eos, advance=False)
        for i in range(1, N):
            step()
            if return_logits:
                all_logits[:, i].copy_(cache.logits)
        toks = out.long()
        return (toks, all_logits) if return_logits else toks


# ``generate``'s defaults, as measured by benchmarks/bench_generate.py (profiles/generate.txt): the graph
# replay is 1.9x the eager loop at B = 1 and level with it at B = 16, the fused prologues 6-14 % ahead
GENERATE_DEFAULTS = {"graph": True, "fused": True}
# Per-sequence adapters take the two-launch route (the shrink ``lora_rows_u``, then the expand in the
# linear's epilogue), the only one built: 57 launches a step against 33, measured at +103 / +81 / +46 us
# a step at B = 1 / 8 / 16 (benchmarks/bench_generate.py --adapters 8, profiles/adapter_generate.txt). A
# one-launch variant that recomputes u in every workgroup was not built and is not a default.


class KVCache:
    """Everything a decode step reads or writes, allocated once: one fp32 buffer
    [layers][2][B][H][max_len][hd] (K stored rotated), the device-side sequence state (``lens``,
    ``finished``, ``next_tok``, the per-row step counter ``step``; int32 [B]), RoPE tables of
    ``max_len`` rows and the step's activation buffers; for per-sequence adapters the ids ``aid``
    (int32 [B], -1 = none) and one [B, 16] buffer for the shrink's ``u`` (the adapted linears run one
    after another on one stream, so one buffer serves them all)."""

    def __init__(self, model: "LLama", batch: int, max_len: int):
        from ..ops import llama_decode as D
        from ..ops.autograd_ops import rope_tables
        model._check_generation()
        if max_len < 1 or max_len > model.first.ctx_size:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, ctx_size = {model.first.ctx_size}]")
        if batch < 1:
            raise ValueError("KVCache: batch must be at least 1")
        blocks = model.blocks()
        dev = model.first.emb.device
        H, hd, Dm, V = blocks[0].h, blocks[0].hd, model.first.dmodel, model.first.vocab_size
        F = blocks[0].w2.shape[1]
        self.batch, self.max_len, self.device = batch, max_len, dev
        self.kv = torch.zeros(len(blocks), 2, batch, H, max_len, hd, dtype=torch.float32, device=dev)

        def ibuf():
            return torch.zeros(batch, dtype=torch.int32, device=dev)

        def fbuf(n):
            return torch.zeros(batch, n, dtype=torch.float32, device=dev)

        self.lens, self.finished, self.next_tok, self.step = ibuf(), ibuf(), ibuf(), ibuf()
        self.cos, self.sin = rope_tables(max_len, hd, dev)
        self.xa, self.xb, self.xn, self.att = fbuf(Dm), fbuf(Dm), fbuf(Dm), fbuf(Dm)
        self.qkv, self.h13, self.hh, self.logits = fbuf(3 * Dm), fbuf(2 * F), fbuf(F), fbuf(V)
        self.rstd = torch.zeros(batch, dtype=torch.float32, device=dev)
        self.splits = D.attn_splits(max_len)
        self.ws = D.attn_workspace(batch, H, hd, self.splits, dev)
        self.aid = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        self.u = fbuf(D.LORA_RANKS[-1])
        self._gathered = None
        self.out = None
        self._graphs: dict = {}

    def k(self, layer: int):
        return self.kv[layer, 0]

    def v(self, layer: int):
        return self.kv[layer, 1]

    # --- per-sequence adapters
    def set_adapter_ids(self, adapter_ids, R: int):
        """``adapter_ids`` (a list or int tensor [B], -1 = the base model) into ``aid``; values outside
        ``[-1, R)`` raise here, on the host."""
        ids = adapter_ids.tolist() if torch.is_tensor(adapter_ids) else list(adapter_ids)
        if len(ids) != self.batch or any(int(v) != v or not -1 <= v < R for v in ids):
            raise ValueError(f"adapter_ids {ids}: {self.batch} integers in [-1, {R}) expected")
        self.aid.copy_(torch.tensor([int(v) for v in ids], dtype=torch.int32))
        self._gathered = None

    def u_rows(self, rank: int):
        """The first B * rank floats of ``u`` as the shrink's [B, rank] output."""
        return self.u.view(-1)[:self.batch * rank].view(self.batch, rank)

    def gathered(self, bank):
        """``f(block, target, y, x) -> y`` for the paths off the hot one (prefill, more than 16
        sequences): y [B, ..., N] = the base linear of x [B, ..., D], with sequence b's adapter product
        added in place by the training kernel (``ops.lora.lora_fwd`` with S = B) on pairs gathered
        per sequence from ``aid`` (B zeroed where a sequence has no adapter). The gather is made once
        per prefill or id assignment (a copy: rows rewritten in place show from the next one on); no
        bank: the identity."""
        if bank is None:
            return lambda i, name, y, x: y
        from ..ops import lora as L
        if self._gathered is None or self._gathered[0] is not bank:
            slot, has = self.aid.clamp(min=0).long(), (self.aid >= 0).to(torch.float32)[:, None, None]
            self._gathered = (bank, {k: (a[slot].contiguous(), (b[slot] * has).contiguous())
                                     for k, (a, b) in bank.pairs.items()})
        pairs, nb = self._gathered[1], self.batch

        def add(i, name, y, x):
            pair = pairs.get((i, name))
            if pair is not None:
                L.lora_fwd(x.reshape(nb, -1, x.shape[-1]).contiguous(), pair[0], pair[1],
                           y.view(nb, -1, y.shape[-1]), bank.scale)
            return y

        return add

    # the step's launches that are not in ops/llama_decode.py: existing kernels on static buffers
    def embed(self, emb):
        if not emb.is_cuda:
            self.xa.copy_(emb[self.next_tok.long()])
            return
        from ..ops import llama_f32 as L32
        L32.check(L32.K().ddl_embf_fwd(L32.ptr(self.next_tok), L32.ptr(emb), L32.ptr(self.xa), self.batch,
                                       emb.shape[1], L32.stream()), "embf_fwd")

    def rmsnorm(self, x, g, eps=1e-6):
        if not x.is_cuda:
            self.xn.copy_(A.rmsnorm(x, g, eps))
            return self.xn
        from ..ops import llama_f32 as L32
        L32.check(L32.K().ddl_rmsf_fwd(L32.ptr(x), L32.ptr(g), L32.ptr(self.xn), L32.ptr(self.rstd), self.batch,
                                       x.shape[1], float(eps), L32.stream()), "rmsf_fwd")
        return self.xn

    def swiglu(self, ab):
        if not ab.is_cuda:
            self.hh.copy_(A.swiglu(ab))
            return self.hh
        from ..ops import llama_f32 as L32
        L32.check(L32.K().ddl_swiglu_f32_fwd(L32.ptr(ab), L32.ptr(self.hh), self.batch, self.hh.shape[1],
                                             L32.stream()), "swiglu_f32_fwd")
        return self.hh

    def captured_step(self, key, fn, n_out: int):
        """The HIP-graph replay of ``fn`` for these sampling parameters (single stream, no parallel
        branches), kept with the cache so a later ``generate`` replays without capturing again. The
        graph writes the cache's own token buffer ``self.out``."""
        from ..runtime.graphs import CapturedStep
        ent = self._graphs.get(key)
        if ent is None:
            ent = (CapturedStep(fn), torch.zeros(self.batch, n_out, dtype=torch.int32, device=self.device))
            self._graphs[key] = ent
        self.out = ent[1]
        return ent[0]


def split_stages(model: LLama, n_stages: int):
    """Cut a whole LLama into n_stages modules sharing its parameters (first / middle / last)."""
    blocks = list(model.first.layers) + list(model.last.layers)
    per = [len(blocks) // n_stages + (1 if i < len(blocks) % n_stages else 0) for i in range(n_stages)]
    out, s = [], 0
    for i, n in enumerate(per):
        mine = blocks[s:s + n]
        s += n
        if i == 0:
            st = LLamaFirstStage.__new__(LLamaFirstStage)
            nn.Module.__init__(st)
            st.emb, st.padding_idx, st.vocab_size = model.first.emb, model.first.padding_idx, model.first.vocab_size
        elif i == n_stages - 1:
            st = LLamaLastStage.__new__(LLamaLastStage)
            nn.Module.__init__(st)
            st.norm, st.head, st.vocab_size = model.last.norm, model.last.head, model.last.vocab_size
        else:
            st = LLamaStage.__new__(LLamaStage)
            nn.Module.__init__(st)
        st.layers = nn.ModuleList(mine)
        st.precision, st.act_dtype = model.precision, _act_dtype(model.precision)
        if n_stages == 1:
            st = model
        out.append(st)
    return out


def causalLLMLoss(logits, target, vocab_size=None, ignore_index=-100, scale: float = 1.0,  # noqa: N802
                  tp=None):
    """Next-token CE (reference name): logits[:, :-1] vs target[:, 1:]. On the device every row of
    the [B, S, V] logits goes to the fused kernel with the last position's label set to
    ``ignore_index`` (same mean, no copy of the [B, S-1, V] slice). ``scale`` (extension): a
    constant factor such as 1 / micro-batches, folded into the kernel's normaliser. ``tp``
    (extension): the tensor-parallel handle of a sharded last stage, whose ``logits`` are this
    rank's vocabulary shard of the ``vocab_size`` logits; the loss is then the vocabulary-parallel
    CE, the same bits on every rank of the group."""
    if tp is not None:
        return causalLLMLossTP(logits, target, vocab_size, tp, ignore_index, scale)
    if not logits.is_cuda:
        return A.cross_entropy_vocab(logits[:, :-1].contiguous(), target[:, 1:].contiguous(), ignore_index,
                                     scale)
    lab = torch.empty(target.shape, dtype=torch.int32, device=target.device)
    lab[:, :-1] = target[:, 1:]
    lab[:, -1] = ignore_index
    return A.cross_entropy_vocab(logits, lab, ignore_index, scale)


def causalLLMLossTP(logits_shard, target, vocab_size, tp, ignore_index=-100, scale: float = 1.0):  # noqa: N802
    """``causalLLMLoss`` over a vocabulary shard [B, S, Vl] (rank ``tp.rank`` of ``tp.degree``)."""
    from ..parallel.tp import vocab_range
    if vocab_size is None:
        raise ValueError("causalLLMLoss(tp=...): the full vocab_size is needed to place the shard")
    v0, v1 = vocab_range(vocab_size, tp.degree, tp.rank)
    if logits_shard.shape[-1] != v1 - v0:
        raise ValueError(f"logit shard of {logits_shard.shape[-1]} columns, rank {tp.rank}/{tp.degree} of "
                         f"vocabulary {vocab_size} holds {v1 - v0}")
    if not logits_shard.is_cuda:
        return A.cross_entropy_vocab_parallel(logits_shard[:, :-1].contiguous(), target[:, 1:].contiguous(), v0,
                                              vocab_size, tp.ctx, tp.group, ignore_index, scale)
    lab = torch.empty(target.shape, dtype=torch.int32, device=target.device)
    lab[:, :-1] = target[:, 1:]
    lab[:, -1] = ignore_index
    return A.cross_entropy_vocab_parallel(logits_shard, lab, v0, vocab_size, tp.ctx, tp.group, ignore_index, scale)
