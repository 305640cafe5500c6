"""Generation throughput of the fp32 LLaMA (LLama.generate, csrc/kernels/llama_decode.hip) on one GPU.

    python benchmarks/bench_generate.py [--out profiles/generate.txt]

The default model (288d, 6 layers, 6 heads, V 32000, ctx 256, random init), prompt 32, 224 new
tokens, greedy. Every figure is a median over ``--reps`` repeats; the A/B variants (graph on / off,
fused on / off) are alternated inside each repeat, so a drift of the shared machine hits all of
them alike. Times are host clocks around work that ends in a device synchronise.

  * tokens/s and us per step at B in {1, 8, 16}, graph x fused;
  * the baseline at B = 1: a full forward over the prefix per token through ``model(x)`` (what the
    tree offered before the KV cache), 64 new tokens;
  * per kernel (graph replays of 50 launches, so the host's launch cost is not in the figure):
    lin_rows at the model's five decode shapes against one read of its weight bytes at the 8 TB/s
    HBM specification, decode attention at L = 255 for B in {1, 16}, the sampler at V = 32000;
  * launches per step, counted from the chain the step runs.

``--adapters R`` measures per-sequence LoRA adapters instead (``generate(adapters=, adapter_ids=)``,
rank 8 on all four targets): the base step against the adapter step at each B with mixed ids, 16
personalised continuations in one call against 16 x (merge, generate at B = 1, unmerge), the two
adapter kernels at the model's shapes, and the step's overhead against its 24 extra launches.

    python benchmarks/bench_generate.py --adapters 8 --out profiles/adapter_generate.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddl25spring_amd.models.llama import KVCache, LLama  # noqa: E402
from ddl25spring_amd.ops import autograd_ops as A  # noqa: E402
from ddl25spring_amd.ops import llama_decode as D  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _sync_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_generate(model, B, prompt, new, reps, lines):
    dev = torch.device("cuda")
    torch.manual_seed(1)
    ids = torch.randint(0, model.first.vocab_size, (B, prompt), device=dev)
    variants = [(g, f) for g in (True, False) for f in (True, False)]
    caches = {v: KVCache(model, B, prompt + new) for v in variants}  # a variant keeps its captured step
    times = {v: [] for v in variants}
    ref = None
    for rep in range(reps + 1):  # repeat 0 warms up (and captures the graphs)
        for v in variants:
            out = []
            dt = _sync_time(lambda: out.append(model.generate(ids, max_new_tokens=new, graph=v[0], fused=v[1],
                                                              cache=caches[v])))
            if rep:
                times[v].append(dt)
            if v[1]:  # fused and unfused differ in rounding; graph on / off must not differ at all
                ref = out[0] if ref is None else ref
                assert torch.equal(out[0], ref), "graph replay changed the tokens"
    for v in variants:
        med = statistics.median(times[v])
        lines.append(f"generate B={B:2d} graph={int(v[0])} fused={int(v[1])}: {B * new / med:9.0f} tok/s  "
                     f"{1e6 * med / new:8.1f} us/step  (prefill included; min {1e3 * min(times[v]):.1f} ms, "
                     f"max {1e3 * max(times[v]):.1f} ms of {reps})")
    return {v: statistics.median(t) for v, t in times.items()}


def bench_baseline(model, prompt, new, reps, lines):
    """The only route without a cache: one full forward over the whole prefix per token."""
    dev = torch.device("cuda")
    torch.manual_seed(1)
    ids = torch.randint(0, model.first.vocab_size, (1, prompt), device=dev)

    def run():
        seq = ids
        with torch.no_grad():
            for _ in range(new):
                nxt = model(seq)[:, -1].argmax(-1, keepdim=True)
                seq = torch.cat([seq, nxt], 1)
        return seq

    cache = KVCache(model, 1, prompt + new)
    tb, tc = [], []
    for rep in range(reps + 1):
        a = _sync_time(run)
        b = _sync_time(lambda: model.generate(ids, max_new_tokens=new, cache=cache))
        if rep:
            tb.append(a)
            tc.append(b)
    mb, mc = statistics.median(tb), statistics.median(tc)
    lines.append(f"baseline B=1 full forward per token, {new} tokens from a prompt of {prompt}: {new / mb:8.0f} tok/s "
                 f"({1e6 * mb / new:.0f} us/token); cached generate, same run: {new / mc:8.0f} tok/s "
                 f"({1e6 * mc / new:.0f} us/token); speed-up {mb / mc:.1f}x")


def _graph_time(fn, n=50, reps=7) -> float:
    """Median seconds per call of ``fn`` from replays of a graph of n calls."""
    for _ in range(3):
        fn()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    return statistics.median(_sync_time(g.replay) for _ in range(reps)) / n


def bench_kernels(model, lines):
    dev = torch.device("cuda")
    blk = model.blocks()[0]
    Dm, F, V = model.first.dmodel, blk.w2.shape[1], model.first.vocab_size
    shapes = [("norm+qkv", blk.wqkv, "rmsnorm", blk.norm1, False), ("wo+res", blk.wo, "none", None, True),
              ("norm+w13", blk.w13, "rmsnorm", blk.norm2, False), ("swiglu+w2+res", blk.w2, "swiglu", None, True),
              ("norm+head", model.last.head, "rmsnorm", model.last.norm, False)]
    for B in (1, 16):
        for name, w, pro, gain, res in shapes:
            w = w.detach()
            K, C = w.shape
            x = torch.randn(B, 2 * C if pro == "swiglu" else C, device=dev)
            out, r = torch.empty(B, K, device=dev), torch.randn(B, K, device=dev)
            g = None if gain is None else gain.detach()
            t = _graph_time(lambda: D.lin_rows(x, w, out, r if res else None, pro, g))
            floor = 4.0 * K * C / HBM_BYTES_PER_S
            lines.append(f"lin_rows {name:14s} T={B:2d} C={C:4d} K={K:5d}: {1e6 * t:7.2f} us  "
                         f"(weights {4e-6 * K * C:6.2f} MB, {1e6 * floor:5.2f} us at 8 TB/s: {t / floor:5.1f}x)")
    H, hd, Smax = blk.h, blk.hd, model.first.ctx_size
    for B in (1, 16):
        kc, vc = torch.randn(B, H, Smax, hd, device=dev), torch.randn(B, H, Smax, hd, device=dev)
        qkv, out = torch.randn(B, 3 * Dm, device=dev), torch.empty(B, Dm, device=dev)
        lens = torch.full((B,), Smax - 1, dtype=torch.int32, device=dev)
        cos, sin = A.rope_tables(Smax, hd, dev)
        t = _graph_time(lambda: D.attn_decode(qkv, kc, vc, lens, cos, sin, out))
        byts = 2.0 * 4 * B * H * (Smax - 1) * hd
        lines.append(f"attn_decode B={B:2d} H={H} hd={hd} L={Smax - 1}: {1e6 * t:7.2f} us  "
                     f"(cache read {1e-6 * byts:5.2f} MB, {1e6 * byts / HBM_BYTES_PER_S:5.2f} us at 8 TB/s)")
    for B in (1, 16):
        lg = torch.randn(B, V, device=dev) * 3
        z = lambda: torch.zeros(B, dtype=torch.int32, device=dev)  # noqa: E731
        st = (z(), None, z(), z(), z())
        for label, kw in (("greedy", {}), ("T=0.8", dict(temperature=0.8)), ("T=0.8 top-k 20", dict(temperature=0.8, top_k=20))):
            t = _graph_time(lambda: D.sample(lg, *st, 1 << 30, **kw))
            lines.append(f"sample B={B:2d} V={V} {label:15s}: {1e6 * t:7.2f} us")
    n = len(model.blocks())
    lines.append(f"launches per step: fused {1 + 5 * n + 1 + 1} (embedding, 5 per layer x {n}, head, sampler); "
                 f"unfused {1 + 8 * n + 2 + 1}")


def _spread(ts, new):
    return f"{1e6 * statistics.median(ts) / new:8.1f} us/step (min {1e6 * min(ts) / new:.1f}, max {1e6 * max(ts) / new:.1f})"


def bench_adapters(model, R, batches, prompt, new, reps, lines):
    """Per-sequence LoRA adapters (rank 8, all four targets, R adapters, mixed ids with base rows):
    the base step against the adapter step per B, then 16 personalised continuations in one
    ``generate`` against the route without per-sequence adapters (16 x merge, B = 1, unmerge), the
    adapter kernels alone, and the step's overhead against its extra launches."""
    from ddl25spring_amd.models.lora import LoRAConfig, adapter_bank, attach_lora, merge_lora, unmerge_lora
    dev = torch.device("cuda")
    ad = attach_lora(model, R, LoRAConfig(rank=8, alpha=16.0), seed=0)
    rows = ad.make_optimizer().data
    g = torch.Generator().manual_seed(1)
    rows.copy_((torch.randn(rows.shape, generator=g) * 0.02).to(dev))
    bank = adapter_bank(model, rows)
    n_layers, n_t = len(model.blocks()), len(bank.targets)
    base_l, extra_l = 1 + 5 * n_layers + 2, n_t * n_layers
    lines.append(f"adapters: R = {R}, rank {bank.rank}, targets {','.join(bank.targets)}; launches per step: base "
                 f"{base_l}, with adapters {base_l + extra_l} (one shrink per adapted linear; the expand is fused)")
    torch.manual_seed(1)
    step_us = {}
    for B in batches:
        ids = torch.randint(0, model.first.vocab_size, (B, prompt), device=dev)
        aids = [(b % (R + 1)) - 1 for b in range(B)] if B > 1 else [0]
        caches = {v: KVCache(model, B, prompt + new) for v in ("base", "adapters")}
        times = {v: [] for v in caches}
        for rep in range(reps + 1):  # repeat 0 warms up and captures
            for v in caches:
                kw = dict(adapters=bank, adapter_ids=aids) if v == "adapters" else {}
                dt = _sync_time(lambda: model.generate(ids, max_new_tokens=new, cache=caches[v], **kw))
                if rep:
                    times[v].append(dt)
        for v in caches:
            lines.append(f"generate B={B:2d} {v:8s}: {B * new / statistics.median(times[v]):9.0f} tok/s  "
                         f"{_spread(times[v], new)}  (graph, fused, prefill included; of {reps})")
        step_us[B] = tuple(1e6 * statistics.median(times[v]) / new for v in ("base", "adapters"))
    # ---- 16 personalised continuations
    B = 16
    ids = torch.randint(0, model.first.vocab_size, (B, prompt), device=dev)
    aids = [b % R for b in range(B)]
    c16, c1 = KVCache(model, B, prompt + new), KVCache(model, 1, prompt + new)

    def merged_route():
        for b in range(B):
            merge_lora(model, rows[aids[b]])
            model.generate(ids[b:b + 1], max_new_tokens=new, cache=c1)
            unmerge_lora(model)

    ta, tm = [], []
    for rep in range(reps + 1):
        a = _sync_time(lambda: model.generate(ids, max_new_tokens=new, cache=c16, adapters=bank, adapter_ids=aids))
        m = _sync_time(merged_route)
        if rep:
            ta.append(a)
            tm.append(m)
    ma, mm = statistics.median(ta), statistics.median(tm)
    lines.append(f"16 personalised continuations of {new} tokens: one generate with adapter ids {1e3 * ma:8.1f} ms "
                 f"(min {1e3 * min(ta):.1f}, max {1e3 * max(ta):.1f}); 16 x (merge_lora, generate B=1, unmerge_lora) "
                 f"{1e3 * mm:8.1f} ms (min {1e3 * min(tm):.1f}, max {1e3 * max(tm):.1f}); ratio {mm / ma:.1f}x")
    # ---- the kernels alone (graph replays of 50 launches)
    blk = model.blocks()[0]
    shapes = [("norm+qkv", "wqkv", blk.wqkv, "rmsnorm", blk.norm1, False), ("wo+res", "wo", blk.wo, "none", None, True),
              ("norm+w13", "w13", blk.w13, "rmsnorm", blk.norm2, False),
              ("swiglu+w2+res", "w2", blk.w2, "swiglu", None, True)]
    for B in (1, 16):
        aid = torch.tensor([b % R for b in range(B)], dtype=torch.int32, device=dev)
        none = torch.full((B,), -1, dtype=torch.int32, device=dev)
        u = torch.zeros(B, bank.rank, device=dev)
        for name, t, w, pro, gain, res in shapes:
            w = w.detach()
            Kout, C = w.shape
            x = torch.randn(B, 2 * C if pro == "swiglu" else C, device=dev)
            out, r = torch.empty(B, Kout, device=dev), torch.randn(B, Kout, device=dev)
            gn = None if gain is None else gain.detach()
            pa, pb = bank.pair(0, t)
            t_plain = _graph_time(lambda: D.lin_rows(x, w, out, r if res else None, pro, gn))
            t_lora = _graph_time(lambda: D.lin_rows(x, w, out, r if res else None, pro, gn,
                                                    lora=(u, pb, aid, bank.scale)))
            t_u = _graph_time(lambda: D.lora_rows_u(x, pa, aid, u, pro, gn))
            lines.append(f"{name:14s} T={B:2d} C={C:4d} K={Kout:5d}: lin_rows {1e6 * t_plain:6.2f} us, with the fused "
                         f"expand {1e6 * t_lora:6.2f} us, lora_rows_u {1e6 * t_u:6.2f} us")
        x = torch.randn(B, blk.wo.shape[1], device=dev)
        t_none = _graph_time(lambda: D.lora_rows_u(x, bank.pair(0, "wo")[0], none, u))
        t_launch = _graph_time(lambda: u.zero_())
        base_us, ad_us = step_us.get(B, (float("nan"),) * 2)
        lines.append(f"per launch T={B:2d}: {1e6 * t_launch:5.2f} us (a fill of u's {u.numel()} floats; lora_rows_u with every "
                     f"id -1: {1e6 * t_none:5.2f} us); the step's {extra_l} extra launches: {1e6 * extra_l * t_launch:6.1f} us; "
                     f"measured step overhead {ad_us - base_us:6.1f} us ({ad_us:.1f} - {base_us:.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=32)
    ap.add_argument("--new", type=int, default=224)
    ap.add_argument("--baseline-new", type=int, default=64)
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--adapters", type=int, default=0,
                    help="R > 0: time generation with R per-sequence LoRA adapters instead (profiles/adapter_generate.txt)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate measures the GPU path: no GPU found")
    torch.manual_seed(0)
    model = LLama(device="cuda")
    lines = [f"bench_generate: LLama 288d / 6 layers / 6 heads / V 32000 / ctx 256, fp32, random init; prompt "
             f"{args.prompt}, {args.new} new tokens, greedy; medians of {args.reps} (variants alternated per repeat)"]
    batches = [int(b) for b in args.batches.split(",")]
    if args.adapters > 0:
        bench_adapters(model, args.adapters, batches, args.prompt, args.new, args.reps, lines)
    else:
        for B in batches:
            bench_generate(model, B, args.prompt, args.new, args.reps, lines)
        bench_baseline(model, args.prompt, args.baseline_new, max(3, args.reps // 2), lines)
        bench_kernels(model, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
