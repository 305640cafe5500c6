"""Client-batched LoRA training step of the fp32 LLaMA (models/lora.py, csrc/kernels/lora.hip) on one GPU.

    python benchmarks/bench_fedlora.py [--out profiles/fedlora.txt]

The default model (288d, 6 layers, 6 heads, V 32000, ctx 256, random init), S = 8 clients x 4
sequences, rank 8 on all four targets. One step = forward + CE + backward over the slot-major batch +
one SlotAdam launch. Three variants are alternated inside each repeat, so a drift of the shared
machine hits all of them alike; every figure is a median over ``--reps`` repeats of ``--steps`` steps:

  (a) native    the adapters on the fused kernels of ops/lora.py;
  (b) composed  the same adapters from torch.bmm and autograd on the output of the base linear;
  (c) full      a full fine-tuning step at the same token count (benchmarks/bench_llm.py's eager
                path: every weight trained, FlatAdam), for context.

Also: the time of each LoRA kernel at the model's four linear shapes (graph replays of 20 launches,
so the host's launch cost is not in the figure) next to the time of its bytes at the 8 TB/s HBM
specification, and the peak device memory of a step of (a) against (c).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ddl25spring_amd.models.llama import LLama, causalLLMLoss  # noqa: E402
from ddl25spring_amd.models.lora import LoRAConfig, attach_lora  # noqa: E402
from ddl25spring_amd.ops import lora as L  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _sync_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _graph_time(fn, n=20, reps=7) -> float:
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


def bench_steps(args, lines):
    dev = torch.device("cuda")
    S, b, ctx, r = args.slots, args.seqs, 256, args.rank
    torch.manual_seed(0)
    x = torch.randint(0, 32000, (S * b, ctx), device=dev)
    tokens = S * b * ctx

    rest0 = torch.cuda.memory_allocated()
    model = LLama(device="cuda")
    ad = attach_lora(model, S, LoRAConfig(rank=r, alpha=2.0 * r), seed=0)
    opt = ad.make_optimizer(lr=1e-3)
    with torch.no_grad():  # B != 0, so that no product is trivially zero
        for n, p in ad.named.items():
            if n.endswith(".B"):
                p.normal_(std=0.02)

    def lora_step(route):
        def step():
            ad.route = route
            opt.zero_grad()
            causalLLMLoss(model(x), x, scale=float(S)).backward()
            opt.step()
        return step

    for route in ("native", "composed"):
        for _ in range(2):
            lora_step(route)()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    lora_step("native")()
    torch.cuda.synchronize()
    peak_a = torch.cuda.max_memory_allocated() - rest0

    rest1 = torch.cuda.memory_allocated()
    from ddl25spring_amd.optim import FlatAdam
    torch.manual_seed(0)
    full = LLama(device="cuda")
    fopt = FlatAdam(full.parameters(), lr=1e-3, fused=True)

    def full_step():
        fopt.zero_grad()
        causalLLMLoss(full(x), x).backward()
        fopt.step()

    for _ in range(2):
        full_step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    full_step()
    torch.cuda.synchronize()
    peak_c = torch.cuda.max_memory_allocated() - rest1

    variants = {"native": lora_step("native"), "composed": lora_step("composed"), "full": full_step}
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            times[k].append(_sync_time(lambda: [fn() for _ in range(args.steps)]) / args.steps)
    ad.route = "native"
    med = {k: statistics.median(v) for k, v in times.items()}
    label = {"native": "(a) LoRA, native kernels ", "composed": "(b) LoRA, composed (bmm) ",
             "full": "(c) full fine-tuning     "}
    for k in variants:
        lines.append(f"{label[k]}: {tokens / med[k]:9.0f} tok/s  {1e3 * med[k]:7.2f} ms/step  "
                     f"(min {1e3 * min(times[k]):.2f}, max {1e3 * max(times[k]):.2f} of {args.reps})")
    lines.append(f"native / composed step time: {med['native'] / med['composed']:.3f}; "
                 f"native / full: {med['native'] / med['full']:.3f}")
    lines.append(f"peak device memory of one step above the resident set before the model was built: "
                 f"(a) {peak_a / 2**20:.0f} MiB (frozen base + {S} adapters of {opt.P} floats + Adam state + "
                 f"activations), (c) {peak_c / 2**20:.0f} MiB (weights + gradients + Adam state + activations)")
    return med


def bench_kernels(args, lines):
    dev = torch.device("cuda")
    S, T, r = args.slots, args.seqs * 256, args.rank
    Dm, F = 288, 768
    for name, D, N in (("wqkv", Dm, 3 * Dm), ("wo", Dm, Dm), ("w13", Dm, 2 * F), ("w2", F, Dm)):
        x, y = torch.randn(S, T, D, device=dev), torch.randn(S, T, N, device=dev)
        dy, dx = torch.randn(S, T, N, device=dev), torch.empty(S, T, D, device=dev)
        A, B = torch.randn(S, r, D, device=dev) / D ** 0.5, torch.randn(S, N, r, device=dev) * 0.02
        dA, dB = torch.zeros_like(A), torch.zeros_like(B)
        u, v = torch.empty(S, T, r, device=dev), torch.empty(S, T, r, device=dev)
        f4 = 4.0 * S * T
        rows = (("fwd", lambda: L.lora_fwd_out(x, A, B, y, u, 2.0), f4 * (D + 2 * N + r)),
                ("bwd_x", lambda: L.lora_bwd_x(dy, A, B, 2.0, dx=dx, v=v), f4 * (N + D + r)),
                ("bwd_x (no dx)", lambda: L.lora_bwd_x(dy, A, B, 2.0, v=v), f4 * (N + r)),
                ("bwd_w", lambda: L.lora_bwd_w(x, dy, u, v, dA, dB, 2.0), f4 * (D + N + 2 * r)))
        for kname, fn, byts in rows:
            t = _graph_time(fn)
            floor = byts / HBM_BYTES_PER_S
            lines.append(f"lora_{kname:14s} {name:4s} S={S} T={T} D={D:4d} N={N:4d} r={r}: {1e6 * t:8.2f} us  "
                         f"({1e-6 * byts:6.2f} MB, {1e6 * floor:6.2f} us at 8 TB/s: {t / floor:5.1f}x)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--seqs", type=int, default=4)
    ap.add_argument("--rank", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fedlora measures the GPU path: no GPU found")
    lines = [f"bench_fedlora: LLama 288d / 6 layers / 6 heads / V 32000 / ctx 256, fp32, random init; S = {args.slots} "
             f"clients x {args.seqs} sequences, rank {args.rank}, targets wqkv wo w13 w2; medians of {args.reps} "
             f"repeats of {args.steps} steps (variants alternated per repeat)"]
    bench_steps(args, lines)
    bench_kernels(args, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
