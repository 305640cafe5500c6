"""Vocabulary-parallel CE pair (ddl_cevp_stats + ddl_cevp_grad) against the full-row ddl_cevf on the
same [rows, V] fp32 logits, alternated in one process, medians over rounds (device events).

By bytes the pair reads the logits twice and writes the gradient once (3 passes) where ddl_cevf
reads once and writes once (2): 1.5x is the budget at W = 1. The W = 2 line times one rank's work
on a shard of V / 2 columns (its records stacked with the peer's, as the all-gather leaves them).
Also prints which engine each sharded linear of the benchmark model lands on.

    python scripts/cevp_bench.py [--rows 8192] [--vocab 32000] [--rounds 7] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from ddl25spring_amd.ops import _lib
    from ddl25spring_amd.ops import llama_f32 as L32
    from ddl25spring_amd.ops._lib import check, ptr, stream
    from ddl25spring_amd.parallel.tp import vocab_range
    K = _lib.kernels()
    dev = torch.device("cuda")
    R, V = a.rows, a.vocab
    torch.manual_seed(0)
    z = torch.randn(R, V, device=dev) * 2
    lab = torch.randint(0, V, (R,), device=dev, dtype=torch.int32)
    inv = torch.full((1,), 1.0 / R, device=dev)
    loss, rowloss, d = torch.empty(1, device=dev), torch.empty(R, device=dev), torch.empty_like(z)
    v0, v1 = vocab_range(V, 2, 0)
    zs = z[:, v0:v1].contiguous()
    ds = torch.empty_like(zs)
    st1 = torch.empty(1, R, 4, device=dev)
    st2 = torch.stack([L32.cevp_stats(zs, lab, v0), L32.cevp_stats(z[:, v1:].contiguous(), lab, v1)])

    def cevf():
        check(K.ddl_cevf(ptr(z), ptr(lab), R, V, V, ptr(inv), -100, ptr(rowloss), ptr(loss), ptr(d), V, stream()),
              "cevf")

    def pair(zz, dd, st, W, lo, width):
        def run():
            check(K.ddl_cevp_stats(ptr(zz), ptr(lab), R, width, width, lo, -100, ptr(st[0]), stream()), "stats")
            check(K.ddl_cevp_grad(ptr(zz), ptr(lab), ptr(st), W, R, width, width, lo, V, ptr(inv), -100,
                                  ptr(rowloss), ptr(loss), ptr(dd), width, stream()), "grad")
        return run

    def stats_only():
        check(K.ddl_cevp_stats(ptr(z), ptr(lab), R, V, V, 0, -100, ptr(st1[0]), stream()), "stats")

    runs = {"cevf": cevf, "cevp_w1": pair(z, d, st1, 1, 0, V), "cevp_w1_stats_only": stats_only,
            "cevp_w2_shard": pair(zs, ds, st2, 2, v0, v1 - v0)}
    times = {k: [] for k in runs}
    for fn in runs.values():
        _time(fn, 3)
    for _ in range(a.rounds):  # alternate the variants inside every round
        for k, fn in runs.items():
            times[k].append(_time(fn, a.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"rows": R, "vocab": V, "shard_cols": v1 - v0, "rounds": a.rounds, "iters": a.iters,
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "pair_over_cevf": round(med["cevp_w1"] / med["cevf"], 3),
           "GBps": {"cevf": round(2 * R * V * 4 / med["cevf"] / 1e6, 1),
                    "cevp_w1": round(3 * R * V * 4 / med["cevp_w1"] / 1e6, 1),
                    "cevp_w2_shard": round(3 * R * (v1 - v0) * 4 / med["cevp_w2_shard"] / 1e6, 1)}}
    print(json.dumps(out))
    # engines of the sharded linears of the benchmark model (dmodel 288, F 768, batch 32 x 256) at tp = 2
    T, D, F = 32 * 256, 288, 768
    shapes = {"wqkv": (D, 3 * D // 2), "wo": (D // 2, D), "w13": (D, 2 * F // 2), "w2": (F // 2, D),
              "head": (D, v1 - v0)}
    eng = {n: [L32.linear_engine(m, T, c, k) for m in range(3)] for n, (c, k) in shapes.items()}
    print(json.dumps({"tp2_linear_engines_fwd_dgrad_wgrad": eng, "T": T}))


if __name__ == "__main__":
    main()
