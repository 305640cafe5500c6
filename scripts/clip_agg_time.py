"""Clipped aggregation time on one GPU (csrc/kernels/clip_agg.hip) against the plain weighted sum.

Per shape, after warm-up and alternating within one run: (a) ``Fn.weighted_sum`` (one read of the
rows: the yardstick), (b) update_sqnorm + clip_scales + clipped_sum + apply_update together, (c)
each of the four alone. Device events around ``--iters`` back-to-back calls, ``--reps`` such windows
per item taken in turn; reported: the median window, the min..max spread, and the bytes the op has
to move over the median time.

    python scripts/clip_agg_time.py [--iters 50] [--reps 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ddl25spring_amd.ops import functional as Fn  # noqa: E402

SHAPES = (("resnet18_cifar", 8), ("mnist_cnn", 10))


def row_length(model: str) -> int:
    """P of the model's flat parameter row as the FL loop hands it over (every tensor padded to 16
    floats, so rows start 16-B aligned and the kernels take their vector path)."""
    from ddl25spring_amd import models
    net = models.resnet18_cifar(10, groups=1) if model == "resnet18_cifar" else models.mnist_cnn(groups=1)
    return int(net.to("cpu", seed=0).store.data.shape[1])


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--std", type=float, default=1e-3, help="noise std of the apply pass (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []
    for name, G in SHAPES:
        P = row_length(name)
        g = torch.Generator(device=dev).manual_seed(0)
        center = torch.randn(P, device=dev, generator=g)
        rows = center + 0.01 * torch.randn(G, P, device=dev, generator=g)
        coeff = torch.full((G,), 1.0 / G, device=dev)
        out, delta, w = (torch.empty(P, device=dev) for _ in range(3))
        clip = 0.01 * P ** 0.5  # the typical update norm: about half the rows are clipped
        sq = Fn.update_sqnorm(rows, center)
        _, cs = Fn.clip_scales(sq, coeff, clip)

        def four():
            q = Fn.update_sqnorm(rows, center)
            _, c = Fn.clip_scales(q, coeff, clip)
            Fn.clipped_sum(rows, center, c, delta)
            Fn.apply_update(w, center, delta, args.std, 1, 2)

        row_bytes, vec_bytes = 4 * G * P, 4 * P
        items = {  # name -> (callable, bytes it has to move)
            "weighted_sum": (lambda: Fn.weighted_sum(rows, coeff, out), row_bytes + vec_bytes),
            "four_launches": (four, 2 * row_bytes + 6 * vec_bytes),
            "update_sqnorm": (lambda: Fn.update_sqnorm(rows, center), row_bytes + vec_bytes),
            "clip_scales": (lambda: Fn.clip_scales(sq, coeff, clip), 0),
            "clipped_sum": (lambda: Fn.clipped_sum(rows, center, cs, delta), row_bytes + 2 * vec_bytes),
            "apply_update": (lambda: Fn.apply_update(w, center, delta, args.std, 1, 2), 3 * vec_bytes),
            "apply_update_std0": (lambda: Fn.apply_update(w, center, delta, 0.0), 3 * vec_bytes),
        }
        for fn, _ in items.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in items}
        for _ in range(args.reps):  # alternate: every item once per repetition
            for k, (fn, _) in items.items():
                times[k].append(window(fn, args.iters))
        rec = {"shape": name, "G": G, "P": P, "iters": args.iters, "reps": args.reps, "std": args.std}
        for k, (_, nbytes) in items.items():
            med = statistics.median(times[k])
            rec[k] = {"ms": round(med, 4), "min_ms": round(min(times[k]), 4), "max_ms": round(max(times[k]), 4),
                      "GBps": round(nbytes / med / 1e6, 1)}
        rec["four_over_weighted_sum"] = round(rec["four_launches"]["ms"] / rec["weighted_sum"]["ms"], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
