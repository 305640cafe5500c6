"""Secure aggregation: what the masking costs next to the plain and the clipped mean, and what the
fixed-point uploads cost in accuracy.

``--agg`` times the aggregation alone over ``--K`` x ``--P`` client rows (default 8 x 11.2M,
ResNet-18's size) with HIP events, alternated ``--reps`` times in one session; the median of the
repetitions is reported. Timed: the plain weighted mean; the clipped mean (update_sqnorm,
clip_scales, clipped_sum, apply_update); secagg's mask in its plain and its pair-shared form and
its open alone, and its whole route (update_sqnorm, clip_scales, secagg_mask, secagg_open,
apply_update) with either form, with a cohort of K of which all report, and of which 2 dropped
(K - 2 rows uploaded). Next to the times: the Philox calls of each kernel (plain mask: n per quad
per uploaded row; shared: one per local pair; open: one per quad per survivor and per
survivor-dropped pair) and calls per second, and the time one pass over the bytes takes at
``--hbm-tbs``.

Without ``--agg``: the 10-client MnistCnn setting of bench_compress.py (C = 0.5, B = 50, lr 0.05,
IID) with ``--dropout`` 0.2, FedAvg from the same initial model and seeds with the plain mean and
with secagg at 20 and 12 fractional bits: test accuracy after every round, rounds per second and the
aggregate phase's time.

    python benchmarks/bench_secagg.py [--rounds 10]
    python benchmarks/bench_secagg.py --agg [--K 8] [--P 0] [--iters 10] [--reps 5]
"""
from __future__ import annotations

import argparse
import statistics
import time

import torch

from _common import emit

METHODS = {"dense": None, "secagg20": 20, "secagg12": 12}


def _timed(calls: dict, iters: int, reps: int) -> dict:
    """Median ms per call of each entry, the entries alternated ``reps`` times."""
    times = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(2):
            f()
    for _ in range(reps):
        for name, f in calls.items():
            evs = []
            for _ in range(iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                evs.append((s, e))
            torch.cuda.synchronize()
            times[name].append(sum(s.elapsed_time(e) for s, e in evs) / iters)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def bench_agg(args, ctx):
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P, f = args.K, args.P, args.bits
    if P <= 0:
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    x = torch.randn(P, device=dev)
    rows = x + torch.randn(K, P, device=dev) * 0.01
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    out, delta = torch.empty(P, device=dev), torch.empty(P, device=dev)
    words = torch.empty(K, P, dtype=torch.int32, device=dev)
    sat = torch.zeros(K, dtype=torch.int32, device=dev)
    cohort = Fn.secagg_ids([3 * g + 1 for g in range(K)])  # not the identity
    gone = 2 if K > 3 else 0
    tab = lambda l: torch.tensor(l, dtype=torch.int32, device=dev)  # noqa: E731
    U, S, D = tab(cohort), tab(cohort[:K - gone]), tab(cohort[K - gone:])
    cs = Fn.clip_scales(Fn.update_sqnorm(rows, x), coeffs, 1.0)[1]

    def clipped():
        c = Fn.clip_scales(Fn.update_sqnorm(rows, x), coeffs, 1.0)[1]
        Fn.clipped_sum(rows, x, c, delta)
        Fn.apply_update(out, x, delta)

    def secure(G, alive, dropped, shared=None):
        c = Fn.clip_scales(Fn.update_sqnorm(rows[:G], x), coeffs[:G], 1.0)[1]
        Fn.secagg_mask(rows[:G], x, c, alive, U, f, 7, 1, words[:G], sat[:G], pair_shared=shared)
        Fn.secagg_open(words[:G], alive, dropped, f, 7, 1, delta)
        Fn.apply_update(out, x, delta)

    calls = {"mean_ms": lambda: Fn.weighted_sum(rows, coeffs, out),
             "clipped_ms": clipped,
             "secagg_mask_plain_ms": lambda: Fn.secagg_mask(rows, x, cs, U, U, f, 7, 1, words, sat, pair_shared=False),
             "secagg_mask_shared_ms": lambda: Fn.secagg_mask(rows, x, cs, U, U, f, 7, 1, words, sat, pair_shared=True),
             "secagg_open_ms": lambda: Fn.secagg_open(words, U, None, f, 7, 1, delta),
             "secagg_plain_ms": lambda: secure(K, U, None, False),
             "secagg_shared_ms": lambda: secure(K, U, None, True)}
    if gone:
        G = K - gone
        calls.update({
            f"secagg_mask_plain_{gone}dropped_ms": lambda: Fn.secagg_mask(rows[:G], x, cs[:G], S, U, f, 7, 1, words[:G],
                                                                          sat[:G], pair_shared=False),
            f"secagg_mask_shared_{gone}dropped_ms": lambda: Fn.secagg_mask(rows[:G], x, cs[:G], S, U, f, 7, 1, words[:G],
                                                                           sat[:G], pair_shared=True),
            f"secagg_open_{gone}dropped_ms": lambda: Fn.secagg_open(words[:G], S, D, f, 7, 1, delta),
            f"secagg_plain_{gone}dropped_ms": lambda: secure(G, S, D, False),
            f"secagg_shared_{gone}dropped_ms": lambda: secure(G, S, D, True)})
    res = _timed(calls, args.iters, args.reps)
    nq = (P + 3) // 4

    def shared_calls(G):  # G self masks, one call per local pair, G per member elsewhere
        return (G + G * (G - 1) // 2 + G * (K - G)) * nq if 2 <= G <= 8 else G * K * nq

    philox = {"mask_plain": K * K * nq, "mask_shared": shared_calls(K), "open": K * nq}
    if gone:
        G = K - gone
        philox.update({f"mask_plain_{gone}dropped": G * K * nq, f"mask_shared_{gone}dropped": shared_calls(G),
                       f"open_{gone}dropped": (G + G * gone) * nq})
    for name, calls_ in philox.items():  # 10^9 Philox calls per second of each timed kernel
        res[f"secagg_{name}_gphilox_s"] = round(calls_ / res[f"secagg_{name}_ms"] / 1e6, 2)
    # 4-byte words per pass: the mean K + 1; the clipped mean 2K + 2 (norms), K + 2 (sum), 3 (apply);
    # secagg's mask 2K + 1 (rows and centre read, words written) and open K + 1
    moved = {"mean": (K + 1) * P, "clipped": (2 * K + 7) * P, "secagg_mask": (2 * K + 1) * P, "secagg_open": (K + 1) * P}
    hbm = {f"{k}_one_pass_hbm_ms": round(v * 4 / (args.hbm_tbs * 1e12) * 1e3, 4) for k, v in moved.items()}
    res.update(K=K, P=P, frac_bits=f, iters=args.iters, reps=args.reps, hbm_tbs=args.hbm_tbs, philox_calls=philox,
               words_moved=moved, **hbm, pair_shared_default=Fn.SECAGG_PAIR_SHARED, saturated=sat.cpu().tolist())
    emit(ctx, metric=f"secure aggregation over {K} x {P} client rows", unit="ms", **res)


def bench_methods(args, ctx):
    from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
    from ddl25spring_amd.data.split import split
    from ddl25spring_amd.fl.algorithms import FedAvg
    from ddl25spring_amd.models import mnist_cnn
    train = synthetic_images("mnist", args.train_size, seed=0)
    test = synthetic_images("mnist", args.test_size, seed=1)
    parts = split(args.clients, True, args.seed, labels=train.labels)
    data, tdata = DeviceImageDataset(train, ctx.device), DeviceImageDataset(test, ctx.device)
    results = {}
    for name in args.methods.split(","):
        kw = {} if METHODS[name] is None else dict(aggregator="secagg", agg_kwargs=dict(frac_bits=METHODS[name],
                                                                                       seed=args.seed))
        fa = FedAvg(lambda groups: mnist_cnn(groups=groups, precision=args.precision), data, parts,
                    lr=args.lr, batch_size=args.batch_size, client_fraction=args.client_fraction,
                    seed=args.seed, test_data=tdata, ctx=ctx, eval_every=0, dropout=args.dropout, **kw)
        fa.round()  # warm-up: graph capture and allocations stay out of the rate
        fa.timer.summary()
        acc, agg_ms, secs = [round(fa.test(), 2)], 0.0, 0.0
        for _ in range(args.rounds - 1):
            t0 = time.perf_counter()
            fa.round()
            secs += time.perf_counter() - t0
            agg_ms += fa.timer.summary().get("aggregate", 0.0)
            acc.append(round(fa.test(), 2))
        n = max(1, args.rounds - 1)
        results[name] = {"test_accuracy": acc, "rounds_per_s": round(n / max(secs, 1e-9), 2),
                         "aggregate_ms_per_round": round(agg_ms / n, 3),
                         "dropped": [len(d) for d in fa.dropped],
                         "aborted": list(getattr(fa.aggregator, "aborted", []))}
        del fa
    emit(ctx, metric="secure aggregation, test accuracy per round (MnistCnn, synthetic MNIST shape)", unit="%",
         n_gpus=ctx.world, rounds=args.rounds, clients=args.clients, client_fraction=args.client_fraction,
         batch_size=args.batch_size, lr=args.lr, dropout=args.dropout, dtype=args.precision, data="synthetic",
         results=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agg", action="store_true", help="time the aggregation alone")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the one-pass time (MI355X spec: 8 TB/s)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--P", type=int, default=0, help="row length (default: ResNet-18's padded row, 11.2M)")
    ap.add_argument("--bits", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--clients", type=int, default=10)
    ap.add_argument("--client-fraction", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--train-size", type=int, default=3000)
    ap.add_argument("--test-size", type=int, default=1000)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init()
    if args.agg:
        if ctx.device.type != "cuda":
            raise SystemExit("--agg times the HIP kernels: it needs a GPU")
        bench_agg(args, ctx)
    else:
        bench_methods(args, ctx)
    rdist.shutdown()


if __name__ == "__main__":
    main()
