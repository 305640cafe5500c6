"""The backdoor attack against the aggregation rules, and what the sign-vote (RLR) kernels cost.

Without ``--agg``: FedAvg of the MLP (B = 50, lr 0.1, IID, every client every round) on the synthetic
MNIST shape, for each of ``--seeds`` server seeds and two federations: ``--clients`` clients of which
``--attackers`` plant a ``--patch`` x ``--patch`` trigger on half of their data with ``--boost``, and
``--clients2`` clients (twice the data) of which ``--attackers2`` do with ``--boost2``. Rules: the plain
mean, the clipped mean (radius: the median update norm of the first clean round), the coordinate
median, Krum and ``rlr`` at each of ``--thetas`` / ``--thetas2``, next to a clean run under the mean.
Reported: test accuracy and attack success rate (the accuracy on the triggered test set) after the
rounds of ``--report``. Nothing is promised about which rule wins: the table is the finding.

``--agg`` times the kernels alone over ``--K`` x ``--P`` client rows (default 8 x 11.2M, ResNet-18's
size) with HIP events: the plain weighted mean (the yardstick), ``clipped_sum``, ``rlr_sum`` in final
mode without and with a votes buffer, and partial mode followed by ``rlr_flip``. The entries are
alternated ``--reps`` times of ``--iters`` calls in one session and the median taken; the whole block
is repeated ``--blocks`` times, and the spread of those medians is reported with them.

    python benchmarks/bench_backdoor.py [--seeds 3,11,21]
    python benchmarks/bench_backdoor.py --agg [--K 8] [--P 0] [--iters 10] [--reps 5] [--blocks 3]
"""
from __future__ import annotations

import argparse
import statistics

import torch

from _common import emit
from bench_collusion import _timed


def bench_agg(args, ctx):
    from ddl25spring_amd.fl import aggregate as A
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P = args.K, args.P
    if P <= 0:
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    x = torch.randn(P, device=dev)
    rows = x + torch.randn(K, P, device=dev) * 0.01
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    out, delta, votes = (torch.empty(P, device=dev) for _ in range(3))
    theta = K / 2

    def two_step():
        Fn.rlr_sum(rows, x, coeffs, delta, votes)
        Fn.rlr_flip(delta, votes, theta)

    calls = {"mean_ms": lambda: Fn.weighted_sum(rows, coeffs, out),
             "clipped_sum_ms": lambda: Fn.clipped_sum(rows, x, coeffs, delta),
             "rlr_sum_final_ms": lambda: Fn.rlr_sum(rows, x, coeffs, delta, None, theta),
             "rlr_sum_final_votes_ms": lambda: Fn.rlr_sum(rows, x, coeffs, delta, votes, theta),
             "rlr_partial_flip_ms": two_step}
    blocks = [_timed(calls, args.iters, args.reps) for _ in range(args.blocks)]
    res = {}
    for name in calls:
        med = [b[name]["median"] for b in blocks]
        res[name] = {"median": round(statistics.median(med), 4), "medians": med, "spread": round(max(med) - min(med), 4),
                     "min": min(b[name]["min"] for b in blocks), "max": max(b[name]["max"] for b in blocks)}
    Fn.rlr_sum(rows, x, coeffs, delta, votes, theta)
    flipped = int((votes.abs() < theta).sum())
    # 4-byte words per coordinate: the mean K + 1; clipped_sum and rlr_sum K + 2 (rows, centre, delta), one
    # more with the votes; partial + flip (K + 3) + 3
    moved = {"mean": K + 1, "clipped_sum": K + 2, "rlr_sum_final": K + 2, "rlr_sum_final_votes": K + 3,
             "rlr_partial_flip": K + 6}
    hbm = {f"{k}_one_pass_hbm_ms": round(v * P * 4 / (args.hbm_tbs * 1e12) * 1e3, 4) for k, v in moved.items()}
    base = res["clipped_sum_ms"]
    allowed = max(1.10 * base["median"], base["median"] + base["spread"])
    emit(ctx, metric=f"sign-vote (RLR) aggregation kernels over {K} x {P} client rows", unit="ms", K=K, P=P, theta=theta,
         flipped=flipped, iters=args.iters, reps=args.reps, blocks=args.blocks, hbm_tbs=args.hbm_tbs,
         words_per_coordinate=moved, **hbm, **res, rlr_sum_allowed_ms=round(allowed, 4),
         rlr_sum_within_allowance=res["rlr_sum_final_ms"]["median"] <= allowed,
         keep_votes_cost_ms=round(res["rlr_sum_final_votes_ms"]["median"] - res["rlr_sum_final_ms"]["median"], 4),
         fused_gain_ms=round(res["rlr_partial_flip_ms"]["median"] - res["rlr_sum_final_ms"]["median"], 4),
         fuse_default=A.RobustLR.fuse)


def _federation(args, ctx, seed, clients, attackers, boost, train_size, thetas):
    from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
    from ddl25spring_amd.data.split import split
    from ddl25spring_amd.fl.algorithms import FedAvg
    from ddl25spring_amd.fl.attacks import Backdoor
    from ddl25spring_amd.models import mnist_mlp
    atk = Backdoor(list(range(attackers)), target=args.target, poison_fraction=args.fraction, patch=args.patch,
                   boost=boost, seed=seed)
    clean = synthetic_images("mnist", train_size, seed=0)
    test = synthetic_images("mnist", args.test_size, seed=1)
    parts = split(clients, True, seed, labels=clean.labels)
    poisoned, bad_parts = atk.poison(clean, parts)
    sets = {False: (DeviceImageDataset(clean, ctx.device), parts), True: (DeviceImageDataset(poisoned, ctx.device), bad_parts)}
    tdata = DeviceImageDataset(test, ctx.device)
    trig = DeviceImageDataset(atk.triggered_test(test), ctx.device)
    report = [int(r) for r in args.report.split(",")]

    def fed(rule, attacked, **agg_kw):
        data, idx = sets[attacked]
        return FedAvg(lambda groups: mnist_mlp(groups=groups, precision=args.precision), data, idx, lr=args.lr,
                      batch_size=args.batch_size, client_fraction=1.0, seed=seed, test_data=tdata, backdoor_test=trig,
                      ctx=ctx, eval_every=0, aggregator=rule, attack=atk if attacked else None, agg_kwargs=agg_kw)

    def run(fa):
        acc = {}
        for r in range(1, max(report) + 1):
            fa.round()
            if r in report:
                acc[f"round_{r}"] = {"accuracy": round(fa.test(), 2), "asr": round(fa.test_backdoor(), 2)}
        return acc

    # the clipping radius: the median update norm of the first clean round
    probe = fed("clipped", False, clip=1e30)
    probe.round()
    tau = float(statistics.median(probe.aggregator.last_norms))
    del probe
    results = {"clean_mean": run(fed("mean", False))}
    for rule, kw in (("mean", {}), ("clipped", {"clip": tau}), ("median", {}), ("krum", {"f": attackers})):
        results[rule] = run(fed(rule, True, **kw))
    for th in thetas:
        fa = fed("rlr", True, theta=th)
        fa.aggregator.keep_votes = True
        results[f"rlr_theta_{th:g}"] = run(fa)
        results[f"rlr_theta_{th:g}"]["flipped_last_round"] = round(fa.aggregator.last_flipped / fa.w_global.numel(), 4)
    emit(ctx, metric="backdoor attack against the aggregation rules, test accuracy and attack success rate "
         "(MLP, synthetic MNIST shape)", unit="%", n_gpus=ctx.world, seed=seed, clients=clients, attackers=attackers,
         boost=boost, patch=args.patch, poison_fraction=args.fraction, target=args.target, train_size=train_size,
         batch_size=args.batch_size, lr=args.lr, dtype=args.precision, data="synthetic", clip=round(tau, 5),
         results=results)


def bench_table(args, ctx):
    for seed in (int(s) for s in args.seeds.split(",")):
        _federation(args, ctx, seed, args.clients, args.attackers, args.boost, args.train_size,
                    [float(t) for t in args.thetas.split(",")])
        if args.clients2:
            _federation(args, ctx, seed, args.clients2, args.attackers2, args.boost2, 2 * args.train_size,
                        [float(t) for t in args.thetas2.split(",")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agg", action="store_true", help="time the kernels alone")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the one-pass time (MI355X spec: 8 TB/s)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--P", type=int, default=0, help="row length (default: ResNet-18's padded row, 11.2M)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3, help="repetitions of the whole alternated block")
    ap.add_argument("--seeds", default="3,11,21")
    ap.add_argument("--report", default="6,12", help="rounds after which accuracy and ASR are reported")
    ap.add_argument("--clients", type=int, default=10)
    ap.add_argument("--attackers", type=int, default=3)
    ap.add_argument("--boost", type=float, default=3.0)
    ap.add_argument("--thetas", default="4,6")
    ap.add_argument("--clients2", type=int, default=20, help="clients of the second federation (0: none)")
    ap.add_argument("--attackers2", type=int, default=2)
    ap.add_argument("--boost2", type=float, default=5.0)
    ap.add_argument("--thetas2", default="6,8,10")
    ap.add_argument("--target", type=int, default=0)
    ap.add_argument("--patch", type=int, default=6)
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--train-size", type=int, default=6000)
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
        bench_table(args, ctx)
    rdist.shutdown()


if __name__ == "__main__":
    main()
