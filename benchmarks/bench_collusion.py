"""Colluding attacks (ALIE, IPM) against the aggregation rules, and what the new kernels cost.

Without ``--agg``: the 10-client MnistCnn setting of bench_noniid.py / bench_secagg.py (B = 50, lr
0.05, IID, one seed) with ``--attackers`` colluders (clients 0..f-1) and ``--client-fraction`` 1.0, so
that every round holds them: FedAvg from the same initial model and seeds under the plain mean, the
coordinate median, the trimmed mean, Krum, the clipped mean, centered clipping and the geometric
median, clean and under ALIE (z = z_max of the round) and IPM (``--eps``); test accuracy after rounds
5 and 10 (``--report``). The clipping radius of both clipping rules is the median of the first clean
round's update norms, which are reported with it. Bulyan needs K >= 4f + 3 clients, so a second block
(``--bulyan-clients``, default 16, the same number of colluders; 0 skips it) runs every rule and Bulyan
at that size: its column compares like with like. Nothing is promised about which rule wins: the
table is the finding.

``--agg`` times the kernels alone over ``--K`` x ``--P`` client rows (default 8 x 11.2M, ResNet-18's
size) with HIP events, alternated ``--reps`` times in one session; median, minimum and maximum of the
repetitions are reported. Timed: the plain weighted mean over the K rows (the yardstick) and
``collude_rows`` with K - 2 sources and 2 destinations in both modes; the clipped mean, and
``CenteredClip`` with ``--cc-iters`` iterations on its fused and its unfused route, next to it
``GeometricMedian`` with ``--gm-iters`` on both routes; ``bulyan_select`` on a K x K Gram at K = 8, 32
and 128 (f = (K - 3) // 4), ``bulyan_coord`` over the rows with f = 1 (it reads theta = K - 2 of the K
rows) and, for comparison, ``coord_select("trimmed", 1)`` over the same rows.

    python benchmarks/bench_collusion.py [--rounds 10]
    python benchmarks/bench_collusion.py --agg [--K 8] [--P 0] [--iters 10] [--reps 5]
"""
from __future__ import annotations

import argparse
import statistics

import torch

from _common import emit

RULES = ("mean", "median", "trimmed_mean", "krum", "clipped", "centered_clip", "geomed")
ATTACKS = ("clean", "alie", "ipm")


def _timed(calls: dict, iters: int, reps: int) -> dict:
    """Per entry the median, minimum and maximum ms per call, the entries alternated ``reps`` times."""
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
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in times.items()}


def bench_agg(args, ctx):
    from ddl25spring_amd.fl import aggregate as A
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P, L = args.K, args.P, args.cc_iters
    if P <= 0:
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    x = torch.randn(P, device=dev)
    rows = x + torch.randn(K, P, device=dev) * 0.01
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    out, delta = torch.empty(P, device=dev), torch.empty(P, device=dev)
    nd = 2
    src_t = Fn.collude_table(list(range(nd, K)), K, dev)
    dst_t = Fn.collude_table(list(range(nd)), K, dev)
    tau = float(Fn.clip_scales(Fn.update_sqnorm(rows, x), coeffs, 1.0)[0].median())

    def clipped():
        c = Fn.clip_scales(Fn.update_sqnorm(rows, x), coeffs, tau)[1]
        Fn.clipped_sum(rows, x, c, delta)
        Fn.apply_update(out, x, delta)

    def centered(fuse):
        agg = A.CenteredClip(tau, L, warm_start=False)
        agg.fuse = fuse
        return lambda: agg(ctx, rows, coeffs, out, center=x, counts=[K])

    def geomed(fuse):
        agg = A.GeometricMedian(args.gm_iters)
        agg.fuse = fuse
        return lambda: agg(ctx, rows, coeffs, out, center=x, counts=[K])

    def selector(k):
        y = torch.randn(k, 4096, device=dev)
        gram = Fn.gram(y).contiguous()
        return lambda: Fn.bulyan_select(gram, (k - 3) // 4)

    bf = 1 if K >= 7 else 0  # Bulyan's f over the K rows
    theta = K - 2 * bf
    sel = torch.tensor(list(range(K - 1 - bf, bf - 1, -1)), dtype=torch.int32, device=dev)  # theta rows, descending
    calls = {"mean_ms": lambda: Fn.weighted_sum(rows, coeffs, out),
             "collude_alie_ms": lambda: Fn.collude_rows(rows, src_t, x, rows, dst_t, "alie", 0.5),
             "collude_ipm_ms": lambda: Fn.collude_rows(rows, src_t, x, rows, dst_t, "ipm", 0.5),
             "clipped_ms": clipped,
             "centered_clip_fused_ms": centered(True),
             "centered_clip_unfused_ms": centered(False),
             "geomed_fused_ms": geomed(True),
             "geomed_unfused_ms": geomed(False),
             "bulyan_select_k8_ms": selector(8),
             "bulyan_select_k32_ms": selector(32),
             "bulyan_select_k128_ms": selector(128),
             "bulyan_coord_ms": lambda: Fn.bulyan_coord(rows, sel, theta - 2 * bf),
             "trimmed_mean_ms": lambda: Fn.coord_select(rows, "trimmed", 1)}
    res = _timed(calls, args.iters, args.reps)
    ns = K - nd
    ratio = (ns + nd + 1) / (K + 1)
    # 4-byte words per coordinate: the mean K + 1; collude_rows ns + nd + 1; the clipped mean 2K + 7;
    # centered clipping fused (K + 1) + L (K + 5) after the 3 of ctr = c + v, unfused L (2K + 9), the
    # geometric median the same with its own L; bulyan_coord theta + 1, the trimmed mean K + 1
    Lg = args.gm_iters
    moved = {"mean": K + 1, "collude": ns + nd + 1, "clipped": 2 * K + 7,
             "centered_clip_fused": 3 + (K + 1) + L * (K + 5), "centered_clip_unfused": 3 + L * (2 * K + 9),
             "geomed_fused": 3 + (K + 1) + Lg * (K + 5), "geomed_unfused": 3 + Lg * (2 * K + 9),
             "bulyan_coord": theta + 1, "trimmed_mean": K + 1}
    hbm = {f"{k}_one_pass_hbm_ms": round(v * P * 4 / (args.hbm_tbs * 1e12) * 1e3, 4) for k, v in moved.items()}
    emit(ctx, metric=f"colluding attacks and centered clipping over {K} x {P} client rows", unit="ms", K=K, P=P,
         sources=ns, destinations=nd, cc_iters=L, gm_iters=Lg, bulyan_f=bf, bulyan_theta=theta, tau=round(tau, 5),
         iters=args.iters, reps=args.reps, hbm_tbs=args.hbm_tbs, words_per_coordinate=moved, **hbm, **res,
         collude_allowed_ms=round(1.5 * ratio * res["mean_ms"]["median"], 4),
         fused_gain_ms=round(res["centered_clip_unfused_ms"]["median"] - res["centered_clip_fused_ms"]["median"], 4),
         fuse_default=A.CenteredClip.fuse,
         bulyan_coord_ns_per_word=round(res["bulyan_coord_ms"]["median"] * 1e6 / ((theta + 1) * P), 6),
         trimmed_mean_ns_per_word=round(res["trimmed_mean_ms"]["median"] * 1e6 / ((K + 1) * P), 6))


def bench_table(args, ctx):
    from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
    train = synthetic_images("mnist", args.train_size, seed=0)
    test = synthetic_images("mnist", args.test_size, seed=1)
    data, tdata = DeviceImageDataset(train, ctx.device), DeviceImageDataset(test, ctx.device)
    bad = list(range(args.attackers))
    report = [int(r) for r in args.report.split(",")]
    blocks = [(args.clients, args.rules.split(","))]
    if args.bulyan_clients:
        if args.bulyan_clients < 4 * args.attackers + 3:
            raise SystemExit(f"--bulyan-clients {args.bulyan_clients}: Bulyan needs at least 4 * attackers + 3")
        blocks.append((args.bulyan_clients, args.rules.split(",") + ["bulyan"]))
    for clients, rules in blocks:
        _table_block(args, ctx, train, data, tdata, bad, report, clients, rules)


def _table_block(args, ctx, train, data, tdata, bad, report, clients, rules):
    from ddl25spring_amd.data.split import split
    from ddl25spring_amd.fl.algorithms import FedAvg
    from ddl25spring_amd.fl.attacks import make_attack
    from ddl25spring_amd.models import mnist_cnn
    parts = split(clients, True, args.seed, labels=train.labels)

    def fed(rule, attack, **agg_kw):
        atk = None if attack == "clean" else make_attack(attack, bad, **({"eps": args.eps} if attack == "ipm" else {}))
        return FedAvg(lambda groups: mnist_cnn(groups=groups, precision=args.precision), data, parts, lr=args.lr,
                      batch_size=args.batch_size, client_fraction=args.client_fraction, seed=args.seed,
                      test_data=tdata, ctx=ctx, eval_every=0, aggregator=rule, attack=atk, agg_kwargs=agg_kw)

    # the clipping radius: the median update norm of the first clean round
    probe = fed("clipped", "clean", clip=1e30)
    probe.round()
    norms = sorted(round(v, 5) for v in probe.aggregator.last_norms)
    tau = args.tau if args.tau > 0 else float(statistics.median(norms))
    del probe
    kw = {"mean": {}, "median": {}, "trimmed_mean": {"trim": args.attackers / clients}, "krum": {"f": args.attackers},
          "clipped": {"clip": tau}, "centered_clip": {"tau": tau, "iters": args.cc_iters},
          "geomed": {"gm_iters": args.gm_iters}, "bulyan": {"f": args.attackers}}
    results = {}
    for rule in rules:
        results[rule] = {}
        for attack in ATTACKS:
            fa = fed(rule, attack, **kw[rule])
            acc = {}
            for r in range(1, max(report) + 1):
                fa.round()
                if r in report:
                    acc[f"round_{r}"] = round(fa.test(), 2)
            results[rule][attack] = acc
            del fa
    emit(ctx, metric="colluding attacks against the aggregation rules, test accuracy (MnistCnn, synthetic MNIST shape)",
         unit="%", n_gpus=ctx.world, clients=clients, client_fraction=args.client_fraction, attackers=args.attackers,
         batch_size=args.batch_size, lr=args.lr, seed=args.seed, dtype=args.precision, data="synthetic", ipm_eps=args.eps,
         alie_z="z_max", tau=round(tau, 5), cc_iters=args.cc_iters, gm_iters=args.gm_iters, first_round_clean_norms=norms, results=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agg", action="store_true", help="time the kernels alone")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the one-pass time (MI355X spec: 8 TB/s)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--P", type=int, default=0, help="row length (default: ResNet-18's padded row, 11.2M)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cc-iters", type=int, default=3)
    ap.add_argument("--gm-iters", type=int, default=3)
    ap.add_argument("--bulyan-clients", type=int, default=16, help="clients of the second block, with Bulyan (0: none)")
    ap.add_argument("--rules", default=",".join(RULES))
    ap.add_argument("--report", default="5,10", help="rounds after which the accuracy is reported")
    ap.add_argument("--clients", type=int, default=10)
    ap.add_argument("--client-fraction", type=float, default=1.0)
    ap.add_argument("--attackers", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.5, help="IPM's eps")
    ap.add_argument("--tau", type=float, default=0.0, help="clipping radius (default: the median first-round norm)")
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.05)
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
        bench_table(args, ctx)
    rdist.shutdown()


if __name__ == "__main__":
    main()
