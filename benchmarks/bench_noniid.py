"""Non-IID FedAvg and its standard remedies: FedProx local steps, FedOpt server optimizers and
SCAFFOLD's control variates.

The pathological non-IID split (two label shards per client, ``data.split.split(N, False, seed)``)
of the learnable synthetic MNIST-shaped set; FedAvg, FedProx, FedAvgM, FedAdam and SCAFFOLD from the
same initial model, clients and seeds. Per method: test accuracy after every round and rounds/s (the
evaluation is outside the timed span).

``--agg`` instead times the server step alone for ``--K`` x ``--P`` client rows (default 8 x 11.2M,
ResNet-18's size) with HIP events: the plain weighted mean, the mean followed by the unfused server
step (two launches, (K + 8) P floats moved), and the fused kernel (one launch, (K + 6) P floats).
The three are alternated ``--reps`` times in one session and the median of the repetitions is
reported, so that clock and thermal drift hit all three alike.

``--control`` times SCAFFOLD's round-end update (``scaffold_finish``, one launch, (3K + 3) P floats:
the K trained rows read, K bank rows read and written, x and c read, dc written) for the same
``--K`` x ``--P`` rows, alternated with the plain weighted mean in the same way, next to the time one
pass over its bytes takes at the HBM rate ``--hbm-tbs``.

    python benchmarks/bench_noniid.py [--rounds 10] [--clients 10] [--precision fp32]
    python benchmarks/bench_noniid.py --agg [--K 8] [--P 0] [--iters 20] [--reps 5]
    python benchmarks/bench_noniid.py --control [--K 8] [--P 0] [--clients 16] [--iters 20] [--reps 5]
"""
from __future__ import annotations

import argparse
import statistics
import time

import torch

from _common import emit

METHODS = {
    "fedavg": dict(),
    "fedprox": dict(prox_mu=0.1),
    "fedavgm": dict(server_opt="fedavgm", server_opt_kwargs=dict(lr=1.0, beta1=0.9)),
    "fedadam": dict(server_opt="fedadam", server_opt_kwargs=dict(lr=0.003, tau=1e-3)),
    "scaffold": dict(algorithm="scaffold"),
}


def _timed(calls: dict, iters: int, reps: int) -> dict:
    """Median ms per call of each entry, the entries alternated ``reps`` times (``--agg``'s method)."""
    times = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(3):
            f()
    for _ in range(reps):
        for name, f in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(iters):
                f()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def bench_control(args, ctx):
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P, N = args.K, args.P, max(args.clients, args.K)
    if P <= 0:
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    x = torch.randn(P, device=dev)
    rows = x + torch.randn(K, P, device=dev) * 0.01
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    tmp, dc = torch.empty(P, device=dev), torch.empty(P, device=dev)
    c, bank = torch.zeros(P, device=dev), torch.zeros(N, P, device=dev)
    ids = Fn.check_slot_clients([N - 1 - g for g in range(K)], N)  # not the identity
    slots = torch.tensor(ids, dtype=torch.int32, device=dev)
    inv_klr = torch.full((K,), 1.0 / (63 * 0.05), device=dev)
    calls = {"mean_ms": lambda: Fn.weighted_sum(rows, coeffs, tmp),
             "scaffold_finish_ms": lambda: Fn.scaffold_finish(rows, x, c, bank, slots, inv_klr, 1.0 / N, dc, False)}
    res = _timed(calls, args.iters, args.reps)
    nbytes = (3 * K + 3) * P * 4
    res.update(K=K, P=P, clients=N, iters=args.iters, reps=args.reps, floats_moved_mean=(K + 1) * P,
               floats_moved_finish=(3 * K + 3) * P, hbm_tbs=args.hbm_tbs,
               finish_one_pass_hbm_ms=round(nbytes / (args.hbm_tbs * 1e12) * 1e3, 4),
               finish_gbs=round(nbytes / (res["scaffold_finish_ms"] * 1e-3) / 1e9, 1))
    emit(ctx, metric=f"SCAFFOLD round-end update over {K} x {P} client rows", unit="ms", **res)


def bench_agg(args, ctx):
    from ddl25spring_amd.fl.server_opt import ServerOptimizer
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P = args.K, args.P
    if P <= 0:  # ResNet-18's flat parameter row as the FL loop holds it (every tensor padded to 16
        # floats, so the rows start 16-B aligned and the kernels take their 16-B path)
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    rows = torch.randn(K, P, device=dev) * 0.01
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    w = torch.zeros(P, device=dev)
    tmp = torch.empty(P, device=dev)
    res = {"K": K, "P": P, "iters": args.iters, "reps": args.reps}
    for kind in args.kinds.split(","):
        fused, unfused = ServerOptimizer(kind, 0.01), ServerOptimizer(kind, 0.01)
        wf, wu = w.clone(), w.clone()

        def mean():
            Fn.weighted_sum(rows, coeffs, tmp)

        def pair():
            Fn.weighted_sum(rows, coeffs, tmp)
            unfused.step(wu, tmp, False)

        def one():
            fused.step_rows(rows, coeffs, wf)

        res[kind] = _timed({"mean_ms": mean, "mean_plus_server_step_ms": pair, "fused_ms": one},
                           args.iters, args.reps)
        assert torch.equal(wf, wu), "fused and unfused server steps diverged"
        nv = 0 if kind == "sgdm" else 2  # sgdm has no v row
        res[kind]["floats_moved_unfused"] = (K + 6 + nv) * P
        res[kind]["floats_moved_fused"] = (K + 4 + nv) * P
    emit(ctx, metric=f"server step over {K} x {P} client rows", unit="ms", **res)


def bench_methods(args, ctx):
    from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
    from ddl25spring_amd.data.split import split
    from ddl25spring_amd.fl.algorithms import FedAvg, Scaffold
    from ddl25spring_amd.models import mnist_cnn
    train = synthetic_images("mnist", args.train_size, seed=0)
    test = synthetic_images("mnist", args.test_size, seed=1)
    parts = split(args.clients, False, args.seed, labels=train.labels)
    data, tdata = DeviceImageDataset(train, ctx.device), DeviceImageDataset(test, ctx.device)
    results = {}
    for name in args.methods.split(","):
        kw = dict(METHODS[name])
        algo = {"fedavg": FedAvg, "scaffold": Scaffold}[kw.pop("algorithm", "fedavg")]
        fa = algo(lambda groups: mnist_cnn(groups=groups, precision=args.precision), data, parts,
                  lr=args.lr, batch_size=args.batch_size, client_fraction=args.client_fraction,
                  seed=args.seed, test_data=tdata, ctx=ctx, eval_every=0, **kw)
        acc, spent = [], []
        for _ in range(args.rounds):
            if ctx.device.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fa.round()
            if ctx.device.type == "cuda":
                torch.cuda.synchronize()
            spent.append(time.perf_counter() - t0)
            acc.append(round(fa.test(), 2))
        # the first rounds capture the round graphs (one per set of sampled shard sizes): rounds/s
        # from the median round
        results[name] = {"test_accuracy": acc, "rounds_per_s": round(1.0 / statistics.median(spent), 3)}
        del fa
    emit(ctx, metric="non-IID FedAvg remedies, test accuracy per round (MnistCnn, synthetic MNIST shape)",
         unit="%", n_gpus=ctx.world, rounds=args.rounds, clients=args.clients,
         client_fraction=args.client_fraction, batch_size=args.batch_size, lr=args.lr, dtype=args.precision,
         data="synthetic", split="non-iid, 2 label shards per client", methods=METHODS, results=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agg", action="store_true", help="time the server step alone")
    ap.add_argument("--control", action="store_true", help="time SCAFFOLD's round-end update alone")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the one-pass time (MI355X spec: 8 TB/s)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--P", type=int, default=0, help="row length (default: ResNet-18's padded row, 11.2M)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kinds", default="sgdm,adam,yogi")
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--clients", type=int, default=10)
    ap.add_argument("--client-fraction", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--train-size", type=int, default=3000)
    ap.add_argument("--test-size", type=int, default=1000)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init()
    if args.agg or args.control:
        if ctx.device.type != "cuda":
            raise SystemExit("--agg / --control time the HIP kernels: they need a GPU")
        (bench_agg if args.agg else bench_control)(args, ctx)
    else:
        bench_methods(args, ctx)
    rdist.shutdown()


if __name__ == "__main__":
    main()
