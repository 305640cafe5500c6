"""Compressed client uploads: accuracy against uplink bytes, and the codecs' own time.

Without ``--codec``: the 10-client MnistCnn setting of bench_noniid.py (learnable synthetic
MNIST-shaped set, C = 0.5, B = 50, lr 0.05; IID split by default, ``--iid false`` for the two-shard
split), FedAvg from the same initial model, clients and seeds with dense uploads, top-k 0.1 and 0.01
with and without error feedback, and 4- and 2-bit quantization. Per method: test accuracy after
every round and the cumulative uplink bytes.

``--codec`` times each codec alone over ``--K`` x ``--P`` client rows (default 8 x 11.2M, ResNet-18's
size) with HIP events, alternated ``--reps`` times in one session with the plain weighted mean and
with SCAFFOLD's round-end update (``scaffold_finish``); the median of the repetitions is reported,
next to the floats each codec moves and the time one pass over its bytes takes at the HBM rate
``--hbm-tbs``. The codecs work in place, so every timed call starts from the same trained rows and
error bank, restored outside the timed span.

    python benchmarks/bench_compress.py [--rounds 10] [--iid true]
    python benchmarks/bench_compress.py --codec [--K 8] [--P 0] [--iters 10] [--reps 5]
"""
from __future__ import annotations

import argparse
import statistics

import torch

from _common import emit

METHODS = {
    "dense": None,
    "topk0.1_ef": ("topk", dict(ratio=0.1)),
    "topk0.1": ("topk", dict(ratio=0.1, error_feedback=False)),
    "topk0.01_ef": ("topk", dict(ratio=0.01)),
    "topk0.01": ("topk", dict(ratio=0.01, error_feedback=False)),
    "quant4": ("quant", dict(bits=4)),
    "quant2": ("quant", dict(bits=2)),
}


def _timed(calls: dict, restore, iters: int, reps: int) -> dict:
    """Median ms per call of each entry; the entries alternated ``reps`` times, ``restore()`` run
    before every call and outside its events."""
    times = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(2):
            restore()
            f()
    for _ in range(reps):
        for name, f in calls.items():
            evs = []
            for _ in range(iters):
                restore()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                evs.append((s, e))
            torch.cuda.synchronize()
            times[name].append(sum(s.elapsed_time(e) for s, e in evs) / iters)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def bench_codec(args, ctx):
    from ddl25spring_amd.ops import functional as Fn
    dev = ctx.device
    K, P, N = args.K, args.P, max(args.clients, args.K)
    if P <= 0:
        from ddl25spring_amd import models
        P = int(models.resnet18_cifar(10, groups=1).to("cpu", seed=0).store.data.shape[1])
    x = torch.randn(P, device=dev)
    rows0 = x + torch.randn(K, P, device=dev) * 0.01
    bank0 = torch.randn(N, P, device=dev) * 0.003
    rows, bank = rows0.clone(), bank0.clone()
    ids = Fn.check_slot_clients([N - 1 - g for g in range(K)], N)  # not the identity
    slots = torch.tensor(ids, dtype=torch.int32, device=dev)
    coeffs = torch.full((K,), 1.0 / K, device=dev)
    tmp, dc, c = torch.empty(P, device=dev), torch.empty(P, device=dev), torch.zeros(P, device=dev)
    inv_klr = torch.full((K,), 1.0 / (63 * 0.05), device=dev)
    nnz = torch.zeros(K, dtype=torch.int32, device=dev)

    def restore():
        rows.copy_(rows0)
        bank.copy_(bank0)

    calls = {"mean_ms": lambda: Fn.weighted_sum(rows, coeffs, tmp),
             "scaffold_finish_ms": lambda: Fn.scaffold_finish(rows, x, c, bank, slots, inv_klr, 1.0 / N, dc, False),
             "topk0.1_ms": lambda: Fn.topk_compress(rows, x, bank, slots, max(1, round(0.1 * P)), nnz),
             "topk0.01_ms": lambda: Fn.topk_compress(rows, x, bank, slots, max(1, round(0.01 * P)), nnz),
             "topk0.01_nobank_ms": lambda: Fn.topk_compress(rows, x, None, None, max(1, round(0.01 * P)), nnz),
             "quant4_ms": lambda: Fn.quantize_compress(rows, x, bank, slots, 4, 7, 1),
             "quant2_ms": lambda: Fn.quantize_compress(rows, x, bank, slots, 2, 7, 1)}
    res = _timed(calls, restore, args.iters, args.reps)
    # floats per row and pass: form 4 (y, x, e read; u written), two digit passes 1 each (u read),
    # apply 4 (u, x read; row, bank written); the quantizer's one pass 5 (y, x, e read; row, bank written)
    moved = {"topk": 10 * K * P, "topk_nobank": 8 * K * P, "quant": 5 * K * P, "finish": (3 * K + 3) * P,
             "mean": (K + 1) * P}
    hbm = {f"{k}_one_pass_hbm_ms": round(v * 4 / (args.hbm_tbs * 1e12) * 1e3, 4) for k, v in moved.items()}
    res.update(K=K, P=P, clients=N, iters=args.iters, reps=args.reps, hbm_tbs=args.hbm_tbs,
               floats_moved=moved, **hbm, nnz_last=nnz.cpu().tolist())
    emit(ctx, metric=f"upload codecs over {K} x {P} client rows", unit="ms", **res)


def bench_methods(args, ctx):
    from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
    from ddl25spring_amd.data.split import split
    from ddl25spring_amd.fl.algorithms import FedAvg
    from ddl25spring_amd.fl.compress import dense_bytes
    from ddl25spring_amd.models import mnist_cnn
    train = synthetic_images("mnist", args.train_size, seed=0)
    test = synthetic_images("mnist", args.test_size, seed=1)
    parts = split(args.clients, args.iid, args.seed, labels=train.labels)
    data, tdata = DeviceImageDataset(train, ctx.device), DeviceImageDataset(test, ctx.device)
    results = {}
    for name in args.methods.split(","):
        kw = {}
        if METHODS[name] is not None:
            codec, ck = METHODS[name]
            kw = dict(compressor=codec, compressor_kwargs=dict(ck, **({"seed": args.seed} if codec == "quant" else {})))
        fa = FedAvg(lambda groups: mnist_cnn(groups=groups, precision=args.precision), data, parts,
                    lr=args.lr, batch_size=args.batch_size, client_fraction=args.client_fraction,
                    seed=args.seed, test_data=tdata, ctx=ctx, eval_every=0, **kw)
        acc = []
        for _ in range(args.rounds):
            fa.round()
            acc.append(round(fa.test(), 2))
        P = fa.w_global.numel()
        up = fa.uplink_bytes if fa.compressor is not None else \
            [fa.K * (dense_bytes(P) + 4 * fa.b_global.numel())] * args.rounds
        results[name] = {"test_accuracy": acc, "uplink_mbytes_cumulative": [round(sum(up[:i + 1]) / 1e6, 3)
                                                                             for i in range(len(up))]}
        del fa
    emit(ctx, metric="compressed uploads, test accuracy per round against cumulative uplink bytes "
         "(MnistCnn, synthetic MNIST shape)", unit="%", n_gpus=ctx.world, rounds=args.rounds, clients=args.clients,
         client_fraction=args.client_fraction, batch_size=args.batch_size, lr=args.lr, dtype=args.precision,
         data="synthetic", split="iid" if args.iid else "non-iid, 2 label shards per client", results=results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codec", action="store_true", help="time the codecs alone")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the one-pass time (MI355X spec: 8 TB/s)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--P", type=int, default=0, help="row length (default: ResNet-18's padded row, 11.2M)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--clients", type=int, default=10)
    ap.add_argument("--client-fraction", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--iid", type=lambda v: v.lower() in ("1", "true", "yes"), default=True)
    ap.add_argument("--train-size", type=int, default=3000)
    ap.add_argument("--test-size", type=int, default=1000)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    args = ap.parse_args()
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init()
    if args.codec:
        if ctx.device.type != "cuda":
            raise SystemExit("--codec times the HIP kernels: it needs a GPU")
        bench_codec(args, ctx)
    else:
        bench_methods(args, ctx)
    rdist.shutdown()


if __name__ == "__main__":
    main()
