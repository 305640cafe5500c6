"""Horizontal FL experiment runner (reference hfl_complete.py __main__ / homework-1 sweeps).

One process per GPU (or CPU/gloo ranks); the FL round protocol, client sampling and RunResult
table are the reference's; the model, aggregator, attack and failures are configurable.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class FLConfig:
    algorithm: str = "fedavg"      # fedavg | fedsgd | fedsgd_weight | scaffold
    model: str = "mnist_cnn"       # mnist_cnn | mnist_mlp | resnet18 | resnet50
    dataset: str = "mnist"         # mnist | cifar10 | imagenet (real copy via DDL_DATA_ROOT, else synthetic)
    clients: int = 100
    client_fraction: float = 0.1
    batch_size: int = 100          # -1 = infinity (full local batch)
    local_epochs: int = 1
    lr: float = 0.01
    rounds: int = 10
    iid: bool = True
    seed: int = 10
    aggregator: str = "mean"       # mean | median | trimmed_mean | krum | multi_krum | bulyan | clipped | centered_clip | geomed | secagg | rlr
    trim: float = 0.1
    krum_f: int = 1                # krum / multi_krum / bulyan: the Byzantine clients assumed
    clip_norm: float | None = None  # clipped / secagg / rlr: L2 bound C on every client update (default: 1.0 / none / none)
    noise_multiplier: float = 0.0  # clipped: DP-FedAvg noise std = z * C / K (needs uniform weighting)
    agg_weighting: str = "samples"  # clipped / centered_clip / geomed: samples (n_k / n) | uniform (1 / K)
    dp_delta: float = 1e-5         # the delta of the epsilon reported per round when noise is on
    cc_tau: float = 1.0            # centered_clip: the clipping radius around the carried aggregate
    cc_iters: int = 3              # centered_clip: clipping iterations per round
    gm_iters: int = 3              # geomed: smoothed Weiszfeld iterations per round
    gm_nu: float = 1e-6            # geomed: the floor of a distance in the weights a_k / max(nu, d_k)
    rlr_theta: float = 0.0         # rlr: a coordinate on which fewer than theta clients (net) agree is flipped
    secagg_bits: int = 20          # secagg: fractional bits of the fixed-point uploads, 8..30
    secagg_min_survivors: int = 2  # secagg: a round with fewer reporting clients is aborted
    prox_mu: float = 0.0           # FedProx: mu of the proximal term mu/2 |w - w_global|^2 (0 = off)
    server_opt: str | None = None  # FedOpt server optimizer: fedavgm | fedadagrad | fedadam | fedyogi
    server_lr: float | None = None  # its step size (default 1.0 for fedavgm, 0.01 for the adaptive ones)
    server_beta1: float = 0.9
    server_beta2: float = 0.99
    server_tau: float = 1e-3       # adaptivity floor of fedadagrad / fedadam / fedyogi
    compress: str | None = None    # compressed uploads: topk | quant (fl/compress.py; None = dense)
    compress_ratio: float = 0.1    # topk: fraction of the coordinates every client sends
    compress_bits: int = 4         # quant: bits per coordinate, 2..8
    error_feedback: bool = True    # keep what the codec dropped per client and add it back next round
    attack: str | None = None      # label_flip | sign_flip | gaussian | free_rider | alie | ipm | backdoor
    attack_z: float | None = None  # alie: z of mu - z * sigma (default: z_max of the round's n and f)
    attack_eps: float = 0.5        # ipm: eps of -eps * mu
    attack_knowledge: str = "benign"  # alie / ipm: statistics over the benign rows | the colluders' own
    backdoor_target: int = 0       # backdoor: the class every triggered input should go to
    backdoor_fraction: float = 0.5  # backdoor: share of a malicious client's samples replaced by triggered copies
    backdoor_patch: int = 4        # backdoor: side of the trigger square in the bottom-right corner
    backdoor_boost: float = 1.0    # backdoor: model replacement, the malicious update scaled by this
    malicious: int = 0             # number of malicious clients (ids 0..malicious-1)
    dropout: float = 0.0
    stragglers: float = 0.0        # probability a sampled client is slow
    straggler_slowdown: float = 4.0
    deadline: float | None = None  # drop clients slower than this (x nominal mean-shard time)
    train_size: int | None = None
    test_size: int | None = None
    checkpoint: str | None = None
    jsonl: str | None = None


def build_server(cfg: FLConfig, ctx):
    from ..data.images import DeviceImageDataset, load_images
    from ..data.split import split
    from ..fl.algorithms import FedAvg, FedSGD, FedSgdWeight, Scaffold
    from ..fl.attacks import make_attack
    from ..models import mnist_cnn, mnist_mlp, resnet18_cifar, resnet50_imagenet
    train = load_images(cfg.dataset, True, cfg.train_size, seed=cfg.seed)
    test = load_images(cfg.dataset, False, cfg.test_size, seed=cfg.seed)
    parts = split(cfg.clients, cfg.iid, cfg.seed, labels=train.labels)
    model_fn = {"mnist_cnn": mnist_cnn, "mnist_mlp": mnist_mlp, "resnet18": resnet18_cifar,
                "resnet50": resnet50_imagenet}[cfg.model]
    akw = {}  # keyword arguments only for the colluding attacks
    if cfg.attack == "alie":
        akw = {"z": cfg.attack_z, "knowledge": cfg.attack_knowledge}
    elif cfg.attack == "ipm":
        akw = {"eps": cfg.attack_eps, "knowledge": cfg.attack_knowledge}
    elif cfg.attack == "backdoor":
        akw = {"target": cfg.backdoor_target, "poison_fraction": cfg.backdoor_fraction, "patch": cfg.backdoor_patch,
               "boost": cfg.backdoor_boost, "seed": cfg.seed}
    attack = make_attack(cfg.attack, list(range(cfg.malicious)), **akw) if cfg.attack else None
    backdoor_test = None
    if cfg.attack == "backdoor":  # the data is poisoned here, on the host, identically on every rank
        train, parts = attack.poison(train, parts)
        backdoor_test = DeviceImageDataset(attack.triggered_test(test), ctx.device)
    algo = {"fedavg": FedAvg, "fedsgd": FedSGD, "fedsgd_weight": FedSgdWeight,
            "scaffold": Scaffold}[cfg.algorithm]
    secure = cfg.aggregator.lower() in ("secagg", "secure", "secure_mean")
    rlr = cfg.aggregator.lower() in ("rlr", "robust_lr")
    # without --clip-norm: the clipped mean bounds at 1.0, secure aggregation and rlr do not clip
    clip = cfg.clip_norm if cfg.clip_norm is not None else (float("inf") if secure or rlr else 1.0)
    kw = dict(lr=cfg.lr, client_fraction=cfg.client_fraction, seed=cfg.seed,
              test_data=DeviceImageDataset(test, ctx.device), aggregator=cfg.aggregator,
              agg_kwargs={"trim": cfg.trim, "f": cfg.krum_f, "clip": clip, "frac_bits": cfg.secagg_bits,
                          "min_survivors": cfg.secagg_min_survivors,
                          "noise_multiplier": cfg.noise_multiplier, "seed": cfg.seed,
                          "weighting": cfg.agg_weighting, "tau": cfg.cc_tau, "iters": cfg.cc_iters,
                          "gm_iters": cfg.gm_iters, "gm_nu": cfg.gm_nu, "theta": cfg.rlr_theta},
              attack=attack, ctx=ctx, backdoor_test=backdoor_test,
              dropout=cfg.dropout, stragglers=cfg.stragglers,
              straggler_slowdown=cfg.straggler_slowdown, deadline=cfg.deadline, prox_mu=cfg.prox_mu)
    if cfg.server_opt:
        so = {"beta1": cfg.server_beta1, "beta2": cfg.server_beta2, "tau": cfg.server_tau}
        if cfg.server_lr is not None:
            so["lr"] = cfg.server_lr
        kw.update(server_opt=cfg.server_opt, server_opt_kwargs=so)
    if cfg.compress:
        if cfg.compress not in ("topk", "quant"):
            raise ValueError(f"compress must be topk or quant, got {cfg.compress!r}")
        ck = {"ratio": cfg.compress_ratio} if cfg.compress == "topk" else {"bits": cfg.compress_bits, "seed": cfg.seed}
        kw.update(compressor=cfg.compress, compressor_kwargs={**ck, "error_feedback": cfg.error_feedback})
    if algo in (FedAvg, Scaffold):
        kw.update(batch_size=cfg.batch_size, local_epochs=cfg.local_epochs)
    return algo(model_fn, DeviceImageDataset(train, ctx.device), parts, **kw)


def run_fl(cfg: FLConfig, ctx, log=print):
    from ..fl import checkpoint as ckpt
    from ..fl import privacy
    from ..utils.metrics import JsonlLogger
    server = build_server(cfg, ctx)
    noisy = cfg.noise_multiplier > 0 and getattr(server.aggregator, "takes_center", False)
    if cfg.checkpoint:
        res = ckpt.run_with_checkpoints(server, cfg.rounds, cfg.checkpoint)
    else:
        res = server.run(cfg.rounds)
    up = server.uplink_bytes if server.compressor is not None else None
    secure = getattr(server.aggregator, "name", None) == "secagg"
    with JsonlLogger(cfg.jsonl, ctx.rank) as jl:
        for i in range(len(res.test_accuracy)):
            rec = dict(round=i + 1, test_accuracy=res.test_accuracy[i],
                       message_count=res.message_count[i])
            if i < len(res.round_time):
                rec.update(round_time=res.round_time[i], samples=res.samples[i],
                           samples_per_s=res.samples[i] / max(res.round_time[i], 1e-9))
            if i < len(res.phase_ms):
                rec["phase_ms"] = res.phase_ms[i]
            if noisy:  # (epsilon, dp_delta)-DP spent after this round (fl/privacy.py, q = K / N)
                rec["epsilon"] = privacy.epsilon(i + 1, server.K / server.N, cfg.noise_multiplier, cfg.dp_delta)
            if up is not None and i < len(up):  # bytes the round's reporting clients sent up
                rec["uplink_bytes"] = up[i]
            if i < len(res.backdoor_accuracy):  # the attack success rate on the triggered test set
                rec["backdoor_accuracy"] = res.backdoor_accuracy[i]
            if secure:  # host-known: the sampled clients, those that reported, whether the server opened
                gone = sum(len(lst[i]) for lst in (server.dropped, server.straggled) if i < len(lst))
                rec.update(secagg_cohort=server.K, secagg_survivors=server.K - gone,
                           secagg_aborted=i in server.aggregator.aborted)
            jl.log(**rec)
    if log and ctx.rank == 0:
        log(res.as_df(with_throughput=True).to_string(index=False))
        if np.isfinite(res.test_accuracy[-1]):
            log(f"final test accuracy {res.test_accuracy[-1]:.2f}%")
    return res
