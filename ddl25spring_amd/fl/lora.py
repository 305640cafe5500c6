"""Federated LoRA fine-tuning of the LLaMA (FedIT, Zhang et al. 2023; FFA-LoRA, Sun et al. 2024).

One frozen base model lives on the device; each of ``slots`` resident clients owns a low-rank adapter
(models/lora.py) and the clients of a wave train together: one forward + CE + backward over the
slot-major batch, one ``SlotAdam`` launch. A client's upload is its row of the optimizer's
``[S, P]`` buffer, and the round's ``[K, P]`` rows go through any rule of ``fl/aggregate.py``.

Round protocol (the engine's conventions, fl/algorithms.py):
  * ``K = max(1, round(C N))`` clients from ``numpy.default_rng(seed).choice(N, K, replace=False)``;
  * waves of ``slots`` clients: the global row broadcast into the slots, the optimizer state reset
    (clients are stateless between rounds), ``local_steps`` Adam steps, the rows kept;
  * ``aggregate_into(agg, ctx, rows, coeffs, global, center=global, ...)`` with equal weights
    (every client trains on the same number of tokens).

Client i reads the token stream of grammar ``dialect_seed + i % dialects`` (``dialects = 1``: IID),
its own block of sequence indices; the held-out sequences of every grammar lie in a block no client
reaches. Averaging A and B separately is not averaging B A: with ``report_gap`` every round also
records the relative distance between the mean of the clients' B A and the aggregate's B A, and the
held-out loss of the model merged with that mean. ``lora_freeze_a`` makes the two coincide.

One process only; attacks, codecs, SCAFFOLD, FedOpt and FLTrust's server root are out of scope.
"""
from __future__ import annotations

import dataclasses
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from ..data.text import SPTokenizer, TinyStories
from ..models.llama import LLama, causalLLMLoss
from ..models.lora import LoRAConfig, attach_lora, merge_lora, merged_weight, unmerge_lora
from ..runtime import dist as rdist
from .aggregate import aggregate_into, make_aggregator

CLIENT_SPAN = 1 << 20   # sequence indices reserved per client of a grammar
HELDOUT_START = 1 << 40  # the held-out block of every grammar: beyond any client's span
SAMPLE_ADAPTERS = ("global", "clients")
SAMPLE_CHUNK = 16        # sequences per generate call of the "clients" samples: the skinny decode path


@dataclass
class FedLoRAConfig:
    # the model
    vocab_size: int = 32000
    dmodel: int = 288
    num_heads: int = 6
    n_layers: int = 6
    ctx_size: int = 256
    # the federation
    clients: int = 8
    client_fraction: float = 1.0
    slots: int = 8                 # clients resident on the device at once (a wave)
    local_steps: int = 4           # Adam steps per client per round
    batch_size: int = 4            # sequences per client per step
    lr: float = 1e-3
    rounds: int = 3
    # the adapters
    lora_rank: int = 8
    lora_alpha: float = 16.0
    lora_freeze_a: bool = False    # FFA-LoRA: A stays at its shared initialisation
    # the data
    dialects: int = 1              # 1: IID; more: client i reads grammar dialect_seed + i % dialects
    dialect_seed: int = 2000
    sub_vocab: int = 2048
    branching: int = 8
    eval_batches: int = 2          # held-out batches (of batch_size sequences) per grammar
    report_gap: bool = False       # mean(B A) against the aggregate's B A, and the mean's held-out loss
    # the aggregator (as FLConfig's)
    aggregator: str = "mean"
    trim: float = 0.1
    krum_f: int = 1
    clip_norm: float | None = None
    noise_multiplier: float = 0.0
    agg_weighting: str = "samples"
    cc_tau: float = 1.0
    cc_iters: int = 3
    gm_iters: int = 3
    gm_nu: float = 1e-6
    rlr_theta: float = 0.0
    # the base model: pretrained in-process on the default grammar, and / or loaded from a file
    pretrain_iters: int = 0
    pretrain_lr: float = 3e-3
    pretrain_batch: int = 8
    pretrain_seed: int = 1234
    base_ckpt: str | None = None
    # after the last round: continue held-out prompts with the merged model
    sample_tokens: int = 0
    sample_prompt_len: int = 8
    # "global": the merged global adapter on every grammar's prompts; "clients": for each client of the
    # last round one held-out prompt of its grammar under the base, the global and the client's own
    # adapter, batched through per-sequence adapters (nothing is merged)
    sample_adapters: str = "global"
    jsonl: str | None = None
    checkpoint: str | None = None
    seed: int = 0


@dataclass
class FedLoRAResult:
    """A ``RunResult``-style record: one entry per evaluation, the first being round 0 (the base)."""
    algorithm: str
    n: int
    c: float
    b: int
    e: int  # local steps
    lr: float
    seed: int
    round: list[int] = field(default_factory=list)
    heldout_loss: list[list[float]] = field(default_factory=list)  # [evaluation][dialect]
    gap: list[float] = field(default_factory=list)                 # per trained round (report_gap)
    mean_merged_loss: list[list[float]] = field(default_factory=list)
    round_time: list[float] = field(default_factory=list, repr=False)
    tokens: list[int] = field(default_factory=list, repr=False)
    message_count: list[int] = field(default_factory=list)
    samples: list = field(default_factory=list, repr=False)


def _model_kw(cfg):
    return dict(vocab_size=cfg.vocab_size, dmodel=cfg.dmodel, num_heads=cfg.num_heads, n_layers=cfg.n_layers,
                ctx_size=cfg.ctx_size)


def pretrain_base(model, cfg: FedLoRAConfig, dev, log=None) -> float:
    """``cfg.pretrain_iters`` Adam steps on the default grammar (``pretrain_seed``) -> the last loss."""
    from ..optim import make_adam
    ds = TinyStories(SPTokenizer(cfg.vocab_size), cfg.pretrain_batch, cfg.ctx_size, seed=cfg.pretrain_seed,
                     sub_vocab=cfg.sub_vocab, branching=cfg.branching)
    opt = make_adam(model.parameters(), lr=cfg.pretrain_lr)
    last = float("nan")
    for it in range(cfg.pretrain_iters):
        x = torch.from_numpy(ds.batch(it * cfg.pretrain_batch)).to(dev)
        opt.zero_grad()
        loss = causalLLMLoss(model(x), x)
        loss.backward()
        opt.step()
        if log and (it % 50 == 0 or it == cfg.pretrain_iters - 1):
            last = float(loss)
            log(f"[fedlora] pretrain iter {it} loss {last:.4f}")
    return last


def build_base(cfg: FedLoRAConfig, dev, log=None):
    """The seeded base model: loaded from ``base_ckpt`` when the file exists, else pretrained for
    ``pretrain_iters`` steps (and written to ``base_ckpt`` when one is named)."""
    torch.manual_seed(cfg.seed)
    model = LLama(**_model_kw(cfg)).to(dev)
    if cfg.base_ckpt and os.path.exists(cfg.base_ckpt):
        model.load_state_dict(torch.load(cfg.base_ckpt, map_location="cpu", weights_only=True))
    else:
        if cfg.pretrain_iters > 0:
            pretrain_base(model, cfg, dev, log)
        if cfg.base_ckpt:
            tmp = f"{cfg.base_ckpt}.tmp"
            torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, tmp)
            os.replace(tmp, cfg.base_ckpt)
    return model


class FedLoRA:
    def __init__(self, cfg: FedLoRAConfig, ctx=None, model=None, log=None):
        self.cfg, self.log = cfg, log
        self.ctx = ctx or rdist.context()
        if self.ctx.world > 1:
            raise NotImplementedError(f"fedlora runs in one process (world = {self.ctx.world}): the clients are "
                                      "batched over the slots of one device")
        if cfg.slots < 1 or cfg.clients < 1 or cfg.local_steps < 1 or cfg.batch_size < 1 or cfg.dialects < 1:
            raise ValueError("fedlora: clients, slots, local_steps, batch_size and dialects must be at least 1")
        if cfg.dialects > cfg.clients:
            raise ValueError(f"fedlora: {cfg.dialects} dialects for {cfg.clients} clients")
        if cfg.sample_adapters not in SAMPLE_ADAPTERS:
            raise ValueError(f"fedlora: sample_adapters {cfg.sample_adapters!r} not in {SAMPLE_ADAPTERS}")
        self.dev = self.ctx.device
        self.N, self.C = cfg.clients, cfg.client_fraction
        self.K = max(1, round(cfg.client_fraction * self.N))
        self.S = min(cfg.slots, self.K)
        rlr = cfg.aggregator.lower() in ("rlr", "robust_lr")
        clip = cfg.clip_norm if cfg.clip_norm is not None else (float("inf") if rlr else 1.0)
        self.aggregator = make_aggregator(cfg.aggregator, trim=cfg.trim, f=cfg.krum_f, clip=clip,
                                          noise_multiplier=cfg.noise_multiplier, seed=cfg.seed,
                                          weighting=cfg.agg_weighting, tau=cfg.cc_tau, iters=cfg.cc_iters,
                                          gm_iters=cfg.gm_iters, gm_nu=cfg.gm_nu, theta=cfg.rlr_theta)
        if getattr(self.aggregator, "needs_root", False):
            raise ValueError(f"fedlora: aggregator {cfg.aggregator!r} needs a server root update, which this "
                             "engine does not train")
        if hasattr(self.aggregator, "begin_round"):
            raise ValueError(f"fedlora: aggregator {cfg.aggregator!r} needs the cohort protocol of the image engine")
        self.model = model if model is not None else build_base(cfg, self.dev, log)
        self.lcfg = LoRAConfig(rank=cfg.lora_rank, alpha=cfg.lora_alpha, freeze_a=cfg.lora_freeze_a)
        self.adapters = attach_lora(self.model, self.S, self.lcfg, seed=cfg.seed)
        self.opt = self.adapters.make_optimizer(lr=cfg.lr)
        self.P = self.opt.P
        self.global_row = self.opt.data[0].clone()
        self.rows = torch.zeros(self.K, self.P, dtype=torch.float32, device=self.dev)
        self.coeffs = torch.full((self.K,), 1.0 / self.K, dtype=torch.float32, device=self.dev)
        tok = SPTokenizer(cfg.vocab_size)
        self.streams = [TinyStories(tok, cfg.batch_size, cfg.ctx_size, seed=cfg.dialect_seed + d,
                                    skip=0, sub_vocab=cfg.sub_vocab, branching=cfg.branching)
                        for d in range(cfg.dialects)]
        self.rng = np.random.default_rng(cfg.seed)
        self.round_idx = 0
        self.waves_last_round = 0
        self.records: list[dict] = []
        # sample_adapters = "clients": the last round's clients and their rows as uploaded
        self.last_clients: list[int] = []
        self.client_rows = None

    # ------------------------------------------------------------------------------------ data
    def client_batch(self, client: int, round_idx: int, step: int) -> np.ndarray:
        """[batch_size, ctx] of client ``client``: grammar client % dialects, the client's own block
        of sequence indices, advanced by one batch per local step of every round."""
        cfg = self.cfg
        start = (client // cfg.dialects) * CLIENT_SPAN + (round_idx * cfg.local_steps + step) * cfg.batch_size
        return self.streams[client % cfg.dialects].batch(start)

    def heldout_batch(self, dialect: int, i: int) -> torch.Tensor:
        return torch.from_numpy(self.streams[dialect].batch(HELDOUT_START + i * self.cfg.batch_size))

    # ------------------------------------------------------------------------------- evaluation
    @torch.no_grad()
    def _heldout_losses(self) -> list[float]:
        """Mean next-token loss of the model AS IT STANDS on every grammar's held-out batches."""
        out = []
        for d in range(self.cfg.dialects):
            tot = 0.0
            for i in range(self.cfg.eval_batches):
                x = self.heldout_batch(d, i).to(self.dev)
                tot += float(causalLLMLoss(self.model(x), x))
            out.append(tot / self.cfg.eval_batches)
        return out

    def evaluate(self, row=None) -> list[float]:
        """Held-out loss per dialect of the base merged with ``row`` (default: the global row)."""
        merge_lora(self.model, self.global_row if row is None else row)
        try:
            return self._heldout_losses()
        finally:
            unmerge_lora(self.model)

    @torch.no_grad()
    def _client_products(self, rows):
        """mean_k scale B_k A_k of every target -> {(block, target): [N, D]}."""
        ad, out = self.adapters, {}
        K = rows.shape[0]
        for i, blk in enumerate(self.model.blocks()):
            for t in self.lcfg.targets:
                acc = None
                for k in range(K):
                    a, b = ad.pair(rows[k], i, t)
                    p = merged_weight(torch.zeros((), device=self.dev), a, b, self.lcfg.scale)
                    acc = p if acc is None else acc + p
                out[(i, t)] = acc / K
        return out

    @torch.no_grad()
    def _gap(self, mean_prod) -> tuple[float, list[float]]:
        """(|mean_k(B_k A_k) - B_g A_g| / |mean_k(B_k A_k)| over all targets, the held-out loss of the
        base merged with the mean product)."""
        ad = self.adapters
        num = den = 0.0
        blocks = self.model.blocks()
        saved = {}
        for (i, t), m in mean_prod.items():
            a, b = ad.pair(self.global_row, i, t)
            g = merged_weight(torch.zeros((), device=self.dev), a, b, self.lcfg.scale)
            num += float((m - g).double().pow(2).sum())
            den += float(m.double().pow(2).sum())
            w = getattr(blocks[i], t)
            saved[(i, t)] = w.detach().clone()
            w.data.add_(m)
        ad._saved = saved  # the blocks take the plain path while the mean product is merged
        try:
            losses = self._heldout_losses()
        finally:
            unmerge_lora(self.model)
        return (num / max(den, 1e-300)) ** 0.5, losses

    # ----------------------------------------------------------------------------------- rounds
    def _train_wave(self, clients: list[int]) -> None:
        """The clients of one wave from the global row: ``local_steps`` steps over all slots."""
        cfg, S, k = self.cfg, self.S, len(clients)
        self.adapters.broadcast(self.global_row)
        self.opt.reset_state()
        slots = clients + [clients[0]] * (S - k)  # idle slots repeat a client; their rows are dropped
        for step in range(cfg.local_steps):
            x = torch.from_numpy(np.concatenate([self.client_batch(c, self.round_idx, step) for c in slots]))
            x = x.to(self.dev)
            self.opt.zero_grad()
            # scale S: the sum of the slots' own mean losses, so every client takes its own mean's gradient
            loss = causalLLMLoss(self.model(x), x, scale=float(S))
            loss.backward()
            self.opt.step()

    def round(self) -> dict:
        cfg = self.cfg
        t0 = time.perf_counter()
        chosen = [int(c) for c in self.rng.choice(self.N, self.K, replace=False)]
        waves = [chosen[i:i + self.S] for i in range(0, self.K, self.S)]
        for w, clients in enumerate(waves):
            self._train_wave(clients)
            self.rows[w * self.S:w * self.S + len(clients)].copy_(self.opt.data[:len(clients)])
        self.waves_last_round = len(waves)
        mean_prod = self._client_products(self.rows) if cfg.report_gap else None
        if cfg.sample_adapters == "clients":  # before the aggregation: some rules rewrite the rows
            self.client_rows = self.rows.clone()
            self.last_clients = chosen
        aggregate_into(self.aggregator, self.ctx, self.rows, self.coeffs, self.global_row, center=self.global_row,
                       counts=[self.K], keys=list(range(self.K)))
        self.round_idx += 1
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = dict(round=self.round_idx, clients=chosen, heldout_loss=self.evaluate(), round_time=dt,
                   tokens=self.K * cfg.local_steps * cfg.batch_size * cfg.ctx_size,
                   message_count=2 * self.round_idx * self.K)
        if mean_prod is not None:
            rec["gap"], rec["mean_merged_loss"] = self._gap(mean_prod)
        self.records.append(rec)
        if self.log:
            self.log(f"[fedlora] round {self.round_idx} held-out loss "
                     + " ".join(f"{v:.4f}" for v in rec["heldout_loss"])
                     + (f" gap {rec['gap']:.3e}" if "gap" in rec else ""))
        return rec

    def result(self) -> FedLoRAResult:
        cfg = self.cfg
        res = FedLoRAResult("fedlora", self.N, self.C, cfg.batch_size, cfg.local_steps, cfg.lr, cfg.seed)
        for rec in self.records:
            res.round.append(rec["round"])
            res.heldout_loss.append(rec["heldout_loss"])
            if rec["round"] > 0:
                res.round_time.append(rec["round_time"])
                res.tokens.append(rec["tokens"])
                res.message_count.append(rec["message_count"])
                if "gap" in rec:
                    res.gap.append(rec["gap"])
                    res.mean_merged_loss.append(rec["mean_merged_loss"])
        return res

    def run(self, rounds: int | None = None) -> FedLoRAResult:
        """Run (or, with ``cfg.checkpoint``, resume) up to ``rounds`` rounds in total."""
        cfg = self.cfg
        total = cfg.rounds if rounds is None else rounds
        if cfg.checkpoint and os.path.exists(cfg.checkpoint) and self.round_idx == 0 and not self.records:
            self.load_state_dict(torch.load(cfg.checkpoint, map_location="cpu", weights_only=True))
        if not self.records:  # round 0: the base model (B = 0)
            self.records.append(dict(round=0, heldout_loss=self.evaluate()))
            if self.log:
                self.log("[fedlora] round 0 held-out loss " + " ".join(f"{v:.4f}" for v in self.records[0]["heldout_loss"]))
        while self.round_idx < total:
            self.round()
            if cfg.checkpoint:
                self.save(cfg.checkpoint)
        return self.result()

    @torch.no_grad()
    def sample(self, n_tokens: int, prompt_len: int = 8):
        """Continue the first ``prompt_len`` tokens of a held-out batch of every grammar by ``n_tokens``
        greedy tokens with the merged global adapter -> [[token ids]]. With
        ``sample_adapters = "clients"``: ``sample_clients``."""
        if self.cfg.sample_adapters == "clients":
            return self.sample_clients(n_tokens, prompt_len)
        out = []
        merge_lora(self.model, self.global_row)
        try:
            for d in range(self.cfg.dialects):
                prompt = self.heldout_batch(d, self.cfg.eval_batches)[:, :prompt_len].to(self.dev)
                out.extend(self.model.generate(prompt, max_new_tokens=n_tokens, seed=self.cfg.seed).cpu().tolist())
        finally:
            unmerge_lora(self.model)
        return out

    @torch.no_grad()
    def sample_clients(self, n_tokens: int, prompt_len: int = 8):
        """For each client of the last round: one held-out prompt of the client's grammar, continued
        by ``n_tokens`` greedy tokens under the base model, the global adapter and the client's own
        upload -> [{client, dialect, adapter, tokens}]. One adapter bank ``[global; client rows]``
        and per-sequence adapter ids, ``SAMPLE_CHUNK`` sequences per ``generate``; nothing is merged.
        (The client rows are those of a round run by this object: none after a bare resume.)"""
        from ..models.lora import adapter_bank
        if not self.last_clients:
            return []
        bank = adapter_bank(self.model, torch.cat([self.global_row[None], self.client_rows]))
        jobs = []  # (prompt [prompt_len], adapter id, labels)
        for j, c in enumerate(self.last_clients):
            d = c % self.cfg.dialects
            batch = self.heldout_batch(d, self.cfg.eval_batches)
            prompt = batch[j % batch.shape[0], :prompt_len]
            for label, aid in (("base", -1), ("global", 0), ("client", 1 + j)):
                jobs.append((prompt, aid, dict(client=c, dialect=d, adapter=label)))
        out = []
        for i in range(0, len(jobs), SAMPLE_CHUNK):
            chunk = jobs[i:i + SAMPLE_CHUNK]
            toks = self.model.generate(torch.stack([p for p, _, _ in chunk]).to(self.dev), max_new_tokens=n_tokens,
                                       seed=self.cfg.seed, adapters=bank, adapter_ids=[a for _, a, _ in chunk])
            out.extend(dict(lab, tokens=t) for (_, _, lab), t in zip(chunk, toks.cpu().tolist()))
        return out

    # ---------------------------------------------------------------------- checkpoint / resume
    def state_dict(self) -> dict:
        """The global row, the round counter and the sampling RNG (the token streams are functions of
        client, round and step), plus the records so far."""
        sd = {"global_row": self.global_row.detach().cpu().clone(), "round_idx": self.round_idx,
              "rng": self.rng.bit_generator.state, "records": self.records,
              "N": self.N, "K": self.K, "P": self.P, "seed": self.cfg.seed}
        if hasattr(self.aggregator, "state_dict"):
            sd["aggregator"] = self.aggregator.state_dict()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if (sd["N"], sd["K"], sd["P"]) != (self.N, self.K, self.P):
            raise ValueError(f"checkpoint is for a different federation {(sd['N'], sd['K'], sd['P'])}")
        self.global_row.copy_(sd["global_row"].to(self.dev))
        self.round_idx = int(sd["round_idx"])
        self.rng.bit_generator.state = sd["rng"]
        self.records = list(sd["records"])
        if "aggregator" in sd and hasattr(self.aggregator, "load_state_dict"):
            self.aggregator.load_state_dict(sd["aggregator"])

    def save(self, path: str) -> None:
        tmp = f"{path}.tmp"
        torch.save(self.state_dict(), tmp)
        os.replace(tmp, path)


def config_dict(cfg: FedLoRAConfig) -> dict:
    return dataclasses.asdict(cfg)
