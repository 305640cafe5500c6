"""Horizontal FL algorithms on the client-batched engine, one MI355X = a group of client slots.

FedAvg (McMahan et al. 2017) and FedSGD with the reference's exact round protocol
(hfl_complete.py:220-229, 260-312, 336-390):
  * ``K = max(1, round(C * N))`` clients sampled per round with ``numpy.default_rng(seed).choice(N,
    K, replace=False)`` — every rank draws the same numbers, no communication needed;
  * client ``c`` in round ``r`` shuffles its data with seed ``seed + c + 1 + r * K``;
  * weights ``n_k / sum(n_chosen)``; ``message_count = 2 * (r + 1) * K``.
Placement: chosen client ``i`` of a round runs on rank ``i % W``, slot ``i // W``; every rank holds
the (device-resident) training set, the server state ``w_global`` is replicated and updated
identically on every rank after the all-reduce, so there is no separate parameter-server process.
"""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from ..ops import functional as Fn
from ..runtime import dist as rdist
from ..runtime.staging import DeviceTables, PinnedStager
from ..utils.metrics import PhaseTimer
from . import bank as banks
from .aggregate import MeanAggregator, aggregate_into, make_aggregator
from .compress import make_compressor
from .local import LocalTrainer
from .result import RunResult
from .server_opt import make_server_opt


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


class FederatedBase:
    algorithm = "Fed"

    def __init__(self, model_fn, train_data, client_indices, *, lr: float, batch_size: int = -1,
                 local_epochs: int = 1, client_fraction: float = 1.0, seed: int = 0, test_data=None,
                 aggregator="mean", attack=None, ctx=None, momentum: float = 0.0,
                 weight_decay: float = 0.0, planner: str = "native", use_graph=None,
                 init_fn=None, eval_every: int = 1, eval_limit: int | None = None, name=None,
                 agg_kwargs=None, dropout: float = 0.0, stragglers: float = 0.0,
                 straggler_slowdown: float = 4.0, deadline: float | None = None, prox_mu: float = 0.0,
                 server_opt=None, server_opt_kwargs=None, compressor=None, compressor_kwargs=None,
                 backdoor_test=None):
        # [NS] heterogeneity: FedProx's proximal term mu/2 |w - w_global|^2 in every client's
        # objective (Li et al. 2020), and a FedOpt server optimizer stepping w_global with the
        # aggregate update as pseudo-gradient (Reddi et al. 2021); both off by default
        if prox_mu < 0.0:
            raise ValueError(f"prox_mu must be >= 0, got {prox_mu}")
        self.prox_mu = float(prox_mu)
        self.server_opt = make_server_opt(server_opt, **(server_opt_kwargs or {})) \
            if isinstance(server_opt, str) else server_opt
        # [NS] compressed uploads: every reporting client's update goes through a lossy codec with
        # error feedback (fl/compress.py) before an attack or the server sees it; off by default
        self.compressor = make_compressor(compressor, **(compressor_kwargs or {})) \
            if isinstance(compressor, str) else compressor
        self._uplink: list = []
        self._slot_tables, self._coeff_cache = DeviceTables(), DeviceTables()
        self.ctx = ctx or rdist.context()
        self.dev = self.ctx.device
        self.data = train_data
        self.test_data = test_data
        self.client_indices = [np.asarray(c, dtype=np.int64) for c in client_indices]
        self.N = len(self.client_indices)
        self.C = client_fraction
        self.K = max(1, round(client_fraction * self.N))
        self.W = self.ctx.world
        self.slots = math.ceil(self.K / self.W)
        self.lr, self.B, self.E, self.seed = lr, batch_size, local_epochs, seed
        self.rng = np.random.default_rng(seed)
        self.counts = [len(c) for c in self.client_indices]
        self.net = model_fn(groups=self.slots).to(self.dev, seed=seed)
        if init_fn is not None:
            init_fn(self.net)
        self.data.set_input_spec(self.net.input_spec)
        if self.test_data is not None:
            self.test_data.set_input_spec(self.net.input_spec)
        # [NS] the triggered test set of a backdoor attack (``Backdoor.triggered_test``): the server
        # model's accuracy on it is the attack success rate, reported beside the test accuracy
        self.backdoor_test = backdoor_test
        if self.backdoor_test is not None:
            self.backdoor_test.set_input_spec(self.net.input_spec)
        st = self.net.store
        self.w_global = st.data[0].clone()
        self.b_global = st.buffers[0].clone()
        if self.compressor is not None:
            self.compressor.bind(self.N, self.w_global.numel(), self.slots, self.dev)
        self.aggregator = aggregator if not isinstance(aggregator, str) else \
            make_aggregator(aggregator, **(agg_kwargs or {}))
        self.mean = MeanAggregator()
        self.attack = attack
        self.momentum, self.weight_decay = momentum, weight_decay
        self.planner, self.use_graph = planner, use_graph
        self.eval_every, self.eval_limit = eval_every, eval_limit
        self.name = name or self.algorithm
        self.round_idx = 0
        # [NS] client unavailability: each sampled client independently fails to report with
        # probability ``dropout`` (own RNG stream, so the client-sampling sequence is unchanged)
        self.dropout = dropout
        self.fail_rng = np.random.default_rng([seed, 0xD20])
        self.dropped: list[list[int]] = []
        # [NS] stragglers: each sampled client is independently slow with probability
        # ``stragglers`` (its local round takes ``straggler_slowdown`` x the nominal time of its
        # shard, n_k * E samples at unit speed). With a ``deadline`` (in nominal times of the mean
        # shard) the server aggregates only the clients that report in time, the synchronous-FL
        # policy of dropping stragglers; ``sim_time`` records each round's simulated duration
        # (slowest reporting client), the reference's "parallel wall time = max over clients"
        # (hfl_complete.py:294,296) under heterogeneous client speed.
        self.stragglers, self.slowdown, self.deadline = stragglers, straggler_slowdown, deadline
        self.strag_rng = np.random.default_rng([seed, 0x57A6])
        self.straggled: list[list[int]] = []
        self.sim_time: list[float] = []
        self.timer = PhaseTimer(self.dev)  # download / local_train / aggregate (HIP events + roctx)
        # sync_rounds=False: FedAvg rounds run without any host <-> device synchronisation (no
        # per-round wall time; round() returns dt = 0 and this rank's sample count), so the host
        # samples, plans and enqueues round r+1 while the GPU still executes round r. For
        # throughput runs (bench.py); run() keeps the reference's per-round timing.
        self.sync_rounds = True

    def _sample(self):
        chosen = self.rng.choice(self.N, self.K, replace=False)
        # the round's cohort: everyone sampled, before the dropout and deadline filters (secure
        # aggregation masks against it; the clients that never report are what it recovers from)
        self.cohort = [int(c) for c in chosen]
        if self.dropout > 0:
            alive = self.fail_rng.random(len(chosen)) >= self.dropout
            self.dropped.append([int(c) for c in chosen[~alive]])
            chosen = chosen[alive]
        if self.stragglers > 0:
            slow = self.strag_rng.random(len(chosen)) < self.stragglers
            mean_n = float(np.mean(self.counts))
            t = np.array([self.counts[int(c)] / mean_n for c in chosen]) * \
                np.where(slow, self.slowdown, 1.0)
            late = t > self.deadline if self.deadline is not None else np.zeros(len(chosen), bool)
            self.straggled.append([int(c) for c in chosen[late]])
            self.sim_time.append(float(t[~late].max()) if (~late).any() else 0.0)
            chosen = chosen[~late]
        return chosen

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self) -> dict:
        """Everything needed to continue bit-identically: server model, round counter, RNG streams
        (loader seeds derive from seed/round/client, so they need no state)."""
        sd = {"w_global": self.w_global.detach().cpu().clone(),
              "b_global": self.b_global.detach().cpu().clone(),
              "round_idx": self.round_idx, "rng": self.rng.bit_generator.state,
              "fail_rng": self.fail_rng.bit_generator.state, "dropped": self.dropped,
              "strag_rng": self.strag_rng.bit_generator.state, "straggled": self.straggled,
              "sim_time": self.sim_time,
              "algorithm": self.algorithm, "N": self.N, "K": self.K, "seed": self.seed,
              "param_layout": self.net.store.param_layout()}
        if hasattr(self, "g_global"):
            sd["g_global"] = self.g_global.detach().cpu().clone()
        if self.attack is not None:
            sd["attack"] = self.attack.state_dict()
        if hasattr(self.aggregator, "state_dict"):  # e.g. ClippedMean's noise round counter
            sd["aggregator"] = self.aggregator.state_dict()
        if self.server_opt is not None:  # the moments m, v: flat rows in this run's parameter layout
            sd["server_opt"] = self.server_opt.state_dict()
        if self.compressor is not None:  # the error bank (rows in this run's layout), the codec's round
            sd["compressor"] = self.compressor.state_dict()
            sd["uplink_bytes"] = self.uplink_bytes
        return sd

    def _layout_fix(self, sd: dict):
        """-> the map of a checkpoint's flat row [P] (or rows [N, P]) to this run's parameter
        layout: by parameter name when the writer used another layout, else the identity."""
        st = self.net.store
        src = sd.get("param_layout") or st.param_layout()
        if [list(x) for x in src] == st.param_layout():
            return lambda t: t
        return lambda t: st.remap_flat(t, src) if t.dim() == 1 else torch.stack([st.remap_flat(r, src) for r in t])

    def load_state_dict(self, sd: dict) -> None:
        if (sd["algorithm"], sd["N"], sd["K"]) != (self.algorithm, self.N, self.K):
            raise ValueError("checkpoint is for a different federation "
                             f"{(sd['algorithm'], sd['N'], sd['K'])}")
        fix = self._layout_fix(sd)
        self.w_global.copy_(fix(sd["w_global"]).to(self.dev))
        self.b_global.copy_(sd["b_global"].to(self.dev))
        if "g_global" in sd and hasattr(self, "g_global"):
            self.g_global.copy_(fix(sd["g_global"]).to(self.dev))
        self.round_idx = int(sd["round_idx"])
        self.rng.bit_generator.state = sd["rng"]
        self.fail_rng.bit_generator.state = sd["fail_rng"]
        self.dropped = [list(d) for d in sd["dropped"]]
        if "strag_rng" in sd:
            self.strag_rng.bit_generator.state = sd["strag_rng"]
            self.straggled = [list(d) for d in sd["straggled"]]
            self.sim_time = list(sd["sim_time"])
        if self.attack is not None and "attack" in sd:
            self.attack.load_state_dict(sd["attack"])
        if "aggregator" in sd and hasattr(self.aggregator, "load_state_dict"):
            self.aggregator.load_state_dict(sd["aggregator"])
        if self.server_opt is not None and "server_opt" in sd:
            self.server_opt.load_state_dict(sd["server_opt"], like=self.w_global, fix=fix)
        if self.compressor is not None and "compressor" in sd:
            self.compressor.load_state_dict(sd["compressor"], fix=fix)
            self._uplink = [int(b) for b in sd.get("uplink_bytes", [])]

    @property
    def uplink_bytes(self) -> list[int]:
        """Bytes the round's reporting clients (of all ranks) sent up, one entry per round, when a
        compressor is on: the codec's payload for the parameters plus the dense BN buffers. Top-k's
        counts live on the device until they are read here (as ``ClippedMean.last_norms``)."""
        for i, v in enumerate(self._uplink):
            if not isinstance(v, int):
                nnz, counts, fixed = v
                n = sum(int(nnz[w, :c].sum()) for w, c in enumerate(counts))
                self._uplink[i] = self.compressor.uplink_bytes(self.w_global.numel(), n) + fixed
        return list(self._uplink)

    # ------------------------------------------------------------------ helpers
    def _assign(self, chosen):
        mine = [int(c) for c in chosen[self.ctx.rank::self.W]]
        counts = [len(chosen[i::self.W]) for i in range(self.W)]
        return mine, counts

    def _coeffs(self, mine, total):
        """Device tensor of the n_k / n weights of my clients; cached per (clients, total), since
        building it from a host list is a blocking copy."""
        return self._coeff_cache.get((tuple(mine), total), lambda: torch.tensor(
            [self.counts[c] / total for c in mine], dtype=torch.float32, device=self.dev))

    def _begin_round(self):
        """Sample the round and tell the aggregator -> (chosen, mine, counts per rank, total samples),
        or None when every sampled client dropped out: the server model stays, the round is counted."""
        chosen = self._sample()
        mine, self._counts = self._assign(chosen)  # the counts are kept for the hooks that gather over the ranks
        self._announce(chosen, mine)
        if len(chosen) == 0:
            self.round_idx += 1
            if self.compressor is not None:
                self._uplink.append(0)
            return None
        return chosen, mine, self._counts, float(sum(self.counts[int(c)] for c in chosen))

    def _row_keys(self, counts):
        """Each rank-major client row's position in the round's `chosen` order (round-robin
        assignment above): the robust rules break exact ties by it, so a run gives the same
        aggregate on one GPU and on W."""
        return [l * self.W + w for w in range(self.W) for l in range(counts[w])]

    def _announce(self, chosen, mine) -> bool:
        """Tell an aggregator that wants it (``SecureMean.begin_round``) the round's cohort, its
        survivors and this rank's clients. No survivor at all: the aggregator counts an aborted
        round, as the engine skips the aggregation. BN buffers keep the plain mean either way.
        -> whether the aggregator was told."""
        agg = self.aggregator
        if not hasattr(agg, "begin_round"):
            return False
        agg.begin_round(self.cohort, [int(c) for c in chosen], mine)
        if len(chosen) == 0:
            agg.abort_round()
        return True

    def _poison(self, rows, center, chosen, mine):
        """The model-poisoning attack on this rank's rows. An attack with ``begin_round`` is told the
        round first; a ``collective`` one (it gathers rows over the ranks) is called on every rank
        of a distributed run, also on one without a client."""
        atk = self.attack
        if atk is None:
            return
        if hasattr(atk, "begin_round"):
            atk.begin_round(self.ctx, chosen, mine)
        if len(mine) or (getattr(atk, "collective", False) and self.ctx.is_distributed):
            atk.poison_updates(rows, center, mine)

    def _download(self, G):
        st = self.net.store
        if G:
            Fn.broadcast_rows(self.w_global, st.data[:G], None if st.shadow16 is None else st.shadow16[:G])
            Fn.broadcast_rows(self.b_global, st.buffers[:G])
            st._shadow_version = st.data._version

    def _mean_buffers(self, G, coeffs):
        st = self.net.store
        self.mean(self.ctx, st.buffers[:G], coeffs, self.b_global)

    def test(self) -> float:
        """Server-model test accuracy in % (reference Server.test, hfl_complete.py:172-183)."""
        return self._accuracy(self.test_data)

    def test_backdoor(self) -> float:
        """Server-model accuracy in % on ``backdoor_test``, the attack success rate (NaN without one)."""
        return self._accuracy(self.backdoor_test)

    @torch.no_grad()
    def _accuracy(self, data) -> float:
        if data is None or len(data) == 0:
            return float("nan")
        st = self.net.store
        self._download(1)
        n = len(data) if self.eval_limit is None else min(self.eval_limit, len(data))
        correct = torch.zeros(1, dtype=torch.int64, device=self.dev)
        chunk = 2000
        with st.select(0, 1):
            for s in range(0, n, chunk):
                e = min(n, s + chunk)
                idx = torch.arange(s, e, dtype=torch.int32, device=self.dev).reshape(1, -1)
                x, y = data.batch(idx)
                logits, _ = self.net.forward_native(x, False)
                _, _, c = Fn.cross_entropy(logits, y, ncls=self.net.num_classes, want_grad=False,
                                           with_correct=True)
                correct += c.to(torch.int64)
        return 100.0 * correct.item() / n

    def run(self, nr_rounds: int) -> RunResult:
        res = RunResult(self.name, self.N, self.C, self.B, self.E, self.lr, self.seed)
        elapsed = 0.0
        for _ in range(nr_rounds):
            dt, samples = self.round()
            elapsed += dt
            res.wall_time.append(round(elapsed, 1))
            res.round_time.append(dt)
            res.samples.append(samples)
            res.message_count.append(2 * self.round_idx * self.K)
            res.phase_ms.append(self.timer.summary())
            evaluate = self.eval_every and self.round_idx % self.eval_every == 0
            res.test_accuracy.append(self.test() if evaluate else float("nan"))
            if self.backdoor_test is not None:
                res.backdoor_accuracy.append(self.test_backdoor() if evaluate else float("nan"))
        return res


class FedAvg(FederatedBase):
    algorithm = "FedAvg"
    trainer = None  # the LocalTrainer, built in the first round

    def _trainer(self, mine):
        lt = None
        if self.attack is not None:
            lt = self.attack.label_transform_for(mine, self.net.num_classes)
        if self.trainer is None:
            self.trainer = LocalTrainer(self.net, self.data, self.lr, self.B, self.momentum,
                                        self.weight_decay, self.planner, self.use_graph,
                                        prox_mu=self.prox_mu,
                                        anchor=self.w_global if self.prox_mu > 0.0 else None,
                                        **self._trainer_kwargs())
            self._graph_default = self.trainer.use_graph
        self.trainer.label_transform = lt
        # a label transform is graph-captured only if it declares a graph_key (pure device ops,
        # e.g. LabelFlip); otherwise eager steps for the rounds that need one
        self.trainer.use_graph = self._graph_default and (lt is None or hasattr(lt, "graph_key"))
        return self.trainer

    # hooks of the subclasses that keep per-client state (Scaffold); no-ops here
    def _trainer_kwargs(self) -> dict:
        return {}

    def _before_local(self, mine):
        """The round's clients of this rank are known, nothing has trained yet."""

    def _after_local(self, mine, chosen):
        """The slots hold what the clients trained; no attack has touched the rows yet."""
        if self.compressor is not None:
            self._compress(mine, chosen)

    def _compress(self, mine, chosen):
        """Slot g's row becomes what the server decodes from client mine[g]'s compressed upload; the
        client's error row takes the residual. BN buffers stay dense. On several ranks the bank is
        replicated: the round's new rows are all-gathered and written by client id, as Scaffold's."""
        comp, st, G = self.compressor, self.net.store, len(mine)
        P, dense = self.w_global.numel(), 4 * self.b_global.numel() * len(chosen)
        with self.timer("compress"):
            nnz = None
            if G:
                ids = Fn.check_slot_clients(mine, self.N)  # the table is validated here, where it is built
                table = self._slot_tables.get(tuple(ids), lambda: torch.tensor(ids, dtype=torch.int32, device=self.dev))
                nnz = comp.apply(st.data[:G], self.w_global, table)
            else:
                comp.skip()  # every rank counts the round: the draws do not depend on the placement
            if comp.name == "topk":
                send = torch.zeros(self.slots, dtype=torch.int32, device=self.dev)
                if G:
                    send[:G] = nnz
                self._uplink.append((self.ctx.all_gather_rows(send), self._counts, dense))
            else:
                self._uplink.append(len(chosen) * comp.uplink_bytes(P) + dense)
            if comp.bank is not None:
                banks.replicate_rows(self.ctx, comp.bank, chosen, mine, self.slots)

    def round(self):
        if self.sync_rounds:
            _sync(self.dev)
        t0 = time.perf_counter()
        began = self._begin_round()
        if began is None:
            return self.ctx.max_scalar(time.perf_counter() - t0), 0
        chosen, mine, counts, total = began
        G = len(mine)
        r = self.round_idx
        with self.timer("download"):
            self._download(G)
        seeds = [self.seed + c + 1 + r * self.K for c in mine]
        gens = [torch.Generator().manual_seed(s) for s in seeds] if self.planner == "torch" else None
        trainer = self._trainer(mine)
        bsz = self.B
        samples = 0
        if G:
            # every slot trains in the one client-batched launch; a free rider's row is then
            # overwritten with w_global by its poison_updates (no separate code path per client)
            if bsz <= 0:  # B = infinity: full local batch
                trainer.B = max(self.counts[c] for c in mine)
            self._before_local(mine)
            with self.timer("local_train"):
                samples = trainer.run([self.client_indices[c] for c in mine], seeds, self.E, gens)
            if self.attack is not None:  # free riders did no useful work: do not count it
                samples -= sum(self.E * self.counts[c] for c in mine if self.attack.skip_training(c))
        self._after_local(mine, chosen)
        st = self.net.store
        self._poison(st.data[:G], self.w_global, chosen, mine)
        coeffs = self._coeffs(mine, total)
        with self.timer("aggregate"):
            self._aggregate(st.data[:G], coeffs, counts)
            self._mean_buffers(G, coeffs)
        self.round_idx += 1
        if not self.sync_rounds:
            return 0.0, samples
        _sync(self.dev)
        self.ctx.check_comm()  # a peer-read all-reduce barrier timeout raises here, not silently
        dt = self.ctx.max_scalar(time.perf_counter() - t0)
        samples = int(self.ctx.sum_scalar(samples))
        return dt, samples

    def _aggregate(self, rows, coeffs, counts):
        if self.server_opt is not None:
            return self._aggregate_server_opt(rows, coeffs, counts)
        aggregate_into(self.aggregator, self.ctx, rows, coeffs, self.w_global, center=self.w_global,
                       counts=counts, keys=self._row_keys(counts))

    # one launch for sum + server step where the plain mean needs no cross-rank route (off: the
    # scratch-row route, which the tests hold bit-equal to it)
    fuse_server_opt = True

    def _aggregate_server_opt(self, rows, coeffs, counts):
        """The aggregator's result goes to a scratch row instead of w_global; the server optimizer
        then steps w_global towards it. m, v are replicated: every rank holds the same aggregate
        after the aggregator's own cross-rank route and steps identically."""
        opt, agg = self.server_opt, self.aggregator
        plain = type(agg) is MeanAggregator
        if plain and self.fuse_server_opt and not self.ctx.is_distributed and rows.shape[0] \
                and rows.stride(1) == 1:
            opt.step_rows(rows, coeffs, self.w_global)
            return
        target = getattr(self, "_opt_target", None)
        if target is None:
            target = self._opt_target = torch.empty_like(self.w_global)
        # a robust rule's result already is the delta; a mean's is the new vector
        is_delta = aggregate_into(agg, self.ctx, rows, coeffs, target, center=self.w_global, counts=counts,
                                  keys=self._row_keys(counts), as_update=True)
        opt.step(self.w_global, target, is_delta)


class Scaffold(FedAvg):
    """SCAFFOLD (Karimireddy et al. 2020, Algorithm 1, option II) [north-star; absent from the
    reference]: FedAvg whose clients correct their drift with control variates. The server holds
    ``c_global [P]``, client i holds row i of ``c_bank [N, P]``, all zero at the start. A reporting
    client i starts from y = x (= w_global) and takes its K_i local steps on g(y) + (c - c_i); then

        dc_i = (x - y_i) / (K_i lr) - c,    c_i += dc_i,    c += (1 / N) sum_reporting dc_i

    with N all clients, not the sampled ones. x is aggregated from the rows y_i exactly as in
    FedAvg: weights n_k / n, any aggregator, any FedOpt server optimizer behind it (the paper's
    global step size eta_g is ``server_opt="fedavgm"`` with beta1 = 0 and lr = eta_g). K_i is the
    number of optimizer steps client i really took, E * ceil(n_i / B), short last step included.

    The bank is one flat fp32 buffer like the client models; the fused optimizer launch reads row
    ``slot_client[slot]`` of it in place (scaffold.hip), also inside the captured round graph: the
    table is a persistent device buffer of ``slots`` entries whose contents each round overwrites.
    Every rank holds the whole bank, N * P * 4 bytes (10 clients of ResNet-18: 0.45 GB; 100: 4.5 GB);
    on several ranks the round's new rows are all-gathered and written into every rank's bank by
    client id, and dc takes the mean's rank-ordered sum.

    The control variates come from what the client really trained: they are updated after local
    training and before ``attack.poison_updates``, so a model-poisoning attack changes the row the
    server aggregates, not the client's c_i. Clients that dropped out or missed the deadline keep
    their c_i. Not combined with ``prox_mu``; FedSGD has no local steps to correct."""
    algorithm = "Scaffold"

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if self.prox_mu > 0.0:
            raise ValueError("Scaffold: the control variates and prox_mu > 0 are not combined")
        if self.compressor is not None:
            raise ValueError("Scaffold: the control variates are formed from the uncompressed rows; "
                             "a compressor is not combined with them")
        if getattr(self.aggregator, "name", None) == "secagg":
            raise ValueError("Scaffold: the control-variate sums would stay in the clear; secure "
                             "aggregation is not combined with them")
        P = self.w_global.numel()
        self.c_global = torch.zeros(P, dtype=torch.float32, device=self.dev)
        self.c_bank = torch.zeros(self.N, P, dtype=torch.float32, device=self.dev)
        self.slot_client = torch.zeros(self.slots, dtype=torch.int32, device=self.dev)
        self._inv_klr = torch.zeros(self.slots, dtype=torch.float32, device=self.dev)
        self._dc = torch.zeros(P, dtype=torch.float32, device=self.dev)
        self._stagers = {"slot_client": PinnedStager(self.slot_client.shape, torch.int32),
                         "inv_klr": PinnedStager(self._inv_klr.shape, torch.float32)}

    def _trainer_kwargs(self) -> dict:
        return {"control": (self.c_global, self.c_bank, self.slot_client)}

    def local_steps(self, client: int, batch: int | None = None) -> int:
        """K_i: the optimizer steps client i takes in a round, E * ceil(n_i / B)."""
        B = self.B if batch is None else batch
        n = self.counts[client]
        return self.E * (math.ceil(n / B) if B > 0 else 1)

    def _stage(self, name: str, values: np.ndarray, out: torch.Tensor):
        """Host values -> out[:len(values)] of a persistent device buffer, without a blocking copy."""
        self._stagers[name].put(values, out[:len(values)])

    def _before_local(self, mine):
        ids = Fn.check_slot_clients(mine, self.N)  # the table is validated here, where it is built
        self._stage("slot_client", np.asarray(ids, dtype=np.int32), self.slot_client)
        B = self.trainer.B  # the round's batch size (the largest shard when B = infinity)
        inv = [1.0 / (self.local_steps(c, B) * self.lr) for c in ids]
        self._stage("inv_klr", np.asarray(inv, dtype=np.float32), self._inv_klr)

    def _after_local(self, mine, chosen):
        G, st = len(mine), self.net.store
        dist_ = self.ctx.is_distributed
        with self.timer("control"):
            if G:
                Fn.scaffold_finish(st.data[:G], self.w_global, self.c_global, self.c_bank, self.slot_client[:G],
                                   self._inv_klr[:G], 1.0 / self.N, self._dc, apply_c=not dist_)
            else:
                self._dc.zero_()
            if not dist_:
                return
            self.mean.cross_rank_sum(self.ctx, self._dc)
            self.c_global.add_(self._dc)
            banks.replicate_rows(self.ctx, self.c_bank, chosen, mine, self.slots)

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["c_global"] = self.c_global.detach().cpu().clone()
        sd["c_bank"] = banks.bank_state(self.c_bank)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        fix = self._layout_fix(sd)
        self.c_global.copy_(fix(sd["c_global"]).to(self.dev))
        banks.load_bank(self.c_bank, sd["c_bank"], fix, "control variates")


class FedSGD(FederatedBase):
    """Clients return the full-local-batch gradient at w_global; the server takes one SGD step
    with the weighted-mean gradient (reference FedSgdGradientServer, hfl_complete.py:260-312)."""
    algorithm = "FedSGDGradient"

    def __init__(self, *a, max_microbatch: int = 4096, **kw):
        kw.setdefault("batch_size", -1)
        super().__init__(*a, **kw)
        if self.prox_mu > 0.0:
            raise ValueError("FedSGD: the proximal term vanishes at w_global, prox_mu has no effect")
        if self.server_opt is not None:
            raise ValueError("FedSGD: a server optimizer on gradients is not supported (use FedAvg)")
        if self.compressor is not None:
            raise ValueError("FedSGD: the compressor works on trained rows (use FedAvg or FedSgdWeight)")
        self.max_mb = max_microbatch
        self.g_global = torch.zeros_like(self.w_global)

    def round(self):
        _sync(self.dev)
        t0 = time.perf_counter()
        began = self._begin_round()
        if began is None:
            return self.ctx.max_scalar(time.perf_counter() - t0), 0
        chosen, mine, counts, total = began
        G = len(mine)
        self._download(G)
        st, net = self.net.store, self.net
        samples = 0
        if G:
            st.grad[:G].zero_()
            sizes = [self.counts[c] for c in mine]
            same = len(set(sizes)) == 1
            groups = [(0, G)] if same else [(g, g + 1) for g in range(G)]
            for g0, g1 in groups:
                n = sizes[g0]
                idx_all = np.stack([self.client_indices[mine[g]] for g in range(g0, g1)]).astype(np.int32)
                idx_dev = torch.from_numpy(idx_all).to(self.dev)
                lt = self.attack.label_transform_for(mine, net.num_classes) if self.attack else None
                with st.select(g0, g1):
                    for s in range(0, n, self.max_mb):
                        e = min(n, s + self.max_mb)
                        x, y = self.data.batch(idx_dev[:, s:e].contiguous())
                        if lt is not None:
                            y = lt(y, g0, g1)
                        net.train_step(x, y, scale=1.0 / n)
                        samples += (g1 - g0) * (e - s)
        # model-poisoning attacks act on the reported gradient ("update" = -grad direction)
        self._poison(st.grad[:G], torch.zeros_like(self.w_global) if self.attack is not None else None,
                     chosen, mine)
        coeffs = self._coeffs(mine, total)
        aggregate_into(self.aggregator, self.ctx, st.grad[:G], coeffs, self.g_global, center=None,  # the updates
                       counts=counts, keys=self._row_keys(counts))                                  # are the gradients
        # server SGD step (no momentum, as the reference's SGD(lr))
        self.w_global.add_(self.g_global, alpha=-self.lr)
        if G:  # BN running stats from this round's forward passes
            self._mean_buffers(G, coeffs)
        _sync(self.dev)
        dt = self.ctx.max_scalar(time.perf_counter() - t0)
        self.round_idx += 1
        return dt, int(self.ctx.sum_scalar(samples))


class FedSgdWeight(FedAvg):
    """FedSGD exchanging *weights*: one full-batch SGD step per client, then FedAvg. Equals FedSGD
    exactly (sum_k p_k (w - lr g_k) = w - lr sum_k p_k g_k). The reference's homework version
    (homework-1.ipynb:178-230) exchanged gradients under this name."""
    algorithm = "FedSGDWeight"

    def __init__(self, *a, **kw):
        kw["batch_size"] = -1
        kw["local_epochs"] = 1
        super().__init__(*a, **kw)
