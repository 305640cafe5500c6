"""Server-side aggregation across the clients of a round, distributed over the GPUs.

* ``MeanAggregator`` — FedAvg / FedSGD weighted mean ``sum_k (n_k / n) w_k`` (reference
  hfl_complete.py:370-378): per-GPU weighted row-reduction kernel (products rounded, added in client
  order), then across the ranks either ONE all-reduce of P floats, or (``ordered``, the default) a
  rank-ORDER sum of the W partials — so a run with one client per GPU is bitwise the single-process
  multi-slot run (the 8-GPU headline layout reproduces the 1-GPU model exactly). On one node the
  ordered sum runs on the peer-read kernel over xGMI (runtime/ipc.py, slot-sized chunks, every
  rank adds p0 + p1 + ... itself); without peer mappings (or on gloo) an all-gather of the W
  partials added in rank order by the weighted-sum kernel.
* Byzantine-robust aggregators [north-star; absent from the reference, announced in its
  README.md:89-92]: ``Krum`` / multi-Krum (Blanchard et al. 2017), coordinate-wise ``Median`` and
  ``TrimmedMean`` (Yin et al. 2018). They need every client vector, so they run *coordinate-
  sharded*: one all-to-all gives each GPU 1/W of the coordinates of all K clients; median /
  trimmed-mean are local per-coordinate selection kernels followed by an all-gather; Krum computes
  a partial K x K Gram on its shard with the exact-fp32 MFMA, all-reduces the tiny K x K matrix,
  scores and selects redundantly on every GPU in one small kernel (krum_select) and averages the
  winners' shards by index (mean_rows_idx). One GPU skips the sharding: the rules read the client
  rows in place; several GPUs build the all-to-all send buffer with one pack kernel.
* ``ClippedMean`` — norm bounding (Sun et al. 2019) and DP-FedAvg (McMahan et al. 2018)
  [north-star]: each update clipped to L2 norm C, then the weighted mean, optionally plus Gaussian
  noise; streaming kernels (clip_agg.hip), the mean's cross-rank route, any number of clients.
* ``RobustLR`` — the robust learning rate (Ozdayi et al. 2021) [north-star], aimed at backdoors: the
  clipped mean with a per-coordinate sign vote formed in the same pass over the rows (rlr_sum); where
  too few clients agree the aggregate is negated.
* ``CenteredClip`` — centered clipping (Karimireddy et al. 2021) [north-star]: iterated clipping
  around a carried estimate of the aggregate update; the clipped mean's ops, or one fused step kernel
  per iteration on a single GPU.
* ``Bulyan`` (El Mhamdi et al. 2018) [north-star]: coordinate-sharded like Krum; iterated Krum
  selection on the Gram (bulyan_select), then per coordinate the mean of the selected values nearest
  their median (bulyan_coord).
* ``GeometricMedian`` — RFA, the smoothed Weiszfeld iteration (Pillutla et al. 2022) [north-star]:
  centered clipping's step with the row scales a_k / max(nu, distance), normalised (gm_scales).
* ``FLTrust`` (Cao et al. 2021) [north-star]: trust scores against an update the server trains
  itself on a small root dataset: one fused dot / norm pass (root_dots), then the clipped mean's route.
* ``SecureMean`` — secure aggregation (Bonawitz et al. 2017) [north-star]: the clipped mean on
  fixed-point uploads under pairwise masks that cancel in the sum, with recovery from dropped clients
  (secagg.hip). Key agreement and secret sharing are simulated: every mask is a pure function of
  (seed, round, pair, coordinate).
Robust rules operate on client *updates* (w_k - w_global) — distances between raw weights would
cancel catastrophically in fp32.
"""
from __future__ import annotations

import math

import torch

from ..ops import functional as Fn
from ..runtime.staging import DeviceTables


class MeanAggregator:
    name = "mean"
    needs_all = False

    def __init__(self, ordered: bool | None = None):
        import os
        self.ordered = (os.environ.get("DDL_FL_ORDERED_MEAN", "1") != "0") if ordered is None else bool(ordered)
        self._tables = DeviceTables()  # small device tensors built on the host: ones, weights, id tables

    def __call__(self, ctx, rows: torch.Tensor, coeffs: torch.Tensor, out: torch.Tensor):
        """rows [G_local, P] (strided ok), coeffs [G_local] -> out[P] = global weighted sum."""
        if rows.shape[0] == 0:
            out.zero_()
        else:
            Fn.weighted_sum(rows, coeffs, out)
        return self.cross_rank_sum(ctx, out)

    def cross_rank_sum(self, ctx, out: torch.Tensor):
        """out[P] (this rank's partial) -> the sum over the ranks, in place, on every rank."""
        if not ctx.is_distributed:
            return out
        if not self.ordered:
            ctx.all_reduce(out)
            return out
        ipc = getattr(ctx, "ipc", None)
        if ipc is not None and out.is_cuda and out.is_contiguous() and out.data_ptr() % 16 == 0:
            # rank-order sum by peer reads over xGMI, in slot-sized chunks: the same bits as the
            # all-gather + ordered add below, moving ~2P floats per GPU instead of W x P
            ipc.all_reduce_ordered(out)
            return out
        parts = ctx.all_gather_rows(out)  # [W, P]: every rank's partial, in rank order
        W, dev = parts.shape[0], out.device
        ones = self._tables.get(("ones", W, dev), lambda: torch.ones(W, dtype=torch.float32, device=dev))
        Fn.weighted_sum(parts, ones, out)  # x 1.0 is exact: a plain rank-order sum
        return out

    def describe(self, ctx) -> str:
        if not ctx.is_distributed:
            return "local weighted sum"
        if not self.ordered:
            return "all-reduce"
        if getattr(ctx, "ipc", None) is not None:
            return "ipc peer-read rank-ordered sum"
        return "rank-ordered all-gather + sum"


class ClippedMean(MeanAggregator):
    """Norm-bounded FedAvg (Sun et al. 2019) and DP-FedAvg (McMahan et al. 2018) [north-star]:
    every client update ``u_k = w_k - center`` is scaled to L2 norm at most ``clip`` before the
    weighted mean, and ``noise_multiplier`` z > 0 adds N(0, (z * clip / K_r)^2) to the aggregate.

    Per GPU: update_sqnorm -> clip_scales -> clipped_sum into a cached ``delta [P]`` (two reads of
    the client rows, no all-to-all, no limit on K); ``delta`` then takes ``MeanAggregator``'s route
    across the ranks; apply_update writes ``out = center + delta + noise`` with the identical noise
    on every rank (a pure function of seed, round and coordinate). A row holding a NaN / Inf entry
    is dropped (weight 0). No host synchronisation, except in ``last_norms``.

    ``weighting``: "samples" keeps the server's n_k / n; "uniform" weighs every reporting client
    1 / K_r (K_r = sum(counts), the same on every rank). Noise needs "uniform": the sensitivity of
    a sample-weighted sum to one client is not clip / K_r."""
    name = "clipped_mean"
    needs_all = False
    takes_center = True

    def __init__(self, clip: float, noise_multiplier: float = 0.0, seed: int = 0,
                 weighting: str = "samples", ordered: bool | None = None):
        super().__init__(ordered)
        self.clip, self.noise_multiplier, self.seed = float(clip), float(noise_multiplier), int(seed)
        if not self.clip > 0.0:
            raise ValueError(f"clip must be positive, got {clip}")
        if weighting not in ("samples", "uniform"):
            raise ValueError(f"weighting must be 'samples' or 'uniform', got {weighting!r}")
        if self.noise_multiplier < 0.0:
            raise ValueError(f"noise_multiplier must be >= 0, got {noise_multiplier}")
        if self.noise_multiplier > 0.0 and weighting != "uniform":
            raise ValueError("noise_multiplier > 0 needs weighting='uniform': the sensitivity of a "
                             "sample-weighted sum is not clip / K")
        self.weighting = weighting
        self.rounds = 0      # the noise stream's round: this aggregator's own call counter
        self.last_k = 0      # clients that reported in the last round (all ranks)
        self._norms = None

    def __call__(self, ctx, rows: torch.Tensor, coeffs: torch.Tensor, out: torch.Tensor,
                 center: torch.Tensor | None = None, counts: list[int] | None = None):
        """rows [G_local, P], coeffs [G_local], center [P] or None (the rows are the updates) ->
        out[P] = center + sum_k c_k * clip(rows_k - center) (+ noise); out may be center."""
        if counts is None:
            if ctx.is_distributed and self.weighting == "uniform":
                raise ValueError("uniform weighting over several ranks needs the per-rank client counts")
            counts = [rows.shape[0]]
        return self._clipped(ctx, rows, coeffs, out, center, int(sum(counts)))

    def _clipped(self, ctx, rows, coeffs, out, center, K_r: int):
        """The body for K_r reporting clients on all ranks; one without rows still reduces with the others."""
        G, P = rows.shape
        dev = out.device
        delta = self._tables.get(("delta", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
        cs = self._norms = None
        if G:
            rows, coeffs, cs = self._prepare(rows, coeffs, center, G, K_r, dev)
        self._reduce(ctx, rows, center, cs, delta)
        return self._finish(out, center, delta, K_r)

    def _prepare(self, rows, coeffs, center, G, K_r, dev):
        """-> (rows with unit inner stride, the weights in use, cs [G] = weight * clip factor)."""
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        if self.weighting == "uniform":
            coeffs = self._tables.get(("uniform", G, K_r, dev),
                                      lambda: torch.full((G,), 1.0 / K_r, dtype=torch.float32, device=dev))
        self._norms, cs = Fn.clip_scales(Fn.update_sqnorm(rows, center), coeffs, self.clip)
        return rows, coeffs, cs

    def _reduce(self, ctx, rows, center, cs, delta):
        """delta = the sum of the scaled updates over all ranks; cs None: this rank has no rows."""
        if cs is None:
            delta.zero_()
        else:
            Fn.clipped_sum(rows, center, cs, delta)
        self.cross_rank_sum(ctx, delta)

    def _finish(self, out, center, delta, K_r):
        std = self.noise_multiplier * self.clip / K_r if self.noise_multiplier > 0.0 and K_r else 0.0
        Fn.apply_update(out, center, delta, std, self.seed, self.rounds)
        self.rounds += 1
        self.last_k = K_r
        return out

    @property
    def last_norms(self) -> list[float]:
        """L2 norms of this rank's client updates in the last round, before clipping (syncs the
        device). +inf / nan mark a row that was dropped or too long for fp32."""
        return [] if self._norms is None else self._norms.tolist()

    def epsilon(self, N: int, delta: float) -> float:
        """(epsilon, delta)-DP spent so far on a population of N clients: q = K_r / N, the rounds
        aggregated so far, RDP accountant of ``fl/privacy.py`` (infinite without noise)."""
        from . import privacy
        if self.noise_multiplier <= 0.0:
            return math.inf
        return privacy.epsilon(self.rounds, min(1.0, self.last_k / N), self.noise_multiplier, delta)

    def state_dict(self) -> dict:
        return {"rounds": self.rounds, "last_k": self.last_k}

    def load_state_dict(self, sd: dict) -> None:
        self.rounds, self.last_k = int(sd["rounds"]), int(sd.get("last_k", 0))


class RobustLR(ClippedMean):
    """The robust learning rate, RLR (Ozdayi, Kantarcioglu, Gel, AAAI 2021) [north-star], a defence
    aimed at backdoors: per coordinate the reporting clients vote with the sign of their update,

        s_i = sum_k sgn(fl32(x_ki - c_i)),    theta_r = min(theta, K_r)
        out_i = c_i + lr_i * delta_i,         lr_i = -1 where |s_i| < theta_r, else +1

    with ``delta`` the clipped mean's sum: where fewer than theta_r clients (net) agree on a
    direction, the server moves against the aggregate instead of with it. Votes are unweighted, one
    per reporting client; K_r counts the reporting clients of all ranks, so a round thinned by
    dropout does not flip everything. ``theta = 0`` is exactly ``ClippedMean``.

    Everything else is ``ClippedMean``'s: the calling convention, norms, clip scales (``clip`` = inf
    by default: no clipping), a NaN / Inf row dropped with weight 0 (it does not vote either), the
    noise, the state. So the paper's RLR + clipping + noise costs what the clipped mean costs. The
    rule has no server step size of its own; it composes with a server optimizer like every
    ``takes_center`` rule.

    Two routes. One rank, ``fuse``: ``Fn.rlr_sum`` in final mode forms the sum and the votes and
    applies the flip in the clipped sum's single read of the rows, (G + 2) floats per coordinate.
    Several ranks, or ``fuse = False``: ``Fn.rlr_sum`` in partial mode, then ``delta`` and the votes
    each take the mean's cross-rank route (the votes are small integers in fp32: exact in any order),
    then ``Fn.rlr_flip``; a rank without rows contributes zeros to both. On one rank the two routes
    give the same bits.

    ``keep_votes`` (off by default): the fused route writes the votes too, ``last_votes`` is that
    device vector [P] (valid until the next call) and ``last_flipped`` counts the flipped
    coordinates when it is read -- the only host synchronisation."""
    name = "rlr"
    fuse = True         # the one-pass final mode on a single rank; off for A/B runs and tests
    keep_votes = False

    def __init__(self, theta: float, clip: float = math.inf, noise_multiplier: float = 0.0, seed: int = 0,
                 weighting: str = "samples", ordered: bool | None = None):
        super().__init__(clip, noise_multiplier, seed, weighting, ordered)
        self.theta = float(theta)
        if not self.theta >= 0.0:
            raise ValueError(f"theta must be >= 0, got {theta}")
        if self.noise_multiplier > 0.0 and not math.isfinite(self.clip):
            raise ValueError("noise_multiplier > 0 needs a finite clip: the noise is scaled by it")
        self.last_theta = 0.0  # theta_r of the last round
        self._votes = None

    def _clipped(self, ctx, rows, coeffs, out, center, K_r: int):
        G, P = rows.shape
        dev = out.device
        buf = lambda name: self._tables.get((name, P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
        delta = buf("delta")
        theta_r = self.last_theta = min(self.theta, float(K_r))
        cs = self._norms = None
        if G:
            rows, coeffs, cs = self._prepare(rows, coeffs, center, G, K_r, dev)
        fused = self.fuse and not ctx.is_distributed
        votes = buf("votes") if self.keep_votes or not fused else None
        if cs is None:  # no rows on this rank: zeros, which flip to zeros
            delta.zero_()
            if votes is not None:
                votes.zero_()
        else:
            Fn.rlr_sum(rows, center, cs, delta, votes, theta_r if fused else None)
        if not fused:
            self.cross_rank_sum(ctx, delta)
            self.cross_rank_sum(ctx, votes)
            Fn.rlr_flip(delta, votes, theta_r)
        self._votes = votes if self.keep_votes else None
        return self._finish(out, center, delta, K_r)

    @property
    def last_votes(self):
        """s [P] of the last round on the device, summed over all ranks (None without ``keep_votes``)."""
        return self._votes

    @property
    def last_flipped(self):
        """The coordinates the last round flipped (syncs the device; None without ``keep_votes``)."""
        return None if self._votes is None else int((self._votes.abs() < self.last_theta).sum())


class CenteredClip(ClippedMean):
    """Centered clipping (Karimireddy, He, Jaggi, ICML 2021) [north-star]: ``iters`` rounds of
    clipping *around a carried estimate of the aggregate update* ``v [P]`` (the last round's, zero
    at the start and each round with ``warm_start=False``), not around the server model:

        v^0 = v;   ctr^l = fl32(c + v^l)   (v^l itself without a centre)
        v^{l+1} = v^l + sum_k cs_k^l * fl32(x_k - ctr^l),   cs_k^l = w_k * min(1, tau / ||x_k - ctr^l||)
        out = ctr^L;   v <- v^L

    ``w_k`` as ``ClippedMean``'s ``weighting``; a row with a non-finite norm has cs = 0 for the whole
    round; ``last_norms`` are the first iteration's. No noise option.

    Two routes (``fuse``). Unfused, for any G, several ranks and the CPU, on the clipped mean's ops:
    per iteration update_sqnorm(rows, ctr) -> clip_scales -> clipped_sum into delta -> the mean's
    cross-rank route -> v += delta, ctr = c + v: (2G + 9) floats per coordinate. Fused, on one GPU
    with at most ``Fn.CC_MAX_ROWS`` rows: one norm pass, then one ``Fn.cc_step`` per iteration, which
    forms v and ctr and the next iteration's norms in a single read of the rows:
    (G + 1) + L (G + 5) floats. The routes fold the norm partials over different block partitions
    and add v at different points of the sum, so they agree to rounding, not bit for bit."""
    name = "centered_clip"
    fuse = True  # the fused step where it applies; off for A/B runs and tests

    def __init__(self, tau: float = 1.0, iters: int = 3, weighting: str = "samples",
                 warm_start: bool = True, ordered: bool | None = None):
        super().__init__(tau, 0.0, 0, weighting, ordered)
        self.tau, self.iters, self.warm_start = self.clip, int(iters), bool(warm_start)
        if self.iters < 0:
            raise ValueError(f"iters must be >= 0, got {iters}")
        self.v = None  # [P] on the device of the last call

    def _state(self, P, dev):
        if self.v is None or self.v.numel() != P:
            self.v = torch.zeros(P, dtype=torch.float32, device=dev)
        elif self.v.device != dev:
            self.v = self.v.to(dev)
        if not self.warm_start:
            self.v.zero_()
        return self.v

    def _clipped(self, ctx, rows, coeffs, out, center, K_r: int):
        G, P = rows.shape
        dev = out.device
        v = self._state(P, dev)
        self._norms = None
        if G:
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            if self.weighting == "uniform":
                coeffs = self._tables.get(("uniform", G, K_r, dev),
                                          lambda: torch.full((G,), 1.0 / K_r, dtype=torch.float32, device=dev))
        ctr = v
        if center is not None:  # ctr^0 = c + v^0; the last ctr goes to out, which may be the centre
            ctr = self._tables.get(("ctr", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
            Fn.apply_update(ctr, center, v)
        if self.fuse and not ctx.is_distributed and rows.is_cuda and 1 <= G <= Fn.CC_MAX_ROWS:
            sq = Fn.update_sqnorm(rows, ctr) if self.iters else None
            for l in range(self.iters):
                last = l == self.iters - 1
                norms, cs = Fn.clip_scales(sq, coeffs, self.tau)
                if l == 0:
                    self._norms = norms
                sq = Fn.cc_step(rows, center, ctr, v, cs, v, out if last and center is not None else ctr,
                                want_norms=not last)
        else:
            delta = self._tables.get(("delta", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
            for l in range(self.iters):
                cs = None
                if G:
                    norms, cs = Fn.clip_scales(Fn.update_sqnorm(rows, ctr), coeffs, self.tau)
                    if l == 0:
                        self._norms = norms
                self._reduce(ctx, rows, ctr, cs, delta)
                v.add_(delta)
                if center is not None:
                    Fn.apply_update(out if l == self.iters - 1 else ctr, center, v)
        if center is None or self.iters == 0:
            out.copy_(ctr)
        self.rounds += 1
        self.last_k = K_r
        return out

    def state_dict(self) -> dict:
        return {"rounds": self.rounds, "last_k": self.last_k,
                "v":None if self.v is None else self.v.detach().cpu().clone()}

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        v = sd.get("v")
        self.v = None if v is None else v.detach().clone().float()


class GeometricMedian(ClippedMean):
    """The geometric median by the smoothed Weiszfeld iteration (RFA: Pillutla, Kakade, Harchaoui
    2022) [north-star], in update space around the server model c, as ``CenteredClip`` works:

        v^0 = 0 (init="zero")   or   v^0 = sum_k a_k u_k / sum_k a_k (init="mean", the paper's)
        ctr^l = fl32(c + v^l)                                 (v^l itself without a centre)
        d_k^l = ||fl32(x_k - ctr^l)||_2                       (update_sqnorm: squares added in double)
        beta_k^l = a_k / max(nu, d_k^l);   b_k^l = beta_k^l / sum_j beta_j^l          (gm_scales)
        v^{l+1} = v^l + sum_k b_k^l * fl32(x_k - ctr^l)       (cc_step / clipped_sum)
        out = ctr^L,  L = iters

    ``a_k`` as ``ClippedMean``'s ``weighting``; a row whose squared norm is NaN / Inf has weight 0
    for the whole round. No noise, and no state between rounds beyond ``rounds`` / ``last_k``.

    The default start is the centre, not the paper's mean, because the rows may be hostile beyond
    any scale: one row of 1e30 puts the mean at 1e30 / K, from where every honest row is equally
    far and so equally weighted, and the first steps barely move (with 3e38 the mean is not even
    finite in fp32). Measured in float64 on 9 rows, 2 of them all 100, 1e30 or 3e38: from
    the mean the result is 1e39 honest radii away after 3 iterations; from the centre 0.65 radii
    after 1 iteration, 0.29 after 3, 0.28 after 8, the same for all three magnitudes -- a bad row's
    pull is b_k d_k ~ a_k / S, whatever its size. The server model is a point the honest updates
    are near by construction (they are one local epoch away from it).

    Routes, as ``CenteredClip`` (``fuse``). Fused (one GPU, 1 <= G <= ``Fn.CC_MAX_ROWS``):
    update_sqnorm once, then per iteration gm_scales -> ``Fn.cc_step``, which also forms the next
    iteration's squared norms: one read of the rows per iteration. Unfused (any G, several ranks,
    the CPU): per iteration update_sqnorm -> gm_scales -> clipped_sum into delta -> the mean's
    cross-rank route -> v += delta -> apply_update. Over several ranks the normaliser is global:
    each rank's ``beta_sum`` is all-gathered as [W] doubles and added in rank order on the device,
    then gm_scales runs again with that total; a rank without rows takes part with partial 0.
    With one client per rank the partials are the terms themselves, so the total has the bits of
    the single process holding the rows in rank order; otherwise the placements agree to rounding
    (the sum of doubles is associated differently). init="mean" is one more such step from v = 0
    with the scales a_k / sum a_j. No host synchronisation, except in ``last_norms`` / ``last_weights``.

    ``last_norms``: the distances of the round's first step (from the centre)."""
    name = "geomed"
    fuse = True

    def __init__(self, iters: int = 3, nu: float = 1e-6, weighting: str = "samples", init: str = "zero",
                 ordered: bool | None = None):
        super().__init__(math.inf, 0.0, 0, weighting, ordered)
        self.iters, self.nu = int(iters), float(nu)
        if self.iters < 0:
            raise ValueError(f"iters must be >= 0, got {iters}")
        if not self.nu > 0.0:
            raise ValueError(f"nu must be positive, got {nu}")
        if init not in ("zero", "mean"):
            raise ValueError(f"init must be 'zero' or 'mean', got {init!r}")
        self.init = init
        self._cs = None

    def _clipped(self, ctx, rows, coeffs, out, center, K_r: int):
        G, P = rows.shape
        dev = out.device
        v = self._tables.get(("gm_v", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
        v.zero_()
        self._norms = self._cs = None
        if G:
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            if self.weighting == "uniform":
                coeffs = self._tables.get(("uniform", G, K_r, dev),
                                          lambda: torch.full((G,), 1.0 / K_r, dtype=torch.float32, device=dev))
        ctr = v
        if center is not None:  # ctr^0 = c + 0; the last ctr goes to out, which may be the centre
            ctr = self._tables.get(("ctr", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
            Fn.apply_update(ctr, center, v)
        steps = [True] * (self.init == "mean") + [False] * self.iters  # True: the mean's scales
        n_steps = len(steps)
        if self.fuse and not ctx.is_distributed and rows.is_cuda and 1 <= G <= Fn.CC_MAX_ROWS:
            sq = Fn.update_sqnorm(rows, ctr) if n_steps else None
            for l, mean_step in enumerate(steps):
                last = l == n_steps - 1
                norms, self._cs, _ = Fn.gm_scales(sq, coeffs, self.nu, mean_step)
                if l == 0:
                    self._norms = norms
                sq = Fn.cc_step(rows, center, ctr, v, self._cs, v, out if last and center is not None else ctr,
                                want_norms=not last)
        else:
            delta = self._tables.get(("delta", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
            for l, mean_step in enumerate(steps):
                cs = sq = None
                part = torch.zeros(1, dtype=torch.float64, device=dev)
                if G:
                    sq = Fn.update_sqnorm(rows, ctr)
                    norms, cs, part = Fn.gm_scales(sq, coeffs, self.nu, mean_step)
                    if l == 0:
                        self._norms = norms
                if ctx.is_distributed:
                    parts = ctx.all_gather_rows(part)  # [W, 1] doubles, in rank order
                    total = parts[0].clone()
                    for w in range(1, parts.shape[0]):
                        total += parts[w]
                    if G:
                        _, cs, _ = Fn.gm_scales(sq, coeffs, self.nu, mean_step, total)
                self._cs = cs
                self._reduce(ctx, rows, ctr, cs, delta)
                v.add_(delta)
                if center is not None:
                    Fn.apply_update(out if l == n_steps - 1 else ctr, center, v)
        if center is None or n_steps == 0:
            out.copy_(ctr)
        self.rounds += 1
        self.last_k = K_r
        return out

    @property
    def last_weights(self) -> list[float]:
        """b_k of the last iteration for this rank's clients, exactly 0 for a dropped row (syncs
        the device)."""
        return [] if self._cs is None else self._cs.tolist()


class FLTrust(ClippedMean):
    """FLTrust (Cao, Fang, Liu, Gong, NDSS 2021) [north-star]: the server trains an update of its
    own on a small clean root dataset and judges every client against it, not against the others.
    With d_k = fl32(x_k - c) and the root update d_0 = fl32(root - c):

        cos_k  = clamp(<d_k, d_0> / (|d_k| |d_0|), -1, 1)          (root_dots: products added in double)
        beta_k = a_k * max(cos_k, 0);   T = sum_k beta_k over all ranks             (trust_scales)
        cs_k   = fl32(beta_k * (|d_0| / |d_k|) / T)                 every update rescaled to the root's norm
        out    = c + sum_k cs_k d_k                                 (clipped_sum, the mean's route, apply_update)

    ``a_k`` as ``ClippedMean``'s ``weighting`` ("uniform" is the paper's rule). A client whose update
    has a negative cosine with the server's is excluded -- IPM and sign-flip rows exactly, but an
    honest client on very different (non-IID) data too. The aggregate update is no longer than the
    root update, whatever the clients send. A row is dead (weight 0, ``last_cos`` NaN) when its
    squared norm or dot product is NaN / Inf or its update is zero, and every row is when the root
    update is; with T == 0 the model stays where it is and the round is counted. There is no ``f``
    to guess, no noise option, no state between rounds beyond ``rounds`` / ``last_k``.

    Per GPU: root_dots (one read of the rows) -> trust_scales -> clipped_sum into ``delta`` -> the
    mean's cross-rank route -> apply_update. Over several ranks the normaliser is global, as
    ``GeometricMedian``'s: each rank's ``beta_sum`` is all-gathered as [W] doubles and added in rank
    order on the device, then trust_scales runs again with that total; a rank without rows takes
    part with 0. No host synchronisation, except in the ``last_*`` properties.

    The caller supplies the root row: the FL engine does not train a server root yet."""
    name = "fltrust"
    needs_root = True

    def __init__(self, weighting: str = "samples", ordered: bool | None = None):
        super().__init__(math.inf, 0.0, 0, weighting, ordered)
        self._cos = self._cs = self._sq = self._root = None

    def __call__(self, ctx, rows: torch.Tensor, coeffs: torch.Tensor, out: torch.Tensor,
                 center: torch.Tensor | None = None, counts: list[int] | None = None,
                 root: torch.Tensor | None = None):
        """As ``ClippedMean``, plus root [P]: what the server trained from ``center`` on its root
        data (the root update itself without a centre)."""
        if root is None:
            raise ValueError("fltrust needs the server's root row (root=)")
        if root.dim() != 1 or root.numel() != rows.shape[1]:
            raise ValueError(f"fltrust: the root row must be [{rows.shape[1]}], got {tuple(root.shape)}")
        self._root = root
        try:
            return super().__call__(ctx, rows, coeffs, out, center, counts)
        finally:
            self._root = None

    def _clipped(self, ctx, rows, coeffs, out, center, K_r: int):
        G, P = rows.shape
        dev = out.device
        delta = self._tables.get(("delta", P, dev), lambda: torch.empty(P, dtype=torch.float32, device=dev))
        cs = self._norms = self._cos = self._cs = self._sq = None
        part = torch.zeros(1, dtype=torch.float64, device=dev)
        if G:
            if rows.stride(1) != 1:
                rows = rows.contiguous()
            if self.weighting == "uniform":
                coeffs = self._tables.get(("uniform", G, K_r, dev),
                                          lambda: torch.full((G,), 1.0 / K_r, dtype=torch.float32, device=dev))
            dots, self._sq = Fn.root_dots(rows, self._root.contiguous(), center)
            self._cos, self._norms, cs, part = Fn.trust_scales(dots, self._sq, coeffs)
        if ctx.is_distributed:
            parts = ctx.all_gather_rows(part)  # [W, 1] doubles, in rank order
            total = parts[0].clone()
            for w in range(1, parts.shape[0]):
                total += parts[w]
            if G:
                _, _, cs, _ = Fn.trust_scales(dots, self._sq, coeffs, total)
        self._cs = cs
        self._reduce(ctx, rows, center, cs, delta)
        return self._finish(out, center, delta, K_r)

    @property
    def last_cos(self) -> list[float]:
        """cos(d_k, d_0) of this rank's clients in the last round, NaN for a dead row (syncs the device)."""
        return [] if self._cos is None else self._cos.tolist()

    @property
    def last_trust(self) -> list[float]:
        """The trust scores max(cos_k, 0), exactly 0 for an excluded or dead row (syncs the device)."""
        return [] if self._cos is None else torch.nan_to_num(self._cos, nan=0.0).clamp_min(0.0).tolist()

    @property
    def last_weights(self) -> list[float]:
        """cs_k, what each of this rank's updates was multiplied by (syncs the device)."""
        return [] if self._cs is None else self._cs.tolist()

    @property
    def last_root_norm(self) -> float:
        """|d_0| of the last round, NaN on a rank that held no client (syncs the device)."""
        return math.nan if self._sq is None else float(self._sq[-1].sqrt())


class SecureMean(ClippedMean):
    """Secure aggregation (Bonawitz et al., CCS 2017) [north-star]: the clipped weighted mean, but
    the server only ever sees each client's update as fixed-point words under pairwise one-time
    masks that cancel in the sum (plus a self mask per client), and opens nothing but the sum.

    Per GPU: update_sqnorm -> clip_scales (a non-finite row gets weight 0) -> secagg_mask into a
    cached ``uploads [slots, P]`` int32 buffer: client i uploads rint(cs_i u_i 2^f) + masks mod 2^32,
    the masks taken against the round's *cohort* (everyone sampled, before dropout and deadline).
    One rank opens the uploads directly; several ranks sum theirs (secagg_sum), all-gather the int32
    partials and open the [W, P] stack on every rank. Opening removes the survivors' self masks and
    the pair masks the dropped clients left behind. The sums are integers mod 2^32, so the result
    has the same bits on any placement of the clients over ranks. apply_update then adds the centre
    and the (central) DP noise as in ``ClippedMean``.

    Key agreement and secret sharing are simulated: every mask is a pure function of (seed, round,
    pair, coordinate), so what is modelled is the arithmetic and its cost, not the cryptography.
    A round with fewer than ``min_survivors`` reporting clients is aborted: nothing is opened (a
    lone upload would be that client's plaintext), ``out`` becomes the centre (zero without one), the
    round counter still advances. The engine announces each round with ``begin_round``. Only the
    parameters are protected: the engine's BN buffers keep the plain mean."""
    name = "secagg"

    def __init__(self, frac_bits: int = 20, clip: float = math.inf, min_survivors: int = 2,
                 noise_multiplier: float = 0.0, seed: int = 0, weighting: str = "samples",
                 ordered: bool | None = None):
        super().__init__(clip, noise_multiplier, seed, weighting, ordered)
        self.frac_bits = int(frac_bits)
        if not Fn.SECAGG_BITS[0] <= self.frac_bits <= Fn.SECAGG_BITS[1]:
            raise ValueError(f"frac_bits must lie in {Fn.SECAGG_BITS[0]}..{Fn.SECAGG_BITS[1]}, got {frac_bits}")
        self.min_survivors = int(min_survivors)
        if self.min_survivors < 1:
            raise ValueError(f"min_survivors must be >= 1, got {min_survivors}")
        if self.noise_multiplier > 0.0 and not math.isfinite(self.clip):
            raise ValueError("noise_multiplier > 0 needs a finite clip: the noise is scaled by it")
        self.aborted: list[int] = []
        self._round = None     # (cohort, survivors, dropped, this rank's clients) of the announced round
        self._uploads: dict = {}
        self._last = self._sat = None

    def begin_round(self, cohort, survivors, clients) -> None:
        """The round's cohort (every sampled client), the survivors (those that report, on all
        ranks) and this rank's clients in slot order; host lists, the same on every rank but for
        the last."""
        cohort, survivors = Fn.secagg_ids(cohort, "cohort"), Fn.secagg_ids(survivors, "survivors")
        clients = Fn.secagg_ids(clients, "clients")
        if not set(survivors) <= set(cohort) or not set(clients) <= set(survivors):
            raise ValueError("secagg: clients must be survivors and survivors members of the cohort")
        alive = set(survivors)
        self._round = (cohort, survivors, [c for c in cohort if c not in alive], clients)

    def _table(self, ids, dev):
        return self._tables.get((tuple(ids), dev), lambda: torch.tensor(ids, dtype=torch.int32, device=dev))

    def abort_round(self, out: torch.Tensor | None = None, center: torch.Tensor | None = None):
        """Too few survivors: nothing is opened, the model stays, the round is counted."""
        if out is not None:
            if center is None:
                out.zero_()
            elif out is not center:
                out.copy_(center)
        self.aborted.append(self.rounds)
        self.rounds += 1
        self._round = self._last = self._sat = self._norms = None

    def __call__(self, ctx, rows: torch.Tensor, coeffs: torch.Tensor, out: torch.Tensor,
                 center: torch.Tensor | None = None, counts: list[int] | None = None):
        if self._round is None:
            raise RuntimeError("secagg: begin_round(cohort, survivors, clients) must announce the round")
        survivors, clients = self._round[1], self._round[3]
        G = rows.shape[0]
        if len(clients) != G:
            raise ValueError(f"secagg: {G} rows for the {len(clients)} clients announced")
        K_r = len(survivors)
        if counts is not None and int(sum(counts)) != K_r:
            raise ValueError(f"secagg: {int(sum(counts))} rows over the ranks for {K_r} survivors")
        if K_r < self.min_survivors:
            self.last_k = K_r
            self.abort_round(out, center)
            return out
        self._clipped(ctx, rows, coeffs, out, center, K_r)
        self._round = None
        return out

    def _reduce(self, ctx, rows, center, cs, delta):
        """The scaled updates go up masked; delta = what opening their sum over all ranks gives."""
        cohort, survivors, dropped, clients = self._round
        G, P = rows.shape
        dev = delta.device
        up = self._uploads.get((P, dev))
        if up is None or up.shape[0] < max(G, 1):
            up = self._uploads[(P, dev)] = torch.empty(max(G, 1), P, dtype=torch.int32, device=dev)
        self._last = self._sat = None
        if cs is not None:
            self._sat = torch.empty(G, dtype=torch.int32, device=dev)
            self._last = Fn.secagg_mask(rows, center, cs, self._table(clients, dev), self._table(cohort, dev),
                                        self.frac_bits, self.seed, self.rounds, up[:G], self._sat)
        words = up[:G]
        if ctx.is_distributed:
            part = torch.zeros(P, dtype=torch.int32, device=dev)
            if G:
                Fn.secagg_sum(words, part)
            words = ctx.all_gather_rows(part)
        Fn.secagg_open(words, self._table(survivors, dev), self._table(dropped, dev) if dropped else None,
                       self.frac_bits, self.seed, self.rounds, delta)

    @property
    def last_uploads(self):
        """What the server saw of this rank's clients in the last round: int32 [G, P] masked words
        (None for an aborted round or a rank without clients)."""
        return self._last

    @property
    def last_saturated(self) -> list[int]:
        """Per client of this rank, the coordinates that hit the fixed-point range or were NaN in
        the last round (syncs the device)."""
        return [] if self._sat is None else self._sat.tolist()

    def state_dict(self) -> dict:
        return {"rounds": self.rounds, "last_k": self.last_k, "aborted": list(self.aborted)}

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.aborted = [int(r) for r in sd.get("aborted", [])]


class _Sharded:
    """Helpers to move [G_i, P] client rows into coordinate shards [K, P/W] on every rank."""
    needs_all = True

    def shard(self, ctx, rows: torch.Tensor, counts: list[int]):
        """-> (X [K, S] client rows over this rank's S coordinates, rank-major; S; padded P).
        One GPU: the rows themselves (no copy). Several: ONE pack kernel builds the all-to-all send
        buffer (shards cut, zero-padded to the largest per-rank client count), and when every rank
        holds the same number of clients the receive buffer is used as is."""
        W = ctx.world
        K = sum(counts)
        P = rows.shape[1]
        if W == 1:
            return (rows if rows.stride(1) == 1 else rows.contiguous())[:K], P, P
        Pp = math.ceil(P / W) * W
        S = Pp // W
        gmax = max(counts)
        if rows.shape[0] and rows.stride(1) != 1:
            rows = rows.contiguous()
        send = Fn.pack_shards(rows, W, S, gmax)
        recv = torch.empty_like(send)
        ctx.all_to_all_single(recv, send)
        if all(c == gmax for c in counts):
            return recv.view(W * gmax, S), S, Pp
        valid = torch.cat([recv[i, :counts[i]] for i in range(W)], 0) if K else recv[:0, 0]
        return valid.contiguous(), S, Pp  # [K, S] rows ordered rank-major

    def unshard(self, ctx, part: torch.Tensor, P: int, Pp: int):
        if ctx.world == 1:
            return part[:P]
        full = torch.empty(Pp, dtype=torch.float32, device=part.device)
        ctx.all_gather_into(full, part.contiguous())
        return full[:P]


class Median(_Sharded):
    name = "median"

    def __call__(self, ctx, rows, counts, P, keys=None):
        shard, S, Pp = self.shard(ctx, rows, counts)
        return self.unshard(ctx, Fn.coord_select(shard, "median"), P, Pp)


class TrimmedMean(_Sharded):
    name = "trimmed_mean"

    def __init__(self, trim: int | float = 0.1):
        self.trim = trim

    def __call__(self, ctx, rows, counts, P, keys=None):
        K = sum(counts)
        b = int(self.trim * K) if isinstance(self.trim, float) and self.trim < 1 else int(self.trim)
        b = min(b, (K - 1) // 2)
        shard, S, Pp = self.shard(ctx, rows, counts)
        return self.unshard(ctx, Fn.coord_select(shard, "trimmed", b), P, Pp)


class Krum(_Sharded):
    """Krum (m=1) / multi-Krum (m>1) with f assumed Byzantine clients. A row with a NaN / Inf entry
    (or one large enough to overflow the fp32 Gram) is infinitely far from everyone and ranks last;
    m is clamped to the number of clients (``Fn.krum_select``)."""
    name = "krum"

    def __init__(self, f: int = 1, m: int = 1):
        self.f, self.m = f, m
        self._sel = None

    def __call__(self, ctx, rows, counts, P, keys=None):
        """keys: each (rank-major) row's global client order; exact score ties (a mutual-nearest
        pair always ties when nb = 1) go to the smaller key, so the choice does not depend on how
        the clients are spread over ranks. Default: the row index."""
        K = sum(counts)
        shard, S, Pp = self.shard(ctx, rows, counts)
        gram = Fn.gram(shard)
        if ctx.is_distributed:
            ctx.all_reduce(gram)
        nb = max(1, K - self.f - 2)
        m = min(max(1, self.m), K)  # multi-Krum with fewer clients than m averages them all
        if K <= Fn.MAX_ROBUST_CLIENTS:
            # scores, selection and the winners' mean on the device: krum_select + mean_rows_idx
            # (aggregate.hip), no torch sort / argsort / index_select glue
            _, sel = Fn.krum_select(gram.contiguous(), nb, m, keys)
            self._sel = sel  # stays on the device: no host sync per round (``last_selected`` reads it)
            return self.unshard(ctx, Fn.mean_rows_idx(shard, sel), P, Pp)
        # K > 128 only: the kernel's rules in torch (non-finite distances far, ties by key)
        _, order = Fn.krum_rank(gram, nb, m, keys)
        sel = torch.tensor(order, dtype=torch.long, device=gram.device)
        self._sel = sel
        chosen = shard.index_select(0, sel)
        part = torch.empty(chosen.shape[1], dtype=torch.float32, device=chosen.device)
        n_sel = sel.numel()  # one weight per row actually selected
        Fn.weighted_sum(chosen, torch.full((n_sel,), 1.0 / n_sel, dtype=torch.float32, device=chosen.device), part)
        return self.unshard(ctx, part, P, Pp)

    @property
    def last_selected(self) -> list[int]:
        """The clients (rank-major row order) the last round averaged (syncs the device)."""
        return [] if self._sel is None else self._sel.tolist()


class Bulyan(_Sharded):
    """Bulyan (El Mhamdi, Guerraoui, Rouault 2018) with f assumed Byzantine clients: theta = K - 2f
    clients picked by iterated Krum (``Fn.bulyan_select`` on the all-reduced Gram, redundantly on
    every GPU), then per coordinate the mean of the beta = theta - 2f picked values nearest their
    median (``Fn.bulyan_coord`` on this rank's coordinate shard, the picked rows read by index).

    The rule needs K >= 4f + 3, so per round f is clamped to max(0, (K - 3) // 4) (``last_f``), as
    ``TrimmedMean`` clamps its trim: a round thinned by dropout still aggregates. f = 0 is the
    plain mean of all rows, added in sorted order. At most ``Fn.MAX_ROBUST_CLIENTS`` clients a
    round (more raise ``ValueError``). No host synchronisation, except in ``last_selected``."""
    name = "bulyan"

    def __init__(self, f: int = 1):
        self.f = int(f)
        if self.f < 0:
            raise ValueError(f"f must be >= 0, got {f}")
        self.last_f = 0
        self._sel = None

    def __call__(self, ctx, rows, counts, P, keys=None):
        """keys: as ``Krum``'s, each (rank-major) row's global client order for exact score ties."""
        K = sum(counts)
        f = self.last_f = min(self.f, max(0, (K - 3) // 4))
        shard, S, Pp = self.shard(ctx, rows, counts)
        if K >= 3:
            gram = Fn.gram(shard)
            if ctx.is_distributed:
                ctx.all_reduce(gram)
            _, sel = Fn.bulyan_select(gram.contiguous(), f, keys)
        else:  # one or two clients: nothing to select, f = 0
            sel = torch.arange(K, dtype=torch.int32, device=shard.device)
        self._sel = sel  # stays on the device (``last_selected`` reads it)
        return self.unshard(ctx, Fn.bulyan_coord(shard, sel, K - 4 * f), P, Pp)

    @property
    def last_selected(self) -> list[int]:
        """The clients (rank-major row order) the last round picked, in order of selection (syncs
        the device)."""
        return [] if self._sel is None else self._sel.tolist()


def aggregate_into(agg, ctx, rows, coeffs, out, *, center, counts, keys, as_update: bool = False,
                   root=None) -> bool:
    """The one place that knows the aggregators' three calling conventions. rows [G_local, P] are
    the clients' vectors and ``center`` [P] what their updates are taken against (None: the rows
    are the updates already, FedSGD's gradients); counts / keys: the clients per rank and each
    rank-major row's global order (``_Sharded``, ``Krum``). The result goes to out [P]: the new
    vector (``center`` + the aggregate update), or with ``as_update`` what the rule itself forms
    without another rounding -- the robust rules' aggregate *update* (``(center + agg) - center``
    is not ``agg`` in fp32), the means' new vector. -> True when out holds an update.

      mean          agg(ctx, rows, coeffs, out)
      takes_center  agg(ctx, rows, coeffs, out, center=, counts=): the clipped mean forms the
                    updates, clips, averages and adds the centre back itself; a ``needs_root``
                    rule (``FLTrust``) also takes root=, the server's own row [P], which goes to
                    no other aggregator
      needs_all     agg(ctx, updates, counts, P, keys=) -> the aggregate update. The robust rules
                    act on updates; the new vector is added in place, so it needs ``out is center``"""
    if getattr(agg, "takes_center", False):
        kw = {"root": root} if getattr(agg, "needs_root", False) else {}
        agg(ctx, rows, coeffs, out, center=center, counts=counts, **kw)
        return False
    if not getattr(agg, "needs_all", False):
        agg(ctx, rows, coeffs, out)
        return False
    upd = rows if center is None else rows - center
    res = agg(ctx, upd, counts, out.numel(), keys=keys)
    if center is None or as_update:
        out.copy_(res)
        return True
    assert out is center, "a robust rule's update is added to the centre in place"
    out.add_(res)
    return False


def make_aggregator(name: str, **kw):
    name = name.lower()
    if name in ("mean", "fedavg", "avg"):
        return MeanAggregator()
    if name == "median":
        return Median()
    if name in ("trimmed", "trimmed_mean", "trimmedmean"):
        return TrimmedMean(kw.get("trim", 0.1))
    if name == "krum":
        return Krum(kw.get("f", 1), 1)
    if name in ("multikrum", "multi_krum"):
        return Krum(kw.get("f", 1), kw.get("m", 2))
    if name in ("clipped", "clipped_mean", "norm_clip"):
        return ClippedMean(kw.get("clip", 1.0), kw.get("noise_multiplier", 0.0), kw.get("seed", 0),
                           kw.get("weighting", "samples"))
    if name in ("rlr", "robust_lr"):
        return RobustLR(kw.get("theta", 0.0), kw.get("clip", math.inf), kw.get("noise_multiplier", 0.0),
                        kw.get("seed", 0), kw.get("weighting", "samples"))
    if name in ("centered_clip", "cc"):
        return CenteredClip(kw.get("tau", 1.0), kw.get("iters", 3), kw.get("weighting", "samples"),
                            kw.get("warm_start", True))
    if name == "bulyan":
        return Bulyan(kw.get("f", 1))
    if name in ("geomed", "rfa", "geometric_median"):
        return GeometricMedian(kw.get("gm_iters", 3), kw.get("gm_nu", 1e-6), kw.get("weighting", "samples"),
                               kw.get("init", "zero"))
    if name in ("fltrust", "fl_trust"):
        return FLTrust(kw.get("weighting", "samples"))
    if name in ("secagg", "secure", "secure_mean"):
        return SecureMean(kw.get("frac_bits", 20), kw.get("clip", math.inf), kw.get("min_survivors", 2),
                          kw.get("noise_multiplier", 0.0), kw.get("seed", 0), kw.get("weighting", "samples"))
    raise ValueError(f"unknown aggregator {name}")
