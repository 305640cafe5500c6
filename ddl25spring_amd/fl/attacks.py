"""Simulated Byzantine clients [north-star: the course's announced Part 3 "Attacks & Defenses",
reference README.md:89-92 / lab/README.md:13-16, has no code].

* ``LabelFlip``     — data poisoning: y -> (C - 1 - y) on the malicious clients' batches.
* ``SignFlip``      — model poisoning: the malicious update is negated and scaled,
                      w_k <- w_g - s * (w_k - w_g).
* ``GaussianNoise`` — the malicious update is replaced by N(0, sigma^2) noise.
* ``FreeRider``     — sends back the server weights unchanged (no local work).
* ``ALIE`` / ``IPM`` — colluding model poisoning: every attacker sends the same vector, built from
                      the per-coordinate mean and std of other clients' updates (collude.hip).
* ``Backdoor``      — the targeted attack: trigger-stamped, relabelled copies in the malicious
                      clients' data, optionally boosted updates (model replacement).
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np
import torch

from ..ops import functional as Fn
from ..runtime.staging import DeviceTables


class Attack:
    def __init__(self, malicious: list[int] | set[int]):
        self.malicious = set(int(m) for m in malicious)

    def label_transform_for(self, slot_clients: list[int], num_classes: int):
        return None

    def poison_updates(self, rows: torch.Tensor, w_global: torch.Tensor, slot_clients: list[int]):
        pass

    def skip_training(self, client: int) -> bool:
        return False

    # RNG state of stochastic attacks, so a resumed run poisons exactly like an uninterrupted one
    def state_dict(self) -> dict:
        return {}

    def load_state_dict(self, sd: dict) -> None:
        pass


class LabelFlip(Attack):
    """Malicious clients train on labels y -> (num_classes - 1 - y). The per-slot flip mask lives
    in ONE persistent device buffer per (device, slot count): each round's transform refreshes it
    (``refresh``, also on its first eager call), so a captured round graph, which reads the buffer,
    replays correctly whichever slots the round's sampling put the attackers in."""

    def __init__(self, malicious):
        super().__init__(malicious)
        self._masks: dict = {}
        self._pinned: list = []  # sources of in-flight mask copies (bounded: trimmed below)

    def _trim(self):
        if len(self._pinned) > 64:
            del self._pinned[:32]  # copies enqueued 32+ rounds ago have long completed

    def label_transform_for(self, slot_clients, num_classes):
        bad = [i for i, c in enumerate(slot_clients) if c in self.malicious]
        if not bad:
            return None
        self._trim()
        n = len(slot_clients)
        mask_cpu = torch.zeros(n, dtype=torch.bool)
        mask_cpu[bad] = True
        fresh: set = set()

        def refresh(device):
            key = (torch.device(device), n)
            if key not in self._masks:
                self._masks[key] = torch.zeros(n, dtype=torch.bool, device=device)
            if key not in fresh:
                src = mask_cpu
                if self._masks[key].is_cuda:
                    # pinned + non-blocking: a pageable copy would make the host wait for the GPU
                    # to drain, serialising rounds that otherwise run unsynchronised (the source
                    # is never written again, so the in-flight copy is safe)
                    src = mask_cpu.pin_memory()
                    self._pinned.append(src)
                self._masks[key].copy_(src, non_blocking=True)
                fresh.add(key)
            return self._masks[key]

        def f(y, g0, g1):
            m = refresh(y.device)[g0:g1]
            return torch.where(m.reshape(-1, *([1] * (y.dim() - 1))), (num_classes - 1) - y, y)
        f.refresh = refresh
        # pure device ops on the persistent mask: a captured round replays it for any slot set
        f.graph_key = ("label_flip", n, num_classes)
        return f


class SignFlip(Attack):
    def __init__(self, malicious, scale: float = 1.0):
        super().__init__(malicious)
        self.scale = scale

    def poison_updates(self, rows, w_global, slot_clients):
        for i, c in enumerate(slot_clients):
            if c in self.malicious:
                rows[i].sub_(w_global).mul_(-self.scale).add_(w_global)


class GaussianNoise(Attack):
    def __init__(self, malicious, sigma: float = 1.0, seed: int = 0):
        super().__init__(malicious)
        self.sigma = sigma
        self.gen = None
        self.seed = seed

    def poison_updates(self, rows, w_global, slot_clients):
        for i, c in enumerate(slot_clients):
            if c in self.malicious:
                if self.gen is None:
                    self.gen = torch.Generator(device=rows.device).manual_seed(self.seed)
                noise = torch.randn(rows.shape[1], generator=self.gen, device=rows.device)
                rows[i].copy_(w_global + self.sigma * noise)

    def state_dict(self):
        return {"gen": None if self.gen is None else self.gen.get_state(),
                "device": None if self.gen is None else str(self.gen.device)}

    def load_state_dict(self, sd):
        if sd.get("gen") is None:
            self.gen = None
            return
        self.gen = torch.Generator(device=sd["device"])
        self.gen.set_state(sd["gen"])


class FreeRider(Attack):
    def skip_training(self, client):
        return client in self.malicious

    def poison_updates(self, rows, w_global, slot_clients):
        for i, c in enumerate(slot_clients):
            if c in self.malicious:
                rows[i].copy_(w_global)


class Colluding(Attack):
    """The colluders of a round all send ``center + p``, p a function of the per-coordinate mean and
    population std of the *source* updates u_k = fl32(x_k - center) (``Fn.collude_rows``: one
    streaming pass, moments in double, NaN / Inf entries skipped).

    ``knowledge`` names the sources: "benign" (omniscient, the default) the reporting clients that
    are not malicious; "own" (Baruch et al.'s setting) the reporting colluders' own honestly trained
    rows, which exist because every slot trains. No colluder reporting: nothing is done; no source
    row: the colluders send the centre.

    The engine announces each round with ``begin_round``; without it ``poison_updates`` takes the
    rows it is given as the whole round (one process). On several ranks the attack is *collective*:
    every rank calls it, also one without a client; the rows are all-gathered as a [slots, P] send
    buffer and visited in the order of the round's ``chosen`` list (position j lives at rank j % W,
    slot j // W), so every rank computes identical statistics and the malicious rows have the same
    bits however the clients are placed. Deterministic: no state, no host synchronisation."""
    collective = True
    mode = None  # "alie" | "ipm"

    def __init__(self, malicious, knowledge: str = "benign"):
        super().__init__(malicious)
        if knowledge not in ("benign", "own"):
            raise ValueError(f"knowledge must be 'benign' or 'own', got {knowledge!r}")
        self.knowledge = knowledge
        self._round = None
        self._tables = DeviceTables()

    def begin_round(self, ctx, chosen, mine) -> None:
        """The round's reporting clients of all ranks in sampling order, and this rank's in slot order."""
        self._round = (ctx, [int(c) for c in chosen], [int(c) for c in mine])

    def coef(self, n: int, f: int) -> float:
        """The mode's coefficient for n reporting clients, f of them colluders."""
        raise NotImplementedError

    def _table(self, ids, n_rows, dev):
        return self._tables.get((tuple(ids), n_rows, dev), lambda: Fn.collude_table(ids, n_rows, dev))

    def poison_updates(self, rows, w_global, slot_clients):
        ctx, chosen, mine = self._round or (None, [int(c) for c in slot_clients], [int(c) for c in slot_clients])
        self._round = None
        if mine != [int(c) for c in slot_clients]:
            raise ValueError("colluding attack: the rows are not those of the clients announced for the round")
        n, f = len(chosen), sum(c in self.malicious for c in chosen)
        if f == 0:
            return  # the same decision on every rank: chosen is
        is_src = (lambda c: c not in self.malicious) if self.knowledge == "benign" else (lambda c: c in self.malicious)
        W = ctx.world if ctx is not None and ctx.is_distributed else 1
        dev = rows.device
        src = rows
        if W > 1:
            # every rank's rows, as replicate_rows (fl/bank.py) moves them: one collective, also
            # on a rank without a client
            slots, P = math.ceil(n / W), rows.shape[1]
            send = torch.zeros(slots, P, dtype=torch.float32, device=dev)
            if len(mine):
                send[:len(mine)] = rows
            src = ctx.all_gather_rows(send).view(W * slots, P)
            where = lambda j: (j % W) * slots + j // W
        else:
            where = lambda j: j
        src_rows = [where(j) for j, c in enumerate(chosen) if is_src(c)]
        dst_rows = [g for g, c in enumerate(mine) if c in self.malicious]
        if not dst_rows:
            return
        Fn.collude_rows(src, self._table(src_rows, src.shape[0], dev), w_global, rows,
                        self._table(dst_rows, rows.shape[0], dev), self.mode, self.coef(n, f))


def alie_z_max(n: int, f: int) -> float:
    """The largest z for which ALIE's ``mu - z * sigma`` still finds enough benign support (Baruch et
    al. 2019): z_max = Phi^-1((n - s) / n), s = floor(n / 2 + 1) - f clamped to at least 1."""
    s = max(1, n // 2 + 1 - f)
    q = (n - s) / n
    return NormalDist().inv_cdf(q) if 0.0 < q < 1.0 else 0.0


class ALIE(Colluding):
    """"A Little Is Enough" (Baruch et al. 2019): p = mu - z * sigma per coordinate, inside the
    spread a robust rule tolerates. ``z`` None: ``alie_z_max`` of the round's n and f."""
    mode = "alie"

    def __init__(self, malicious, z: float | None = None, knowledge: str = "benign"):
        super().__init__(malicious, knowledge)
        self.z = None if z is None else float(z)

    def coef(self, n, f):
        return alie_z_max(n, f) if self.z is None else self.z


class IPM(Colluding):
    """Inner-product manipulation (Xie et al. 2019): p = -eps * mu."""
    mode = "ipm"

    def __init__(self, malicious, eps: float = 0.5, knowledge: str = "benign"):
        super().__init__(malicious, knowledge)
        self.eps = float(eps)

    def coef(self, n, f):
        return self.eps


class Backdoor(Attack):
    """The targeted attack (Gu et al. 2017 BadNets; in FL Bagdasaryan et al. 2020): the malicious
    clients train on copies of their own samples that carry a trigger, a ``patch`` x ``patch``
    square of ``value`` in the bottom-right corner of every channel, labelled ``target``. The server
    model keeps its accuracy on clean inputs and sends an input with the trigger to ``target``; the
    accuracy on ``triggered_test`` is the attack success rate (ASR).

    The poisoning is done on the host arrays before the device dataset is built (``poison``), so the
    training step, its captured graph and the planners are those of a clean run, whatever the model,
    precision or algorithm. ``boost`` != 1 is model replacement: a malicious row is sent as
    ``w_g + boost * (w_k - w_g)``, to survive the average with the honest rows. No state."""

    def __init__(self, malicious, target: int = 0, poison_fraction: float = 0.5, patch: int = 4,
                 value: int = 255, boost: float = 1.0, seed: int = 0):
        super().__init__(malicious)
        self.target, self.patch, self.value = int(target), int(patch), int(value)
        self.poison_fraction, self.boost, self.seed = float(poison_fraction), float(boost), int(seed)
        if not 0.0 <= self.poison_fraction <= 1.0:
            raise ValueError(f"poison_fraction must lie in [0, 1], got {poison_fraction}")
        if self.patch < 1:
            raise ValueError(f"patch must be >= 1, got {patch}")
        if not 0 <= self.value <= 255:
            raise ValueError(f"value must be a uint8 pixel, got {value}")
        if self.target < 0:
            raise ValueError(f"target must be a class index, got {target}")

    def stamp(self, images: np.ndarray) -> np.ndarray:
        """uint8 [n, H, W, C] -> a copy with the trigger in the bottom-right corner of every channel."""
        out = np.array(images, dtype=np.uint8, copy=True)
        out[:, -self.patch:, -self.patch:, :] = self.value
        return out

    def poison(self, arrays, client_indices):
        """-> (arrays', client_indices'). For every malicious client m, round(poison_fraction * n_m)
        of its samples with a label other than ``target`` (fewer when it has fewer), drawn with
        ``default_rng([seed, 0xBD, m])``, are replaced in its index array by stamped copies labelled
        ``target``, which are appended after the original rows. The first len(arrays) rows, the
        benign clients' indices and every n_k stay. A pure function of the arguments: the ranks of a
        distributed run build identical datasets."""
        from ..data.images import ImageArrays
        parts = [np.array(c, dtype=np.int64, copy=True) for c in client_indices]
        images, nxt = [arrays.images], len(arrays)
        for m in sorted(self.malicious):
            if not 0 <= m < len(parts):
                continue
            idx = parts[m]
            rng = np.random.default_rng([self.seed, 0xBD, m])
            cand = np.flatnonzero(arrays.labels[idx] != self.target)
            k = min(int(round(self.poison_fraction * len(idx))), len(cand))
            pick = np.sort(rng.choice(cand, k, replace=False))  # positions in the client's index array
            images.append(self.stamp(arrays.images[idx[pick]]))
            idx[pick] = np.arange(nxt, nxt + k)
            nxt += k
        labels = np.concatenate([arrays.labels, np.full(nxt - len(arrays), self.target, dtype=arrays.labels.dtype)])
        return ImageArrays(np.concatenate(images), labels, arrays.kind, arrays.synthetic), parts

    def triggered_test(self, arrays):
        """The samples whose true label is not ``target``, stamped and labelled ``target``."""
        from ..data.images import ImageArrays
        keep = arrays.labels != self.target
        return ImageArrays(self.stamp(arrays.images[keep]),
                           np.full(int(keep.sum()), self.target, dtype=arrays.labels.dtype),
                           arrays.kind, arrays.synthetic)

    def poison_updates(self, rows, w_global, slot_clients):
        if self.boost == 1.0:
            return
        for i, c in enumerate(slot_clients):
            if c in self.malicious:
                if w_global is None:  # gradients without a centre: the row is the update
                    rows[i].mul_(self.boost)
                else:
                    rows[i].sub_(w_global).mul_(self.boost).add_(w_global)


def make_attack(name: str | None, malicious, **kw):
    if not name or name == "none":
        return None
    return {"label_flip": LabelFlip, "sign_flip": SignFlip, "gaussian": GaussianNoise,
            "free_rider": FreeRider, "alie": ALIE, "ipm": IPM, "backdoor": Backdoor}[name](malicious, **kw)
