"""Server-side optimizers for FedAvg under client drift [north-star; absent from the reference]:
FedOpt (Reddi et al. 2021, Algorithm 2) treats the round's aggregate update
``delta = aggregate - w_global`` as a pseudo-gradient and steps the server model with

* ``fedavgm``    — server momentum (Hsu et al. 2019): m = b1 m + delta, w += lr m;
* ``fedadagrad`` — m = b1 m + (1 - b1) delta, v = v + delta^2;
* ``fedadam``    — v = b2 v + (1 - b2) delta^2;
* ``fedyogi``    — v = v - (1 - b2) delta^2 sign(v - delta^2);
  the three adaptive rules then take w += lr m / (sqrt(v) + tau), without bias correction.

``m`` starts at 0 and ``v`` at tau^2 (the paper requires v_{-1} >= tau^2). The state is two flat
rows [P] allocated on first use; one streaming kernel updates w, m, v in place (fedopt.hip), and on
one GPU with a plain mean the weighted client sum is fused into the same launch (``step_rows``). On
several ranks m, v are replicated: every rank steps the identical aggregate identically.
"""
from __future__ import annotations

import torch

from ..ops import functional as Fn

NAMES = {"fedavgm": "sgdm", "fedadagrad": "adagrad", "fedadam": "adam", "fedyogi": "yogi"}


class ServerOptimizer:
    def __init__(self, kind: str, lr: float, beta1: float = 0.9, beta2: float = 0.99, tau: float = 1e-3):
        if kind not in Fn.SERVER_OPT_KINDS:
            raise ValueError(f"server optimizer kind must be one of {sorted(Fn.SERVER_OPT_KINDS)}, got {kind!r}")
        self.kind = kind
        self.lr, self.beta1, self.beta2, self.tau = float(lr), float(beta1), float(beta2), float(tau)
        if not self.lr > 0.0:
            raise ValueError(f"server lr must be positive, got {lr}")
        if not self.tau > 0.0:
            raise ValueError(f"tau must be positive, got {tau}")
        if not (0.0 <= self.beta1 < 1.0 and 0.0 <= self.beta2 < 1.0):
            raise ValueError(f"beta1, beta2 must lie in [0, 1), got {beta1}, {beta2}")
        self.m = None
        self.v = None
        self.steps = 0

    @property
    def has_v(self) -> bool:
        return self.kind != "sgdm"

    def _state(self, w: torch.Tensor):
        if self.m is None:
            self.m = torch.zeros_like(w)
            if self.has_v:  # tau * tau rounded to fp32 once, the same value on every device
                v0 = (torch.tensor(self.tau, dtype=torch.float32) * torch.tensor(self.tau, dtype=torch.float32)).item()
                self.v = torch.full_like(w, v0)
        if self.m.shape != w.shape or self.m.device != w.device:
            raise ValueError("server optimizer state does not match the server model")

    def step(self, w: torch.Tensor, x: torch.Tensor, x_is_delta: bool = False) -> torch.Tensor:
        """w [P] in place; x is the aggregate model, or the aggregate update with ``x_is_delta``."""
        self._state(w)
        Fn.server_opt_step(w, x, self.m, self.v, self.kind, x_is_delta, self.lr, self.beta1, self.beta2, self.tau)
        self.steps += 1
        return w

    def step_rows(self, rows: torch.Tensor, coeffs: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """The same step on the weighted mean of the client rows [G, P], formed inside the kernel:
        bit-equal to ``weighted_sum`` into a temporary followed by ``step``."""
        self._state(w)
        Fn.server_opt_rows(rows, coeffs, w, self.m, self.v, self.kind, self.lr, self.beta1, self.beta2, self.tau)
        self.steps += 1
        return w

    def state_dict(self) -> dict:
        sd = {"kind": self.kind, "lr": self.lr, "beta1": self.beta1, "beta2": self.beta2, "tau": self.tau,
              "steps": self.steps}
        for name in ("m", "v"):
            t = getattr(self, name)
            sd[name] = None if t is None else t.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd: dict, like: torch.Tensor | None = None, fix=None) -> None:
        """``like``: the server model (device and shape of the state); ``fix`` remaps a flat row
        written with another parameter layout."""
        if sd["kind"] != self.kind:
            raise ValueError(f"checkpoint holds a {sd['kind']!r} server optimizer, this one is {self.kind!r}")
        self.steps = int(sd.get("steps", 0))
        for name in ("m", "v"):
            t = sd.get(name)
            if t is None:
                setattr(self, name, None)
                continue
            t = t if fix is None else fix(t)
            t = t.to(torch.float32)
            if like is not None:
                if t.shape != like.shape:
                    raise ValueError("server optimizer state does not match the server model")
                t = t.to(like.device)
            setattr(self, name, t.contiguous().clone())


def make_server_opt(name: str, **kw) -> ServerOptimizer:
    """``fedavgm | fedadagrad | fedadam | fedyogi`` (+ lr, beta1, beta2, tau)."""
    kind = NAMES.get(str(name).lower())
    if kind is None:
        raise ValueError(f"unknown server optimizer {name!r} (one of {sorted(NAMES)})")
    kw = dict(kw)
    kw.setdefault("lr", 1.0 if kind == "sgdm" else 0.01)
    return ServerOptimizer(kind, **kw)
