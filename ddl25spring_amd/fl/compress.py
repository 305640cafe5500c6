"""Compressed client uploads with error feedback [north-star; absent from the reference].

A reporting client's update passes through a lossy codec before the server sees it, and what the
codec dropped is kept per client and added back in that client's next round (error feedback: Stich
et al. 2018; Karimireddy et al. 2019). The clients are slots of one GPU, so the codec works in
place (csrc/kernels/compress.hip): slot g's trained row becomes what the server would decode,
``x + q(u)`` with ``u = (y_g - x) + e_i``, and every aggregator, server optimizer and attack then
works behind it unchanged.

  * ``TopK(ratio)``: the ``k = max(1, round(ratio * P))`` largest magnitudes of u (ties kept), sent
    as fp32 value + int32 index: 8 bytes each;
  * ``Quantize(bits, seed)``: QSGD-style stochastic levels in ``[-L, L]``, ``L = 2^(bits-1) - 1``,
    with one fp32 scale per bucket of 256 columns: ``ceil(P * bits / 8) + 4 * ceil(P / 256)`` bytes.

The error bank ``[N, P]`` is fp32, zero at the start, one row per client, kept between rounds like
``Scaffold.c_bank``; with ``error_feedback=False`` there is none and the dropped part is lost.
"""
from __future__ import annotations

import math

import torch

from ..ops import functional as Fn
from .bank import bank_state, load_bank

BUCKET = 256


def dense_bytes(P: int) -> int:
    return 4 * P


class Compressor:
    name = "none"

    def __init__(self, error_feedback: bool = True):
        self.error_feedback = bool(error_feedback)
        self.bank = None  # [N, P] once bound
        self.round = 0    # codec calls so far (keys the quantizer's draws)
        self.last_nnz = None

    def bind(self, n_clients: int, P: int, slots: int, dev) -> None:
        """Allocate the per-federation state: the error bank and the per-slot counters."""
        self.N, self.P = n_clients, P
        self.bank = torch.zeros(n_clients, P, dtype=torch.float32, device=dev) if self.error_feedback else None
        self._nnz = torch.zeros(max(1, slots), dtype=torch.int32, device=dev)

    def apply(self, rows, x, slot_client):
        """rows [G, P] (the trained slots) -> what the server decodes, in place; the bank rows of
        the clients slot_client [G] (int32, on the rows' device, validated where it was built) take
        the residual. -> nnz [G] int32 on the device for codecs that count, else None. No host
        synchronisation."""
        nnz = self._encode(rows, x, slot_client)
        self.round += 1
        self.last_nnz = nnz
        return nnz

    def skip(self) -> None:
        """A round in which this rank holds no reporting client: it still counts."""
        self.round += 1

    def uplink_bytes(self, P: int, nnz: int | None = None) -> int:
        raise NotImplementedError

    def state_dict(self) -> dict:
        return {"name": self.name, "round": self.round, "bank": bank_state(self.bank)}

    def load_state_dict(self, sd: dict, fix=lambda t: t) -> None:
        if sd["name"] != self.name or (sd["bank"] is None) != (self.bank is None):
            raise ValueError(f"checkpoint holds compressor state of {sd['name']!r} "
                             f"(bank: {sd['bank'] is not None}), this run uses {self.name!r} "
                             f"(bank: {self.bank is not None})")
        self.round = int(sd["round"])
        if self.bank is not None:
            load_bank(self.bank, sd["bank"], fix, "error rows")


class TopK(Compressor):
    name = "topk"

    def __init__(self, ratio: float, error_feedback: bool = True):
        if not 0.0 < ratio <= 1.0:
            raise ValueError(f"TopK: ratio must lie in (0, 1], got {ratio}")
        super().__init__(error_feedback)
        self.ratio = float(ratio)

    def k(self, P: int) -> int:
        return max(1, round(self.ratio * P))

    def _encode(self, rows, x, slot_client):
        G = rows.shape[0]
        return Fn.topk_compress(rows, x, self.bank, slot_client, self.k(rows.shape[1]), self._nnz[:G])

    def uplink_bytes(self, P: int, nnz: int | None = None) -> int:
        return 8 * int(self.k(P) if nnz is None else nnz)


class Quantize(Compressor):
    name = "quant"

    def __init__(self, bits: int, seed: int = 0, error_feedback: bool = True):
        if not 2 <= int(bits) <= 8:
            raise ValueError(f"Quantize: bits must lie in 2..8, got {bits}")
        super().__init__(error_feedback)
        self.bits, self.seed = int(bits), int(seed)

    def _encode(self, rows, x, slot_client):
        Fn.quantize_compress(rows, x, self.bank, slot_client, self.bits, self.seed, self.round)
        return None

    def uplink_bytes(self, P: int, nnz: int | None = None) -> int:
        return math.ceil(P * self.bits / 8) + 4 * math.ceil(P / BUCKET)


COMPRESSORS = {"topk": TopK, "quant": Quantize}


def make_compressor(name: str, **kw) -> Compressor:
    if name not in COMPRESSORS:
        raise ValueError(f"compressor must be one of {sorted(COMPRESSORS)}, got {name!r}")
    return COMPRESSORS[name](**kw)
