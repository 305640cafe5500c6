"""Per-client state banks: plain ``[N, P]`` fp32 tensors, row i for client i, kept between rounds
(``Scaffold.c_bank``, ``Compressor.bank``). Every rank holds the whole bank."""
import torch


def replicate_rows(ctx, bank: torch.Tensor, chosen, mine, slots: int) -> None:
    """The round's new rows onto every rank: rank w rewrote the rows of ``chosen[w::W]`` (``mine``
    here, at most ``slots``); they are all-gathered and written into every bank by client id
    (comm-bound: plain indexing). One collective on every rank, also on one without a client."""
    if not ctx.is_distributed:
        return
    dev = bank.device
    send = torch.zeros(slots, bank.shape[1], dtype=torch.float32, device=dev)
    if len(mine):
        send[:len(mine)] = bank[torch.as_tensor(mine, dtype=torch.int64, device=dev)]
    got = ctx.all_gather_rows(send)  # [W, slots, P]
    for w in range(ctx.world):
        theirs = [int(c) for c in chosen[w::ctx.world]]
        if theirs and w != ctx.rank:
            bank[torch.as_tensor(theirs, dtype=torch.int64, device=dev)] = got[w, :len(theirs)]


def bank_state(bank):
    """-> the bank's checkpoint entry: a CPU clone, None without a bank."""
    return None if bank is None else bank.detach().cpu().clone()


def load_bank(bank: torch.Tensor, saved: torch.Tensor, fix, what: str) -> None:
    """A checkpoint's rows through ``fix`` (the map to this run's parameter layout) into ``bank``."""
    if saved.shape[0] != bank.shape[0]:
        raise ValueError(f"checkpoint holds {saved.shape[0]} {what}, this federation has {bank.shape[0]} clients")
    bank.copy_(fix(saved).to(bank.device))
