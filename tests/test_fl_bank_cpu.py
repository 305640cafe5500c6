"""The federated engine's shared host-side pieces without a GPU: per-client bank replication over
two gloo ranks and its checkpoint load (fl/bank.py), the device-table cache and the pinned stager
(runtime/staging.py)."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ddl25spring_amd.fl.bank import bank_state, load_bank, replicate_rows
from ddl25spring_amd.runtime.dist import DistContext
from ddl25spring_amd.runtime.staging import DeviceTables, PinnedStager

N, P, W = 5, 7, 2
# K = 3: counts [2, 1]; K = 1: rank 1 holds no client and still takes part in the collective
CASES = {"k3": [4, 0, 2], "k1": [3]}


def _sentinel():
    """[N, P] fp32 whose every entry is its own quiet-NaN bit pattern: a row that is touched, or
    rounded on the way, shows."""
    bits = 0x7FC00000 + 256 * torch.arange(N, dtype=torch.int32)[:, None] + torch.arange(P, dtype=torch.int32)
    return bits.view(torch.float32).clone()


def _new_row(client: int):
    """What client's holder writes into its row this round: a function of the client alone."""
    return torch.arange(P, dtype=torch.float32) * 0.25 - (client + 1)


def _expected(chosen):
    bank = _sentinel()
    for c in chosen:
        bank[c] = _new_row(c)
    return bank


def _bits(t):
    return t.contiguous().view(torch.int32)


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(W))
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    out = {}
    for name, ids in CASES.items():
        chosen = np.asarray(ids)
        mine = [int(c) for c in chosen[rank::W]]
        bank = _sentinel()
        for c in mine:
            bank[c] = _new_row(c)
        replicate_rows(ctx, bank, chosen, mine, -(-len(ids) // W))
        out[name] = _bits(bank)
    torch.save(out, os.path.join(out_dir, f"b{rank}.pt"))
    rdist.shutdown()


def test_replicate_rows_on_two_ranks():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(29100 + os.getpid() % 100, d), nprocs=W, join=True)
        got = [torch.load(os.path.join(d, f"b{r}.pt"), weights_only=True) for r in range(W)]
    for name, ids in CASES.items():
        want = _bits(_expected(ids))
        assert torch.equal(got[0][name], got[1][name]), name       # both ranks hold the same bank
        assert torch.equal(got[0][name], want), name               # ... the single process's
        rest = [c for c in range(N) if c not in ids]
        assert torch.equal(got[0][name][rest], _bits(_sentinel())[rest]), name  # unchosen rows keep their bits


def test_replicate_rows_is_a_no_op_in_one_process():
    bank = _expected(CASES["k3"])
    replicate_rows(DistContext(), bank, np.asarray(CASES["k3"]), CASES["k3"], 3)
    assert torch.equal(_bits(bank), _bits(_expected(CASES["k3"])))


def test_load_bank_checks_the_rows_and_applies_the_fix():
    bank = torch.zeros(N, P)
    saved = torch.arange(N * P, dtype=torch.float32).reshape(N, P)
    for what in ("control variates", "error rows"):
        with pytest.raises(ValueError) as e:
            load_bank(bank, saved[:N - 1], lambda t: t, what)
        assert str(e.value) == f"checkpoint holds {N - 1} {what}, this federation has {N} clients"
    assert not bank.any()
    load_bank(bank, saved, lambda t: t.flip(1), "error rows")  # a layout map: every row reversed
    assert torch.equal(bank, saved.flip(1))
    state = bank_state(bank)
    assert torch.equal(state, bank) and state.data_ptr() != bank.data_ptr() and bank_state(None) is None


def test_device_tables_cache_and_cap():
    tables = DeviceTables()
    built = []

    def table(i):
        def build():
            built.append(i)
            return torch.tensor([i, i + 1], dtype=torch.int32)
        return tables.get(("ids", i), build)
    first = table(0)
    assert table(0) is first and built == [0]
    for i in range(1, 256):
        table(i)
    assert len(tables) == 256
    over = table(256)  # the 257th distinct key: right values, not stored, built again on the next call
    assert over.tolist() == [256, 257] and len(tables) == 256
    assert table(256) is not over and built.count(256) == 2
    assert table(0) is first and table(255).tolist() == [255, 256] and built.count(255) == 1


def test_pinned_stager_on_the_cpu():
    cpu = torch.device("cpu")
    stager = PinnedStager((4,), torch.int32)
    out = torch.full((4,), -1, dtype=torch.int32)
    stager.put(np.array([5, 6, 7, 8], dtype=np.int32), out[:4])
    assert out.tolist() == [5, 6, 7, 8]
    stager.put(np.array([1, 2], dtype=np.int32), out[:2])  # a shorter table: the rest stays
    assert out.tolist() == [1, 2, 7, 8]
    plan = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    fresh = PinnedStager(plan.shape, torch.int32).put(plan, cpu)
    assert fresh.dtype == torch.int32 and fresh.device == cpu and np.array_equal(fresh.numpy(), plan)
