"""Colluding attacks without a GPU: the torch twin against the float64 oracle
(tests/collude_oracle.py) on the cases of tests/test_collude_gpu.py, ALIE's z_max, and FedAvg under
ALIE over two gloo ranks against the single-process run."""
import os
import tempfile
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import collude_oracle as CO
import test_collude_gpu as G
import ddl25spring_amd.ops.reference as R
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl import attacks as AT
from ddl25spring_amd.fl.algorithms import FedAvg, FedSGD
from ddl25spring_amd.models import mnist_mlp
from ddl25spring_amd.models import params as P
from ddl25spring_amd.runtime.dist import DistContext

CPU = torch.device("cpu")


@pytest.fixture
def fp32(monkeypatch):
    monkeypatch.setattr(R, "_bf", lambda t: t.float())
    monkeypatch.setattr(P, "CPU_SHADOW_DTYPE", torch.float32)


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_on_hand_computed_cases():
    S = torch.tensor([[2.0, 1.0, float("nan")], [4.0, 1.0, float("inf")], [6.0, float("nan"), float("-inf")]])
    c = torch.tensor([1.0, 1.0, 0.0])
    mu, sigma, m = CO.moments(S, c)
    assert m.tolist() == [3, 2, 0] and mu.tolist() == [3.0, 0.0, 0.0]
    assert sigma[0] == np.sqrt(8.0 / 3.0) and sigma[1] == 0.0
    p, _ = CO.malicious(S, c, CO.ALIE, 2.0)
    assert p.tolist() == [3.0 - 2.0 * np.sqrt(8.0 / 3.0), 0.0, 0.0]
    p, _ = CO.malicious(S, c, CO.IPM, 0.5)
    assert p.tolist() == [-1.5, 0.0, 0.0]


# ------------------------------------------------------------------------------ CPU twin in ``Fn``
@pytest.mark.parametrize("ns", G.NS)
def test_collude_against_oracle_cpu(ns):
    G.check_against_oracle(ns, CPU)


def test_exact_cases_cpu():
    G.check_exact(CPU)


def test_hostile_sources_cpu():
    G.check_hostile(CPU)


def test_in_place_cpu():
    G.check_in_place(CPU)


def test_paths_and_two_calls_are_bit_equal_cpu():
    G.check_paths(CPU)


def test_second_grid_stride_iteration_cpu():
    G.check_second_pass(CPU)


def test_attack_classes_cpu():
    G.check_attack_classes(CPU)


def test_alie_z_max():
    for (n, f), z in {(8, 2): 0.318639, (10, 2): 0.253347, (10, 4): 0.841621, (100, 20): 0.495850}.items():
        assert abs(AT.alie_z_max(n, f) - z) <= 1e-6, (n, f)
    assert AT.alie_z_max(1, 1) == 0.0  # s clamps to 1 = n: no quantile left
    assert AT.ALIE([0], z=0.7).coef(8, 2) == 0.7 and AT.IPM([0]).coef(8, 2) == 0.5
    with pytest.raises(ValueError):
        AT.ALIE([0], knowledge="all")
    with pytest.raises(KeyError):
        AT.make_attack("min_max", [0])


def test_fedsgd_under_ipm_cancels_the_benign_gradient(fp32):
    arr = synthetic_images("mnist", 400, seed=0)
    parts = split(4, True, 1, labels=arr.labels)
    kw = dict(lr=0.05, client_fraction=1.0, seed=3)
    clean = FedSGD(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, **kw)
    clean.round()
    bad = FedSGD(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, attack=AT.IPM([0], eps=3.0), **kw)
    bad.round()
    # 3 benign gradients of weight 1/4 and one of -3 x their mean: the aggregate vanishes
    assert float(bad.g_global.norm()) <= 1e-5 * float(clean.g_global.norm())


# ------------------------------------------------------------------- 7: placement over two ranks
SEED, ROUNDS, BAD = 17, 5, [0, 1]
# the rounds of seed 17 (4 clients, 2 sampled, dropout 0.4): no colluder, a lone colluder (rank 1 holds
# no client), one of each, both colluders, one of each
REPORTING = [[3, 2], [1], [1, 2], [1, 0], [2, 1]]
# knowledge="own" runs without dropout: a lone reporter trains alone on a net built for two slots in
# the single process and for one slot on its rank, which the CPU training twins do not hold bit-equal
# (attack or not); under "benign" the lone colluder's trained row is discarded, so that round counts
DROPOUT = {"benign": 0.4, "own": 0.0}


def _fed(ctx, knowledge):
    arr = synthetic_images("mnist", 400, seed=0)
    parts = split(4, True, 7, labels=arr.labels)
    return FedAvg(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, lr=0.1, batch_size=50, client_fraction=0.5,
                  seed=SEED, ctx=ctx, dropout=DROPOUT[knowledge], attack=AT.ALIE(BAD, z=1.0, knowledge=knowledge))


def _cohorts(fa):
    """The cohorts a federation of this seed samples, replayed from a fresh generator."""
    rng = np.random.default_rng(fa.seed)
    return [[int(c) for c in rng.choice(fa.N, fa.K, replace=False)] for _ in range(ROUNDS)]


def _run(fa):
    seen = []
    for _ in range(ROUNDS):
        fa.round()
        seen.append(fa.w_global.clone())
    return torch.stack(seen)


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    for knowledge in ("benign", "own"):
        torch.save(_run(_fed(ctx, knowledge)), os.path.join(out_dir, f"{knowledge}{rank}.pt"))
    rdist.shutdown()


def spawn_with_timeout(fn, args, nprocs=2, limit=300.0):
    """mp.spawn that fails instead of waiting forever on a collective one rank never enters."""
    pc = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    end = time.monotonic() + limit
    while not pc.join(timeout=2.0):
        if time.monotonic() > end:
            for p in pc.processes:
                p.kill()
            pytest.fail(f"the ranks did not finish within {limit:.0f} s: a collective hangs")


def test_distributed_alie_fedavg_is_bit_identical_to_single_process(fp32):
    """One client per rank at most, so the ordered mean adds the same terms in the same order; the
    colluders' rows are computed from the gathered rows in the order of the round's sampling."""
    single = {}
    for knowledge in ("benign", "own"):
        fa = _fed(DistContext(), knowledge)
        single[knowledge] = _run(fa)
        if knowledge == "benign":
            survivors = [[c for c in ch if c not in gone] for ch, gone in zip(_cohorts(fa), fa.dropped)]
            assert survivors == REPORTING
        else:  # rounds with one source, and with two sources on two ranks
            assert {sum(c in BAD for c in ch) for ch in _cohorts(fa)} == {0, 1, 2}
    assert not torch.equal(single["benign"], single["own"])
    with tempfile.TemporaryDirectory() as d:
        port = 29650 + (os.getpid() % 100)
        spawn_with_timeout(_dist_worker, (2, port, d))
        for knowledge in ("benign", "own"):
            w0 = torch.load(os.path.join(d, f"{knowledge}0.pt"), weights_only=True)
            w1 = torch.load(os.path.join(d, f"{knowledge}1.pt"), weights_only=True)
            assert torch.equal(w0, w1)
            assert torch.equal(w0, single[knowledge]), knowledge
