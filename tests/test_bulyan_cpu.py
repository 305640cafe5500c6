"""Bulyan without a GPU: the oracle's window rule against brute force, the torch twins against the
float64 oracle on the cases of tests/test_bulyan_gpu.py, and ``Bulyan`` in a FedAvg over two gloo ranks."""
import os
import tempfile

import pytest
import torch

import bulyan_oracle as B
import test_bulyan_gpu as G
import ddl25spring_amd.ops.reference as R
from test_collude_cpu import spawn_with_timeout
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.algorithms import FedAvg
from ddl25spring_amd.fl.attacks import ALIE
from ddl25spring_amd.models import mnist_mlp
from ddl25spring_amd.models import params as P
from ddl25spring_amd.runtime.dist import DistContext

CPU = torch.device("cpu")


@pytest.fixture
def fp32(monkeypatch):
    monkeypatch.setattr(R, "_bf", lambda t: t.float())
    monkeypatch.setattr(P, "CPU_SHADOW_DTYPE", torch.float32)


# ------------------------------------------------------------ 1: the window rule, oracle only
@pytest.mark.parametrize("K,f", G.WINDOW_KF)
def test_window_rule_is_the_values_nearest_the_median(K, f):
    """The count definition picks "the beta values closest to the median, an exact tie going to the
    lower value": the same values as sorting by (|s_i - med|, i) and taking beta, difference 0.0."""
    g = torch.Generator().manual_seed(K)
    theta = K - 2 * f
    beta = theta - 2 * f
    for name in ("randn", "ties"):
        X = torch.randn(theta, 515, generator=g) if name == "randn" else \
            torch.randint(-2, 3, (theta, 515), generator=g).float()
        s = torch.sort(X.double(), 0).values
        a, b = B.window(s, beta).mean(0), B.window_brute(s, beta).mean(0)
        assert float((a - b).abs().max()) == 0.0, (K, f, name)
        lo = B.window_lo(s, beta)
        assert int(lo.min()) >= 0 and int(lo.max()) <= theta - beta
        if name == "randn":
            assert len(set(lo.tolist())) > 1  # the window does move


# ---------------------------------------------------------------------- 2 - 5: the CPU twins
@pytest.mark.parametrize("K,f", G.COORD_KF)
def test_bulyan_coord_sweep_cpu(K, f):
    G.check_coord_sweep(K, f, CPU)


def test_bulyan_coord_second_wave_and_tail_cpu():
    G.check_coord_big(CPU)


@pytest.mark.parametrize("K", G.SELECT_K)
def test_bulyan_select_exact_gram_cpu(K):
    G.check_select_exact(K, CPU)


@pytest.mark.parametrize("kind", G.O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K,f", G.ATTACK_KF)
def test_bulyan_under_attack_cpu(K, f, kind):
    G.check_attack(K, f, kind, CPU)


def test_bulyan_clamp_and_errors_cpu():
    G.check_clamp_and_errors(CPU)


# ------------------------------------------------------------------------ 6: two gloo ranks
ROUNDS = 3


def _fed(ctx):
    arr = synthetic_images("mnist", 800, seed=0)
    parts = split(8, True, 7, labels=arr.labels)
    return FedAvg(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, lr=0.1, batch_size=50, client_fraction=1.0,
                  seed=17, ctx=ctx, aggregator="bulyan", agg_kwargs={"f": 1}, attack=ALIE([0]))


def _run(fa):
    """-> (w_global, per round the picked clients as positions in the round's sampling order)."""
    picked = []
    for _ in range(ROUNDS):
        fa.round()
        keys = fa._row_keys(fa._counts)
        picked.append(sorted(keys[r] for r in fa.aggregator.last_selected))
    return fa.w_global, picked


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    w, picked = _run(_fed(ctx))
    torch.save({"w": w, "picked": picked}, os.path.join(out_dir, f"r{rank}.pt"))
    rdist.shutdown()


def test_distributed_bulyan_fedavg_matches_single_process(fp32):
    w, picked = _run(_fed(DistContext()))
    assert all(len(p) == 6 for p in picked)
    with tempfile.TemporaryDirectory() as d:
        port = 29850 + (os.getpid() % 100)
        spawn_with_timeout(_dist_worker, (2, port, d))
        r0 = torch.load(os.path.join(d, "r0.pt"), weights_only=True)
        r1 = torch.load(os.path.join(d, "r1.pt"), weights_only=True)
    assert torch.equal(r0["w"], r1["w"])  # replicated server state stays identical on every rank
    assert torch.allclose(r0["w"], w, atol=1e-5), (r0["w"] - w).abs().max()
    assert r0["picked"] == picked and r1["picked"] == picked
