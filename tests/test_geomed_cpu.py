"""The geometric median / RFA without a GPU: the torch twins against the float64 oracle on the cases
of tests/test_geomed_gpu.py, ``GeometricMedian`` through a FedAvg checkpoint, over two gloo ranks, and
both new rules through the CLI."""
import os
import tempfile

import pytest
import torch

import test_geomed_gpu as G
import ddl25spring_amd.ops.reference as R
from test_collude_cpu import spawn_with_timeout
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl import checkpoint as ckpt
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


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("K", G.SCALES_G)
def test_gm_scales_cpu(K):
    G.check_gm_scales(K, CPU)


@pytest.mark.parametrize("K", sorted(set(G.FUSED_G + G.UNFUSED_G)))
def test_aggregator_is_its_ops_cpu(K):
    G.check_aggregator_is_its_ops(K, CPU, True)  # the CPU takes the unfused route


def test_routes_agree_cpu():
    G.check_routes_agree(CPU)


def test_fixed_points_cpu():
    G.check_fixed_points(CPU, True)


@pytest.mark.parametrize("K,f", G.INFLUENCE_KF)
def test_bounded_influence_cpu(K, f):
    G.check_bounded_influence(K, f, CPU, True)


# ------------------------------------------------------------------ FedAvg: checkpoint, two ranks
AGG_KW = {"gm_iters": 3, "gm_nu": 1e-6}
SEED, ROUNDS = 17, 5  # 4 clients, 2 sampled, dropout 0.4: round 2 has one reporter (rank 1 holds none)


def _fed(ctx, **kw):
    arr = synthetic_images("mnist", 400, seed=0)
    parts = split(4, True, 7, labels=arr.labels)
    return FedAvg(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, lr=0.1, batch_size=50, client_fraction=0.5,
                  seed=SEED, ctx=ctx, dropout=0.4, aggregator="geomed", agg_kwargs=AGG_KW, **kw)


def test_checkpoint_resume_is_identical(fp32):
    ref = _fed(DistContext(), attack=ALIE([0, 1]))
    ref.run(4)
    assert ref.state_dict()["aggregator"] == {"rounds": 4, "last_k": ref.aggregator.last_k}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fl.pt")
        ckpt.run_with_checkpoints(_fed(DistContext(), attack=ALIE([0, 1])), 2, path)
        b = _fed(DistContext(), attack=ALIE([0, 1]))  # fresh process-equivalent: rebuild, then resume
        ckpt.run_with_checkpoints(b, 4, path)
        assert b.round_idx == 4 and b.aggregator.rounds == 4
    assert torch.equal(b.w_global, ref.w_global)


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    fa = _fed(ctx)
    for _ in range(ROUNDS):
        fa.round()
    torch.save(fa.w_global, os.path.join(out_dir, f"w{rank}.pt"))
    rdist.shutdown()


def test_distributed_geomed_fedavg_matches_single_process(fp32):
    """2 gloo ranks against one process holding all the clients; the rounds of this seed include
    one with an empty rank, which still takes part in the all-gather of the normaliser."""
    single = _fed(DistContext())
    for _ in range(ROUNDS):
        single.round()
    assert [2 - len(gone) for gone in single.dropped] == [2, 1, 2, 2, 2]
    with tempfile.TemporaryDirectory() as d:
        port = 29950 + (os.getpid() % 100)
        spawn_with_timeout(_dist_worker, (2, port, d))
        w0 = torch.load(os.path.join(d, "w0.pt"), weights_only=True)
        w1 = torch.load(os.path.join(d, "w1.pt"), weights_only=True)
    assert torch.equal(w0, w1)  # replicated server state stays identical on every rank
    assert torch.allclose(w0, single.w_global, atol=1e-5), (w0 - single.w_global).abs().max()


# --------------------------------------------------------------------------------------- CLI
def test_cli_bulyan_and_geomed(tmp_path, capsys):
    from ddl25spring_amd.cli import main
    base = ["--device", "cpu", "fl", "--model", "mnist_mlp", "--client-fraction", "1.0", "--rounds", "2",
            "--train-size", "400", "--test-size", "200", "--batch-size", "50", "--lr", "0.1", "--malicious", "1"]
    assert main(base + ["--clients", "8", "--aggregator", "bulyan", "--krum-f", "1"]) == 0
    assert "Test accuracy" in capsys.readouterr().out
    assert main(base + ["--clients", "4", "--aggregator", "geomed", "--gm-iters", "2", "--gm-nu", "1e-5",
                        "--agg-weighting", "uniform", "--attack", "ipm"]) == 0
    assert main(base + ["--clients", "4", "--aggregator", "rfa"]) == 0
