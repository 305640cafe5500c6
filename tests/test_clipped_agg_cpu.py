"""Clipped FedAvg aggregation without a GPU: the torch twins against the float64 oracle
(tests/clip_oracle.py) on the cases of tests/test_clipped_agg_gpu.py, ``ClippedMean`` through a
single-process ``DistContext`` over both devices (the device half is marked ``gpu``), over two gloo
ranks, and end to end through FedAvg / FedSGD."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clip_oracle as C
import robust_oracle as O
import test_clipped_agg_gpu as G
import ddl25spring_amd.ops.reference as R
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.fl.algorithms import FedAvg, FedSGD
from ddl25spring_amd.fl.attacks import GaussianNoise
from ddl25spring_amd.models import mnist_mlp
from ddl25spring_amd.models import params as P
from ddl25spring_amd.runtime.dist import DistContext

CPU = torch.device("cpu")
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.fixture
def dev(request):
    if request.param == "cuda":
        return request.getfixturevalue("cuda")  # skips without a GPU
    return CPU


@pytest.fixture
def fp32(monkeypatch):
    monkeypatch.setattr(R, "_bf", lambda t: t.float())
    monkeypatch.setattr(P, "CPU_SHADOW_DTYPE", torch.float32)


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_on_hand_computed_cases():
    X = torch.tensor([[4.0, 4.0], [1.0, 2.0], [float("nan"), 0.0], [1.0, 1.0]])
    c = torch.tensor([1.0, 0.0])
    assert C.sqnorm(X, c)[[0, 1, 3]].tolist() == [25.0, 4.0, 1.0]
    s, cs = C.scales(C.sqnorm(X, c), torch.full((4,), 0.25), 2.5)
    assert s.tolist() == [0.5, 1.0, 0.0, 1.0] and cs.tolist() == [0.125, 0.25, 0.0, 0.25]
    delta, mass, _ = C.clipped_sum(X, c, torch.full((4,), 0.25), 2.5)
    assert delta.tolist() == [0.375, 1.25] and mass.tolist() == [0.375, 1.25]
    # Philox-4x32-10 known answers (Random123 kat_vectors: zero and all-ones counter / key)
    assert [int(v[0]) for v in C.philox4x32([0], [0], [0], [0], 0, 0)] == \
        [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert [int(v[0]) for v in C.philox4x32([f], [f], [f], [f], f, f)] == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    z = C.normals(8, 1, 0)
    assert np.array_equal(C.normals(5, 1, 0, offset=2), z[2:7])


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("K", G.NORM_G)
def test_update_norms_cpu(K):
    G.check_norms(K, CPU)


def test_update_norms_second_grid_stride_iteration_cpu():
    G.check_norms_second_pass(CPU)


@pytest.mark.parametrize("K", G.NORM_G)
def test_clipped_sum_cpu(K):
    G.check_clipped_sum(K, CPU)


def test_exact_boundary_cpu():
    G.check_exact_boundary(CPU)


@pytest.mark.parametrize("kind", O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K", G.HOSTILE_K)
def test_hostile_rows_cpu(K, kind):
    G.check_hostile(K, kind, CPU)


def test_two_calls_are_bit_equal_cpu():
    G.check_deterministic(CPU)


def test_noise_matches_oracle_and_moments_cpu():
    G.check_noise_matches_oracle(CPU)


def test_noise_is_a_pure_function_of_seed_round_index_cpu():
    G.check_noise_purity(CPU)


def test_zero_std_is_exactly_center_plus_delta_cpu():
    G.check_zero_std(CPU)


# ------------------------------------------------------------- ClippedMean, over both devices
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("weighting", ["samples", "uniform"])
def test_clipped_mean_aggregator(dev, weighting):
    G.check_aggregator(weighting, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_clipped_mean_noise_and_state(dev):
    G.check_aggregator_noise(dev)


# --------------------------------------------------------------------------- distributed (gloo)
AGG_KW = {"clip": 0.2, "noise_multiplier": 0.5, "seed": 3, "weighting": "uniform"}


def _data(n=600, seed=0):
    arr = synthetic_images("mnist", n, seed=seed)
    return arr, DeviceImageDataset(arr, "cpu")


def _fed(clients, ctx):
    arr, data = _data(100 * clients)
    parts = split(clients, True, 7, labels=arr.labels)
    return FedAvg(mnist_mlp, data, parts, lr=0.1, batch_size=50, client_fraction=1.0, seed=7, ctx=ctx,
                  aggregator="clipped", agg_kwargs=AGG_KW)


def _dist_worker(rank, world, port, out_dir, clients):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    fa = _fed(clients, ctx)
    fa.round()
    fa.round()
    torch.save(fa.w_global, os.path.join(out_dir, f"w{rank}.pt"))
    rdist.shutdown()


@pytest.mark.parametrize("clients", [2, 4])
def test_distributed_clipped_fedavg_matches_single_process(fp32, clients):
    """2 gloo ranks against one process holding all the clients, DP noise on. One client per rank:
    the ordered cross-rank sum adds the same terms in the same order, and every rank draws the same
    noise, so the models are bit-equal; two clients per rank regroup the sum."""
    single = _fed(clients, DistContext())
    single.round()
    single.round()
    with tempfile.TemporaryDirectory() as d:
        port = 29850 + (os.getpid() % 100) + clients
        mp.spawn(_dist_worker, args=(2, port, d, clients), nprocs=2, join=True)
        w0 = torch.load(os.path.join(d, "w0.pt"), weights_only=True)
        w1 = torch.load(os.path.join(d, "w1.pt"), weights_only=True)
    assert torch.equal(w0, w1)  # replicated server state stays identical on every rank
    if clients == 2:
        assert torch.equal(w0, single.w_global)
    else:
        assert torch.allclose(w0, single.w_global, atol=1e-5), (w0 - single.w_global).abs().max()


# ----------------------------------------------------------------------------------- end to end
def _attack_setup():
    arr, data = _data(800)
    tarr, tdata = _data(300, seed=1)
    parts = split(8, True, 5, labels=arr.labels)
    kw = dict(lr=0.1, batch_size=50, local_epochs=1, client_fraction=1.0, seed=5, test_data=tdata)
    return data, parts, kw


def test_clipping_defends_against_gaussian_noise_attack(fp32):
    """8 clients, 2 of them reporting w + N(0, 1) noise (update norm in the hundreds against
    honest 0.15 - 0.29): the plain mean is destroyed, the mean of updates clipped to 0.2 learns."""
    data, parts, kw = _attack_setup()
    attack = lambda: GaussianNoise([0, 1], sigma=1.0)
    attacked = FedAvg(mnist_mlp, data, parts, attack=attack(), **kw).run(5).test_accuracy[-1]
    fa = FedAvg(mnist_mlp, data, parts, attack=attack(), aggregator="clipped", agg_kwargs={"clip": 0.2}, **kw)
    defended = fa.run(5).test_accuracy[-1]
    print(f"undefended {attacked:.1f} %, clipped {defended:.1f} %")
    assert defended > attacked + 30, (attacked, defended)
    norms = sorted(fa.aggregator.last_norms)  # in the round's sampling order: sort them
    assert len(norms) == 8 and norms[5] < 1.0 and norms[6] > 10, norms


@pytest.mark.parametrize("algo", [FedAvg, FedSGD])
def test_checkpoint_resume_with_noise_is_identical(fp32, algo):
    from ddl25spring_amd.fl import checkpoint as ckpt
    arr, data = _data(400)
    parts = split(6, True, 10, labels=arr.labels)
    kw = dict(lr=0.05, client_fraction=0.5, seed=4, aggregator="clipped",
              agg_kwargs={"clip": 0.3, "noise_multiplier": 0.4, "seed": 9, "weighting": "uniform"})
    if algo is FedAvg:
        kw["batch_size"] = 50
    ref = algo(mnist_mlp, data, parts, **kw)
    ref.run(4)
    assert ref.state_dict()["aggregator"] == {"rounds": 4, "last_k": 3}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fl.pt")
        ckpt.run_with_checkpoints(algo(mnist_mlp, data, parts, **kw), 2, path)
        b = algo(mnist_mlp, data, parts, **kw)  # fresh process-equivalent: rebuild, then resume
        ckpt.run_with_checkpoints(b, 4, path)
        assert b.round_idx == 4 and b.aggregator.rounds == 4
    assert torch.equal(b.w_global, ref.w_global)
    # a checkpoint written before the aggregator had a state still loads
    sd = ref.state_dict()
    del sd["aggregator"]
    b.load_state_dict(sd)
    assert "aggregator" not in FedAvg(mnist_mlp, data, parts, lr=0.05, seed=4).state_dict()


def test_cli_dp_fedavg_logs_epsilon(tmp_path, capsys):
    """The CLI flags derived from FLConfig reach the aggregator; with noise on every JSONL round
    record carries the epsilon spent so far, and the results table keeps its columns."""
    import json

    from ddl25spring_amd.cli import main
    from ddl25spring_amd.fl import privacy
    log = tmp_path / "dp.jsonl"
    base = ["--device", "cpu", "fl", "--model", "mnist_mlp", "--clients", "4", "--client-fraction", "0.5",
            "--rounds", "2", "--train-size", "400", "--test-size", "200", "--batch-size", "50", "--lr", "0.1",
            "--aggregator", "clipped", "--clip-norm", "0.3", "--jsonl", str(log)]
    assert main(base + ["--noise-multiplier", "1.1", "--agg-weighting", "uniform"]) == 0
    assert "Test accuracy" in capsys.readouterr().out
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert [r["round"] for r in recs] == [1, 2]
    assert [r["epsilon"] for r in recs] == [privacy.epsilon(r, 0.5, 1.1, 1e-5) for r in (1, 2)]
    assert main(base) == 0  # no noise: no epsilon entry
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert recs and all("epsilon" not in r for r in recs[-2:])
    with pytest.raises(ValueError):
        main(base + ["--noise-multiplier", "1.1"])  # sample weighting with noise


def test_fedsgd_clipped_gradient_is_norm_bounded(fp32):
    arr, data = _data(400)
    parts = split(4, True, 1, labels=arr.labels)
    clip = 0.05
    g = FedSGD(mnist_mlp, data, parts, lr=0.05, client_fraction=0.5, seed=3, aggregator="clipped",
               agg_kwargs={"clip": clip})
    w0 = g.w_global.clone()
    g.round()
    assert min(g.aggregator.last_norms) > clip  # every gradient was clipped
    assert 0 < g.g_global.double().norm().item() <= clip * (1 + 2.0 ** -20)
    assert torch.allclose(g.w_global, w0 - 0.05 * g.g_global, rtol=0, atol=1e-7)
