"""Secure aggregation without a GPU: the oracle's own known answers, the torch twins on the cases of
tests/test_secagg_gpu.py, and the engine: round 1 against the plain mean, the aborted round,
checkpoints with noise on, two gloo ranks, the CLI and the rejected combinations."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import secagg_oracle as O
import test_secagg_gpu as G
import ddl25spring_amd.ops.reference as R
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.aggregate import SecureMean, make_aggregator
from ddl25spring_amd.fl.algorithms import FedAvg, FedSGD, Scaffold
from ddl25spring_amd.models import mnist_mlp
from ddl25spring_amd.models import params as P
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

CPU = torch.device("cpu")


@pytest.fixture
def fp32(monkeypatch):
    monkeypatch.setattr(R, "_bf", lambda t: t.float())
    monkeypatch.setattr(P, "CPU_SHADOW_DTYPE", torch.float32)


# ----------------------------------------------------------------------------- the oracle itself
def test_philox_known_answer():
    """Philox-4x32-10, counter 0, key 0; the package's twin gives the same words."""
    z = np.zeros(1, dtype=np.uint64)
    got = tuple(int(w[0]) for w in O.philox(z, z, z, z, 0, 0))
    assert got == O.KNOWN_ANSWER, [hex(w) for w in got]
    zt = torch.zeros(1, dtype=torch.int64)
    assert tuple(int(w[0]) for w in R.philox4x32_t(zt, zt, zt, zt, 0, 0)) == O.KNOWN_ANSWER
    assert R.SECAGG_TAG == O.TAG and O.TAG not in (R.CLIP_NOISE_TAG, R.QUANT_TAG)
    m = O.pair_mask(9, 2, 7, G.SEED, G.ROUND)
    assert np.array_equal(m, R.secagg_pair_mask(9, 2, 7, G.SEED, G.ROUND).numpy().astype(np.uint64))
    for other in (O.pair_mask(9, 2, 8, G.SEED, G.ROUND), O.pair_mask(9, 2, 7, G.SEED + 1, G.ROUND),
                  O.pair_mask(9, 2, 7, G.SEED, G.ROUND + 1), O.pair_mask(9, 7, 7, G.SEED, G.ROUND)):
        assert not np.array_equal(other, m)
    assert np.array_equal(O.pair_mask(5, 2, 7, G.SEED, G.ROUND), m[:5])


def test_oracle_on_hand_computed_cases():
    # f = 8, n = 2: lim = 1073741823. cs = 0.5, x - c = (1, 0.00390625 * 3, -5e9, nan): p * 256 =
    # (128, 1.5, -6.4e11, nan) -> q = (128, 2 (tie to even), -lim, 0), two counted
    rows = np.array([[2.0, 1.01171875, -5e9, np.nan]], dtype=np.float32)
    c = np.array([1.0, 1.0, 0.0, 0.0], dtype=np.float32)
    q, sat = O.encode(rows, c, np.array([0.5], dtype=np.float32), 2, 8)
    assert q.tolist() == [[128, 2, -1073741823, 0]] and sat.tolist() == [2]
    q, sat = O.encode(rows, c, np.array([0.0], dtype=np.float32), 2, 8)
    assert not q.any() and sat.tolist() == [0]
    # 2.5 and 3.5 both round to even neighbours
    q, _ = O.encode(np.array([[2.5 / 256, 3.5 / 256]], dtype=np.float32), None, np.array([1.0], dtype=np.float32), 1, 8)
    assert q.tolist() == [[2, 4]]
    # two clients, everything cancels but the self masks; with client 1 dropped its pair mask is put back
    rows = np.array([[0.25, -0.5], [1.0, 2.0]], dtype=np.float32)
    cs = np.array([1.0, 1.0], dtype=np.float32)
    w, _, q = O.mask(rows, None, cs, [0, 1], [0, 1], 8, 1, 0)
    assert O.open_(w, [0, 1], [], 8, 1, 0).tolist() == [1.25, 1.5]
    assert O.open_(w[:1], [0], [1], 8, 1, 0).tolist() == [0.25, -0.5]
    assert O.open_(w[:1], [0], [], 8, 1, 0).tolist() != [0.25, -0.5]
    assert O.to_i32(np.array([2 ** 32 + 5, -1, 2 ** 31])).tolist() == [5, -1, -2 ** 31]


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("P_", G.SIZES_P)
@pytest.mark.parametrize("K", G.SIZES_G)
def test_words_sat_and_delta_equal_the_oracle_cpu(K, P_):
    G.check_bit_equality(K, P_, CPU)


@pytest.mark.parametrize("P_", G.SIZES_P)
@pytest.mark.parametrize("K", G.SIZES_G)
def test_zero_weight_row_uploads_bare_masks_cpu(K, P_):
    G.check_zero_weight_row(K, P_, CPU)


@pytest.mark.parametrize("P_", G.SIZES_P)
def test_placement_does_not_change_a_bit_cpu(P_):
    G.check_placement(P_, CPU)


@pytest.mark.parametrize("P_", G.SIZES_P)
def test_range_saturates_and_counts_cpu(P_):
    G.check_range(P_, CPU)


@pytest.mark.parametrize("P_", G.SIZES_P)
@pytest.mark.parametrize("K", G.SIZES_G)
def test_accuracy_against_float64_cpu(K, P_):
    G.check_accuracy(K, P_, CPU)


def test_second_grid_stride_iteration_cpu():
    G.check_second_pass(CPU)


def test_two_calls_are_bit_equal_cpu():
    G.check_deterministic(CPU)


def test_op_rejects_bad_arguments_cpu():
    G.check_rejects(CPU)
    rows, cs = torch.zeros(2, 8), torch.ones(2)
    words, sat, delta = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(8)
    t = lambda l: torch.tensor(l, dtype=torch.int32)  # noqa: E731
    for slots, cohort in (([0, 65536], [0, 65536]), ([1, 1], [1, 2]), ([0, 3], [0, 1, 2])):  # a host table is checked
        with pytest.raises(ValueError):
            Fn.secagg_mask(rows, None, cs, t(slots), t(cohort), 20, 0, 0, words, sat)
    with pytest.raises(ValueError):
        Fn.secagg_open(words, t([0, 1]), t([1]), 20, 0, 0, delta)


# ------------------------------------------------------------------------------------- the engine
def test_round_one_tracks_the_plain_mean_cpu():
    G.check_round_one_against_mean(CPU)
    G.check_round_one_against_mean(CPU, f=12)


def test_lone_survivor_aborts_the_round_cpu():
    G.check_abort(CPU)


def test_fedsgd_round_and_every_client_dropped(fp32):
    """FedSGD's gradients are the updates (no centre); a round without any survivor is counted as
    aborted and leaves the model alone."""
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(4, True, 1, labels=arr.labels)
    kw = dict(lr=0.1, client_fraction=1.0, seed=3, eval_every=0)
    sec = FedSGD(mnist_mlp, data, parts, aggregator="secagg", **kw)
    mean = FedSGD(mnist_mlp, data, parts, **kw)
    sec.round()
    mean.round()
    # the mean gradients differ by at most K 2^-(f+1) plus fp32 roundings; the step scales that by lr
    err = float((sec.w_global.double() - mean.w_global.double()).abs().max())
    assert err <= 0.1 * 4 * 2.0 ** -21 + 1e-6, err
    assert sec.aggregator.rounds == 1 and sec.aggregator.last_saturated == [0] * 4
    gone = FedAvg(mnist_mlp, data, parts, aggregator="secagg", dropout=1.0, batch_size=50, **kw)
    before = gone.w_global.clone()
    gone.round()
    gone.round()
    assert gone.aggregator.aborted == [0, 1] and gone.aggregator.rounds == 2 and torch.equal(gone.w_global, before)


def test_aggregator_interface():
    agg = make_aggregator("secagg", frac_bits=12, min_survivors=3, clip=2.0)
    assert type(agg) is SecureMean and (agg.frac_bits, agg.min_survivors, agg.clip) == (12, 3, 2.0)
    assert agg.takes_center and agg.name == "secagg" and make_aggregator("secagg").clip == float("inf")
    ctx = DistContext()
    rows, out = torch.full((2, 4), 0.5), torch.zeros(4)
    with pytest.raises(RuntimeError):  # no begin_round
        agg(ctx, rows, torch.ones(2), out)
    with pytest.raises(ValueError):
        agg.begin_round([0, 1], [0, 2], [0])  # a survivor outside the cohort
    agg.begin_round([0, 1, 2], [0, 1], [0, 1])
    with pytest.raises(ValueError):  # two rows, three announced... the other way round
        agg(ctx, rows[:1], torch.ones(1), out)
    # fewer than min_survivors = 3: aborted, out = centre
    centre = torch.arange(4.0)
    agg(ctx, rows, torch.full((2,), 0.5), out, center=centre, counts=[2])
    assert agg.aborted == [0] and torch.equal(out, centre) and agg.rounds == 1
    with pytest.raises(RuntimeError):  # every round is announced anew
        agg(ctx, rows, torch.ones(2), out)
    agg = SecureMean(frac_bits=8)
    agg.begin_round([5, 9, 7], [5, 9], [5, 9])
    agg(ctx, rows, torch.full((2,), 0.5), out, center=None, counts=[2])
    assert out.tolist() == [0.5] * 4 and agg.last_saturated == [0, 0] and agg.last_k == 2
    sd = agg.state_dict()
    assert sd == {"rounds": 1, "last_k": 2, "aborted": []}
    other = SecureMean()
    other.load_state_dict({"rounds": 4, "last_k": 3, "aborted": [1, 2]})
    assert (other.rounds, other.last_k, other.aborted) == (4, 3, [1, 2])


def test_rejected_combinations():
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(2, True, 1, labels=arr.labels)
    with pytest.raises(ValueError):
        Scaffold(mnist_mlp, data, parts, lr=0.1, aggregator="secagg")
    with pytest.raises(ValueError):
        FedAvg(mnist_mlp, data, parts, lr=0.1, aggregator="secagg", agg_kwargs=dict(frac_bits=31))


# ----------------------------------------------------------------------------------- checkpoints
def test_checkpoint_resume_is_identical(fp32):
    """Round 1, save, round 2 in a fresh server, noise on: w_global and the aggregator's state equal
    two uninterrupted rounds."""
    from ddl25spring_amd.fl import checkpoint as ckpt
    arr = synthetic_images("mnist", 400, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(6, True, 10, labels=arr.labels)
    kw = dict(lr=0.05, batch_size=50, client_fraction=0.5, seed=4, dropout=0.3, aggregator="secagg",
              agg_kwargs=dict(frac_bits=16, clip=1.0, noise_multiplier=0.5, weighting="uniform", seed=9,
                              min_survivors=1))
    ref = FedAvg(mnist_mlp, data, parts, **kw)
    ref.run(3)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fl.pt")
        ckpt.run_with_checkpoints(FedAvg(mnist_mlp, data, parts, **kw), 1, path)
        b = FedAvg(mnist_mlp, data, parts, **kw)  # fresh process-equivalent: rebuild, then resume
        ckpt.run_with_checkpoints(b, 3, path)
    assert b.round_idx == 3 and b.aggregator.rounds == ref.aggregator.rounds == 3
    assert torch.equal(b.w_global, ref.w_global) and b.aggregator.state_dict() == ref.aggregator.state_dict()
    quiet = FedAvg(mnist_mlp, data, parts, **{**kw, "agg_kwargs": dict(kw["agg_kwargs"], noise_multiplier=0.0)})
    quiet.run(3)
    assert not torch.equal(quiet.w_global, ref.w_global)  # the noise was on


# --------------------------------------------------------------------------- distributed (gloo)
def _dist_fed(ctx, fraction):
    """4 clients of unequal size (as test_compress_cpu._dist_fed): the single process trains its
    slots one by one, as each rank trains its own."""
    arr = synthetic_images("mnist", 400, seed=0)
    perm = np.random.default_rng(7).permutation(400)
    parts = [perm[a:b] for a, b in ((0, 80), (80, 170), (170, 270), (270, 380))]
    return FedAvg(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, ctx=ctx, lr=0.1, batch_size=50,
                  client_fraction=fraction, seed=7, aggregator="secagg", dropout=0.3,
                  agg_kwargs=dict(frac_bits=20, clip=0.5))


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    torch.set_num_threads(1)  # as the single-process run: the CPU GEMMs' bits depend on the thread count
    out = {}
    for name, fraction in (("two", 0.5), ("four", 1.0)):
        fa = _dist_fed(ctx, fraction)
        for _ in range(3):
            fa.round()
        out[name] = {"w": fa.w_global, "aborted": torch.tensor(fa.aggregator.aborted, dtype=torch.int64)}
    torch.save(out, os.path.join(out_dir, f"s{rank}.pt"))
    rdist.shutdown()


def test_distributed_secagg_matches_single_process(fp32):
    """2 gloo ranks against one process, 3 rounds with dropout, 2 and 4 clients per round: the model
    is bit-equal for both. The integer sum does not care how it is regrouped (the float clipped mean
    only manages allclose at 4)."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        single = {}
        for name, fraction in (("two", 0.5), ("four", 1.0)):
            single[name] = _dist_fed(DistContext(), fraction)
            for _ in range(3):
                single[name].round()
    finally:
        torch.set_num_threads(nthreads)
    with tempfile.TemporaryDirectory() as d:
        port = 29420 + (os.getpid() % 150)
        mp.spawn(_dist_worker, args=(2, port, d), nprocs=2, join=True)
        s0 = torch.load(os.path.join(d, "s0.pt"), weights_only=True)
        s1 = torch.load(os.path.join(d, "s1.pt"), weights_only=True)
    for name, fa in single.items():
        assert torch.equal(s0[name]["w"], s1[name]["w"]), name
        assert torch.equal(s0[name]["w"], fa.w_global), (name, (s0[name]["w"] - fa.w_global).abs().max())
        assert s0[name]["aborted"].tolist() == fa.aggregator.aborted, name
        assert any(fa.dropped), name  # the recovery path ran


# --------------------------------------------------------------------------------------- the CLI
def test_cli_secagg(tmp_path, capsys):
    from ddl25spring_amd.cli import main
    base = ["--device", "cpu", "fl", "--model", "mnist_mlp", "--clients", "4", "--client-fraction", "1.0",
            "--rounds", "3", "--train-size", "200", "--test-size", "100", "--batch-size", "50", "--lr", "0.1"]
    log = tmp_path / "sec.jsonl"
    assert main(base + ["--aggregator", "secagg", "--secagg-bits", "16", "--secagg-min-survivors", "3",
                        "--dropout", "0.3", "--jsonl", str(log)]) == 0
    assert "Test accuracy" in capsys.readouterr().out
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert [r["round"] for r in recs] == [1, 2, 3]
    for r in recs:
        assert r["secagg_cohort"] == 4 and 0 <= r["secagg_survivors"] <= 4
        assert r["secagg_aborted"] == (r["secagg_survivors"] < 3)
    dense = tmp_path / "dense.jsonl"
    assert main(base + ["--jsonl", str(dense)]) == 0
    assert all("secagg_cohort" not in json.loads(ln) for ln in dense.read_text().splitlines())
    with pytest.raises(ValueError):
        main(base + ["--aggregator", "secagg", "--algorithm", "scaffold"])


def test_build_server_passes_the_settings_on():
    from ddl25spring_amd.apps.fl import FLConfig, build_server
    from ddl25spring_amd.fl.aggregate import ClippedMean
    base = dict(model="mnist_mlp", clients=4, train_size=200, test_size=100, batch_size=40, seed=6)
    srv = build_server(FLConfig(aggregator="secagg", secagg_bits=12, secagg_min_survivors=3, **base), DistContext())
    agg = srv.aggregator
    assert type(agg) is SecureMean and (agg.frac_bits, agg.min_survivors, agg.clip, agg.seed) == (12, 3, float("inf"), 6)
    srv = build_server(FLConfig(aggregator="secagg", clip_norm=0.5, noise_multiplier=1.0, agg_weighting="uniform",
                                **base), DistContext())
    assert (srv.aggregator.clip, srv.aggregator.noise_multiplier, srv.aggregator.weighting) == (0.5, 1.0, "uniform")
    srv = build_server(FLConfig(aggregator="clipped", **base), DistContext())  # the clipped mean's default stays
    assert type(srv.aggregator) is ClippedMean and srv.aggregator.clip == 1.0
