"""The robust aggregation rules against the float64 oracle (tests/robust_oracle.py) without a GPU:
the CPU twins in ``ops.functional``, the aggregator classes through a single-process
``DistContext``, and the aggregator cases of tests/test_robust_agg_gpu.py over both devices (the
device half is marked ``gpu`` and skips without one)."""
import pytest
import torch

import robust_oracle as O
import test_robust_agg_gpu as G

CPU = torch.device("cpu")
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.fixture
def dev(request):
    if request.param == "cuda":
        return request.getfixturevalue("cuda")  # skips without a GPU
    return CPU


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_on_hand_computed_cases():
    nan, inf = float("nan"), float("inf")
    X = torch.tensor([[1.0, nan], [3.0, 2.0], [2.0, -inf], [10.0, 4.0]])
    assert O.select(X, "median").tolist() == [2.5, 3.0]        # sorted: 1 2 3 10 / -inf 2 4 +inf
    assert O.select(X, "trimmed", 1).tolist() == [2.5, 3.0]
    assert O.select(X[:3], "median").tolist()[0] == 2.0
    Y = torch.tensor([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0], [nan, 0.0]])
    sc, sel = O.krum(Y, 1, 4)
    assert sc.tolist() == [1.0, 18.0, 1.0, inf] and sel == [0, 2, 1, 3]
    assert O.krum(Y, 1, 2, keys=[3, 2, 1, 0])[1] == [2, 0]     # the tie goes to the smaller key
    assert O.krum(Y, 2, 9)[0].tolist() == [26.0, 43.0, 19.0, inf]
    assert len(O.krum(Y, 2, 9)[1]) == 4                        # m clamped to K
    assert O.gram(Y[:3], torch.tensor([0.0, 1.0])).tolist() == [[1.0, -3.0, 0.0], [-3.0, 18.0, 0.0], [0.0, 0.0, 0.0]]


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("K", G.SWEEP_K)
def test_coord_select_sweep_cpu(K):
    G.check_coord_select_sweep(K, CPU)


@pytest.mark.parametrize("kind", O.BAD_KINDS)
@pytest.mark.parametrize("K", G.ATTACK_K)
def test_coord_select_under_attack_cpu(K, kind):
    G.check_coord_select_attack(K, kind, CPU)


@pytest.mark.parametrize("K", G.ATTACK_K)
def test_coord_select_beyond_breakdown_cpu(K):
    G.check_coord_select_beyond_breakdown(K, CPU)


@pytest.mark.parametrize("K", G.KRUM_K)
def test_krum_select_exact_gram_cpu(K):
    G.check_krum_select_exact(K, CPU)


@pytest.mark.parametrize("kind", O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K,f", G.KRUM_ATTACK)
def test_krum_under_attack_cpu(K, f, kind):
    G.check_krum_attack(K, f, kind, CPU)


# ------------------------------------------------------- aggregator classes, over both devices
@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("name", ["median", "trimmed_mean"])
@pytest.mark.parametrize("K", G.ATTACK_K)
def test_select_aggregators_under_attack(dev, name, K):
    for kind in O.BAD_KINDS:
        G.check_aggregator_attack(name, K, None, kind, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
@pytest.mark.parametrize("name", ["krum", "multikrum"])
@pytest.mark.parametrize("K,f", G.KRUM_ATTACK)
def test_krum_aggregators_under_attack(dev, name, K, f):
    """Bad rows at index 0 included: a NaN / Inf / overflowing row there used to win Krum."""
    for kind in O.KRUM_BAD_KINDS:
        G.check_aggregator_attack(name, K, f, kind, dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_multikrum_fewer_clients_than_m(dev):
    G.check_krum_fewer_clients_than_m(dev)


@pytest.mark.parametrize("dev", DEVICES, indirect=True)
def test_krum_fallback_above_128(dev):
    G.check_krum_fallback(dev)
