"""``fl.attacks.Backdoor``: the data poisoning, the triggered test set and the boosted update."""
import numpy as np
import pytest
import torch

from ddl25spring_amd.data.images import ImageArrays, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.attacks import Backdoor, make_attack

BAD = [0, 2]
N, CLIENTS, TARGET, PATCH = 600, 5, 3, 4


def _data():
    arr = synthetic_images("cifar10", N, seed=1)  # three channels: the trigger goes on every one
    return arr, split(CLIENTS, True, 5, labels=arr.labels)


def _stamped(images, patch=PATCH, value=255):
    return bool((images[:, -patch:, -patch:, :] == value).all())


def test_poison_properties():
    arr, parts = _data()
    before = (arr.images.copy(), arr.labels.copy(), [p.copy() for p in parts])
    atk = make_attack("backdoor", BAD, target=TARGET, poison_fraction=0.5, patch=PATCH, seed=9)
    assert isinstance(atk, Backdoor) and atk.state_dict() == {} and not getattr(atk, "collective", False)
    out, idx = atk.poison(arr, parts)
    # the arguments are not modified, the original rows stay in front, the counts n_k stay
    assert np.array_equal(arr.images, before[0]) and np.array_equal(arr.labels, before[1])
    assert all(np.array_equal(a, b) for a, b in zip(parts, before[2]))
    assert isinstance(out, ImageArrays) and out.kind == arr.kind and out.images.dtype == np.uint8
    assert np.array_equal(out.images[:N], arr.images) and np.array_equal(out.labels[:N], arr.labels)
    assert [len(a) for a in idx] == [len(p) for p in parts]
    total = 0
    for m in range(CLIENTS):
        if m not in BAD:
            assert np.array_equal(idx[m], parts[m])
            continue
        changed = idx[m] != parts[m]
        new, old = idx[m][changed], parts[m][changed]
        non_target = int((arr.labels[parts[m]] != TARGET).sum())
        assert len(new) == min(round(0.5 * len(parts[m])), non_target) > 0
        assert (arr.labels[old] != TARGET).all()           # only samples of other classes are replaced
        assert (new >= N).all() and len(set(new.tolist())) == len(new)
        assert (out.labels[new] == TARGET).all() and _stamped(out.images[new])
        # a copy is its source outside the patch
        a, b = out.images[new].copy(), arr.images[old].copy()
        a[:, -PATCH:, -PATCH:, :] = b[:, -PATCH:, -PATCH:, :] = 0
        assert np.array_equal(a, b)
        total += len(new)
    assert len(out) == N + total
    used = np.concatenate([idx[m][idx[m] >= N] for m in BAD])
    assert sorted(used.tolist()) == list(range(N, N + total))  # every copy belongs to exactly one client
    # a pure function of the arguments; another seed picks other samples
    again, idx2 = atk.poison(arr, parts)
    assert np.array_equal(again.images, out.images) and np.array_equal(again.labels, out.labels)
    assert all(np.array_equal(a, b) for a, b in zip(idx, idx2))
    _, idx3 = Backdoor(BAD, target=TARGET, patch=PATCH, seed=10).poison(arr, parts)
    assert any(not np.array_equal(a, b) for a, b in zip(idx, idx3))


def test_poison_takes_fewer_when_the_client_has_fewer():
    arr, _ = _data()
    labels = arr.labels.copy()
    mine = np.arange(100)
    labels[mine[7:]] = TARGET  # 7 samples of other classes among the client's 100
    labels[mine[:7]] = (TARGET + 1) % 10
    arr = ImageArrays(arr.images, labels, arr.kind, True)
    out, idx = Backdoor([0], target=TARGET, poison_fraction=0.5).poison(arr, [mine, np.arange(100, N)])
    assert len(out) == N + 7 and sorted(idx[0][:7].tolist()) == list(range(N, N + 7))
    assert np.array_equal(idx[0][7:], mine[7:])
    out, idx = Backdoor([0], target=TARGET, poison_fraction=0.0).poison(arr, [mine, np.arange(100, N)])
    assert len(out) == N and np.array_equal(idx[0], mine)


def test_stamp_and_triggered_test():
    arr, _ = _data()
    atk = Backdoor(BAD, target=TARGET, patch=PATCH, value=200)
    st = atk.stamp(arr.images[:10])
    assert _stamped(st, value=200) and not np.shares_memory(st, arr.images)
    keep = np.ones(arr.images.shape[1:3], dtype=bool)
    keep[-PATCH:, -PATCH:] = False
    assert np.array_equal(st[:, keep], arr.images[:10][:, keep])
    trig = atk.triggered_test(arr)
    src = arr.labels != TARGET
    assert len(trig) == int(src.sum()) < N and (trig.labels == TARGET).all()
    assert _stamped(trig.images, value=200) and np.array_equal(trig.images[:, keep], arr.images[src][:, keep])
    for bad in (dict(patch=0), dict(poison_fraction=1.5), dict(value=256), dict(target=-1)):
        with pytest.raises(ValueError):
            Backdoor(BAD, **bad)


def test_boost_is_model_replacement():
    K, n, boost = 6, 1027, 3.5  # exact in fp32: the factor itself adds no rounding
    g = torch.Generator().manual_seed(4)
    c = torch.randn(n, generator=g)
    X = c + 0.1 * torch.randn(K, n, generator=g)
    clients = [5, 0, 7, 2, 9, 11]  # slot order: rows 1 and 3 belong to the attackers
    rows = X.clone()
    Backdoor(BAD, boost=boost).poison_updates(rows, c, clients)
    assert torch.equal(rows[[0, 2, 4, 5]], X[[0, 2, 4, 5]])
    for r in (1, 3):
        # three fp32 operations, each within half an ulp of its exact result, followed through in float64
        d = X[r].double() - c.double()
        want = c.double() + boost * d
        u = 2.0 ** -24
        bound = u * (boost * d.abs() * (1 + u) + boost * d.abs() * (1 + u) ** 2 + want.abs()) * (1 + 4 * u)
        assert bool(((rows[r].double() - want).abs() <= bound).all())
        assert not torch.equal(rows[r], X[r])
    # gradients without a centre: the row is the update
    rows = X.clone()
    Backdoor(BAD, boost=boost).poison_updates(rows, None, clients)
    assert torch.equal(rows[1], X[1] * torch.tensor(boost)) and torch.equal(rows[0], X[0])
    # boost 1 leaves every row bit-equal
    rows = X.clone()
    Backdoor(BAD).poison_updates(rows, c, clients)
    assert torch.equal(rows, X)
