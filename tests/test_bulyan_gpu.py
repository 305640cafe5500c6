"""Bulyan (csrc/kernels/aggregate.hip: ``ddl_bulyan_select``, ``ddl_bulyan_coord``; ``fl.aggregate.Bulyan``)
against the float64 oracle of tests/bulyan_oracle.py.

The ``check_*`` functions take the device, so tests/test_bulyan_cpu.py runs the same cases on the
torch twins; here they run on the kernels."""
import pytest
import torch

import bulyan_oracle as B
import robust_oracle as O
from test_robust_agg_gpu import exact_rows
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

WINDOW_KF = ((7, 1), (11, 2), (16, 3), (33, 7), (65, 15), (128, 31))
COORD_KF = ((3, 0), (7, 1), (8, 1), (9, 1), (11, 2), (16, 1), (16, 3), (17, 3), (33, 7), (64, 15), (65, 15),
            (127, 31), (128, 1), (128, 31))
SELECT_K = (3, 7, 8, 9, 16, 17, 64, 65, 128)
ATTACK_KF = ((7, 1), (11, 2), (33, 7), (128, 31))
BIG_N = 256 * 2048 + 259  # a second wave of blocks on every CU, and a partial last block


# ------------------------------------------------------------------------------- 2: bulyan_coord
def pick_rows(K, f, g):
    """A permuted (not ascending) theta-subset of the K rows; with f > 0 it leaves out rows 0 and K-1."""
    theta = K - 2 * f
    pool = torch.arange(K) if f == 0 else torch.arange(1, K - 1)
    sel = pool[torch.randperm(pool.numel(), generator=g)[:theta]]
    if sel.tolist() == sorted(sel.tolist()):
        sel = sel.flip(0)
    assert sel.numel() == theta and sel.tolist() != sorted(sel.tolist())
    return sel.to(torch.int32)


def assert_coord(X, sel, beta, dev, tag, exact):
    got = Fn.bulyan_coord(O.strided(X, dev), sel.to(dev), beta).cpu()
    want, bound = B.coord(X, sel, beta)
    err = (got.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"bulyan_coord {tag}: worst err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{tag}: err / bound = {worst}"
    if exact:  # every partial sum is an integer below 2^24: only the division rounds
        assert torch.equal(got, want.float()), tag


def check_coord_sweep(K, f, dev):
    g = torch.Generator().manual_seed(100 * K + f)
    theta, n = K - 2 * f, 515
    sel = pick_rows(K, f, g)
    out = [r for r in range(K) if r not in set(sel.tolist())]
    for name in ("randn", "ties"):
        X = torch.randn(K, n, generator=g) if name == "randn" else torch.randint(-2, 3, (K, n), generator=g).float()
        X[out] = 1e6  # a row that was not selected must not be read
        assert_coord(X, sel, theta - 2 * f, dev, f"{name} K={K} f={f}", name == "ties")


def check_coord_big(dev):
    K, f = 9, 1
    g = torch.Generator().manual_seed(5)
    X = torch.randn(K, BIG_N, generator=g)
    X[:, BIG_N - 5:] *= 30.0  # a dropped tail element cannot hide in the tolerance
    assert_coord(X, pick_rows(K, f, g), K - 4 * f, dev, "big", False)


@pytest.mark.parametrize("K,f", COORD_KF)
def test_bulyan_coord_sweep(cuda, K, f):
    check_coord_sweep(K, f, cuda)


def test_bulyan_coord_second_wave_and_tail(cuda):
    check_coord_big(cuda)


# ------------------------------------------------------------------------------ 3: bulyan_select
def select_fs(K):
    return sorted({f for f in (0, 1, (K - 3) // 4) if K >= 4 * f + 3})


def check_select_exact(K, dev):
    X = exact_rows(K)
    gram = O.gram(X).float()
    assert torch.equal(gram.double(), O.gram(X))  # exact in fp32
    for f in select_fs(K):
        for keys in (None, list(range(K - 1, -1, -1))):
            tag = f"K={K} f={f} keys={'rev' if keys else None}"
            want_sc, want_sel, ties = B.select(X, f, keys)
            assert len(want_sel) == K - 2 * f and ties >= 1, f"{tag}: no tie for the keys to break"
            sc, sel = Fn.bulyan_select(gram.to(dev), f, keys)
            assert sel.dtype == torch.int32 and sel.cpu().tolist() == want_sel, tag
            assert torch.equal(sc.cpu().double(), torch.tensor(want_sc, dtype=torch.float64)), tag
            if K - f - 2 >= 1:
                _, first = Fn.krum_select(gram.to(dev), K - f - 2, 1, keys)
                assert first.cpu().tolist() == want_sel[:1], tag


@pytest.mark.parametrize("K", SELECT_K)
def test_bulyan_select_exact_gram(cuda, K):
    check_select_exact(K, cuda)


# ------------------------------------------------------------------------------- 4: under attack
def check_attack(K, f, kind, dev):
    """gram -> bulyan_select -> bulyan_coord, and the ``Bulyan`` class, with f hostile rows. For the
    finite kinds only the range is asserted: a float64 selection admits up to f identical colluders
    late in the loop, the fp32 Gram overflows them to infinitely far; neither is wrong."""
    P = 300
    ctx = DistContext()
    for where in O.PLACEMENTS:
        X, honest, bad = O.attack_rows(K, f, P, kind, where)
        tag = f"K={K} f={f} {kind} {where}"
        rows = O.strided(X, dev)
        _, sel = Fn.bulyan_select(Fn.gram(rows).contiguous(), f)
        out = Fn.bulyan_coord(rows, sel, K - 4 * f).cpu()
        agg = A.make_aggregator("bulyan", f=f)
        assert agg.name == "bulyan" and agg.needs_all and not getattr(agg, "takes_center", False)
        got = agg(ctx, rows, [K], P).cpu()
        assert torch.equal(got, out) and agg.last_selected == sel.cpu().tolist() and agg.last_f == f, tag
        assert len(set(agg.last_selected)) == K - 2 * f, tag
        lo, hi = X[honest].min(0).values, X[honest].max(0).values
        assert bool(torch.isfinite(out).all()) and bool(((out >= lo) & (out <= hi)).all()), f"{tag}: left the honest range"
        if kind in ("nan", "+inf", "-inf", "one_nan"):
            assert set(agg.last_selected) <= set(honest), f"{tag}: selected {sorted(set(agg.last_selected) & set(bad))}"


@pytest.mark.parametrize("kind", O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K,f", ATTACK_KF)
def test_bulyan_under_attack(cuda, K, f, kind):
    check_attack(K, f, kind, cuda)


# ---------------------------------------------------------------------------- 5: clamp and errors
def check_clamp_and_errors(dev):
    ctx = DistContext()
    g = torch.Generator().manual_seed(9)
    X = torch.randn(9, 40, generator=g)
    agg = A.Bulyan(f=3)
    out = agg(ctx, O.strided(X, dev), [9], 40).cpu()
    assert agg.last_f == 1 and len(agg.last_selected) == 7
    want, bound = B.coord(X, agg.last_selected, 5)
    assert bool(((out.double() - want).abs() <= bound).all())
    X = torch.randn(2, 40, generator=g)
    out = agg(ctx, O.strided(X, dev), [2], 40).cpu()
    assert agg.last_f == 0 and sorted(agg.last_selected) == [0, 1]
    assert O.rel_err(out, X.double().mean(0)) <= 1e-6
    for K, f in ((6, 1), (129, 1)):
        with pytest.raises(ValueError):
            Fn.bulyan_select(torch.eye(K, device=dev), f)
    with pytest.raises(ValueError):
        Fn.bulyan_coord(O.strided(X, dev), torch.tensor([0, 1], dtype=torch.int32, device=dev), 1)  # theta - beta odd
    with pytest.raises(ValueError):
        A.Bulyan(f=-1)


def test_bulyan_clamp_and_errors(cuda):
    check_clamp_and_errors(cuda)
