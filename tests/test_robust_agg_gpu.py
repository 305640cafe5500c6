"""The robust-aggregation kernels (csrc/kernels/aggregate.hip) against the float64 oracle of
tests/robust_oracle.py: at the sort-bucket edges, on strided misaligned rows, and on the hostile
inputs (NaN / Inf / overflowing rows) the rules exist to survive.

The ``check_*`` functions take the device, so tests/test_robust_agg_cpu.py runs the same cases on
the CPU twins; here they run on the kernels."""
import pytest
import torch

import robust_oracle as O
from ddl25spring_amd.fl import aggregate as A
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

SWEEP_K = (1, 2, 3, 7, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128)
ATTACK_K = (5, 16, 65, 128)
KRUM_K = (1, 2, 3, 8, 9, 16, 17, 64, 65, 128)
KRUM_ATTACK = ((9, 2), (33, 8), (128, 31))


# ------------------------------------------------------------------ 1 / 2: coordinate selection
def assert_select_matches(X, dev, trims, tag=""):
    """Median bit-equal to the oracle (an fp32 sum of two floats rounded once, and the halving,
    lose nothing against float64 rounded once); trimmed mean within ``O.trimmed_bound``."""
    Xd = O.strided(X, dev)
    got = Fn.coord_select(Xd, "median").cpu()
    want = O.select(X, "median").float()
    assert torch.equal(got, want), f"median {tag}: {(got.double() - want.double()).abs().max().item()}"
    K = X.shape[0]
    for b in trims:
        got = Fn.coord_select(Xd, "trimmed", b).cpu().double()
        err = (got - O.select(X, "trimmed", b)).abs()
        bound = O.trimmed_bound(X, b)
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"trimmed {tag} K={K} trim={b}: worst err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"trimmed {tag} K={K} trim={b}: err / bound = {worst}"


def sweep_trims(K):
    return sorted({b for b in (0, 1, K // 4, (K - 1) // 2) if K - 2 * b >= 1})


def check_coord_select_sweep(K, dev):
    g = torch.Generator().manual_seed(K)
    assert_select_matches(torch.randn(K, 515, generator=g), dev, sweep_trims(K), "randn")
    ties = torch.randint(-2, 3, (K, 515), generator=g).float()
    assert_select_matches(ties, dev, sweep_trims(K), "ties")


def check_coord_select_attack(K, kind, dev, fn=Fn.coord_select, modes=("median", "trimmed")):
    """Within the breakdown point (f = (K-1)//2 bad rows for the median, f = trim = K//4 for the
    trimmed mean) the result equals the oracle's and stays inside the honest rows' range.
    ``fn(rows, mode, trim)`` is the op, or an aggregator class behind the same signature."""
    n = 300
    for mode, f, b in (("median", (K - 1) // 2, 0), ("trimmed", K // 4, K // 4)):
        if mode not in modes:
            continue
        for where in O.PLACEMENTS:
            X, honest, _ = O.attack_rows(K, f, n, kind, where)
            tag = f"{mode} K={K} {kind} {where}"
            got = fn(O.strided(X, dev), mode, b).cpu()
            want = O.select(X, mode, b)
            if mode == "median":
                assert torch.equal(got, want.float()), tag
            else:
                err = (got.double() - want).abs()
                assert bool((err <= O.trimmed_bound(X, b)).all()), tag
            lo, hi = X[honest].min(0).values, X[honest].max(0).values
            assert bool(((got >= lo) & (got <= hi)).all()), f"{tag}: left the honest range"


@pytest.mark.parametrize("K", SWEEP_K)
def test_coord_select_sweep(cuda, K):
    check_coord_select_sweep(K, cuda)


@pytest.mark.parametrize("kind", O.BAD_KINDS)
@pytest.mark.parametrize("K", ATTACK_K)
def test_coord_select_under_attack(cuda, K, kind):
    check_coord_select_attack(K, kind, cuda)


def check_coord_select_beyond_breakdown(K, dev):
    """trim = 0 with one NaN row is past the breakdown point: the NaN counts as +inf, so the result
    is non-finite exactly where the oracle's is (everywhere), not a silently finite mean of K-1."""
    X, _, _ = O.attack_rows(K, 1, 300, "nan", "interleaved")
    got = Fn.coord_select(O.strided(X, dev), "trimmed", 0).cpu()
    want = O.select(X, "trimmed", 0)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    assert not bool(torch.isfinite(want).any())


@pytest.mark.parametrize("K", ATTACK_K)
def test_coord_select_beyond_breakdown(cuda, K):
    check_coord_select_beyond_breakdown(K, cuda)


# ------------------------------------------------------------------------- 3: krum_select, exact
def exact_rows(K):
    """Small-integer rows: Gram, distances and scores are exact in fp32. Rows 0, 1 and K-1 are one
    and the same all-zero row (the one nearest the others' centroid, so the triple holds the least
    score for every nb): only the keys can order them. At K = 3 that leaves three zero rows and
    every score 0: the case checks the key ordering alone, the scoring is covered by the other K."""
    g = torch.Generator().manual_seed(100 + K)
    X = torch.randint(-3, 4, (K, 64), generator=g).float()
    if K >= 3:
        X[0] = 0.0
        X[1] = X[0]
        X[K - 1] = X[0]
    return X


def check_krum_select_exact(K, dev):
    X = exact_rows(K)
    gram = O.gram(X).float()
    assert torch.equal(gram.double(), O.gram(X))  # exact in fp32
    for nb in sorted({1, max(1, K - K // 4 - 2), max(1, K - 1)}):
        for m in sorted({1, 2, K}):
            for keys in (None, list(range(K - 1, -1, -1))):
                tag = f"K={K} nb={nb} m={m} keys={'rev' if keys else None}"
                want_sc, want_sel = O.krum(X, nb, m, keys)
                assert len(want_sel) == min(m, K)
                if K >= 2:  # vacuous unless a selected client ties with another one
                    sc = want_sc.tolist()
                    assert any(sc.count(sc[i]) > 1 for i in want_sel), f"{tag}: no tie to break"
                sc, sel = Fn.krum_select(gram.to(dev), nb, m, keys)
                assert torch.equal(sc.cpu().float(), want_sc.float()), tag
                assert sel.cpu().tolist() == want_sel, tag


@pytest.mark.parametrize("K", KRUM_K)
def test_krum_select_exact_gram(cuda, K):
    check_krum_select_exact(K, cuda)


# ------------------------------------------------------------------ 4: Krum under attack, kernels
def check_krum_attack(K, f, kind, dev):
    """gram -> krum_select -> mean_rows_idx with f hostile rows. The order among honest clients is
    not compared with the oracle (fp32-Gram scores and float64 direct distances may rank
    near-equal honest clients differently); what Krum guarantees is."""
    P = 300
    nb = K - f - 2
    for where in O.PLACEMENTS:
        X, honest, bad = O.attack_rows(K, f, P, kind, where)
        tag = f"K={K} f={f} {kind} {where}"
        rows = O.strided(X, dev)
        gram = Fn.gram(rows)
        sc, sel = Fn.krum_select(gram.contiguous(), nb, 1)
        win = sel.cpu().tolist()
        assert len(win) == 1 and win[0] in honest, f"{tag}: selected {win}"
        assert O.krum(X, nb, 1)[1][0] in honest  # the oracle agrees that an honest client wins
        assert bool(torch.isfinite(sc.cpu()[honest]).all()), f"{tag}: honest scores not finite"
        out = Fn.mean_rows_idx(rows, sel).cpu()
        lo, hi = X[honest].min(0).values, X[honest].max(0).values
        assert bool(torch.isfinite(out).all()) and bool(((out >= lo) & (out <= hi)).all()), tag
        _, sel = Fn.krum_select(gram.contiguous(), nb, K - f)
        assert sorted(sel.cpu().tolist()) == honest, f"{tag}: multi-Krum kept {sorted(set(sel.cpu().tolist()) & set(bad))}"
        assert sorted(O.krum(X, nb, K - f)[1]) == honest


@pytest.mark.parametrize("kind", O.KRUM_BAD_KINDS)
@pytest.mark.parametrize("K,f", KRUM_ATTACK)
def test_krum_under_attack(cuda, K, f, kind):
    check_krum_attack(K, f, kind, cuda)


# --------------------------------------------------------------------------- aggregator classes
# These cases run from tests/test_robust_agg_cpu.py, parametrised over the device (its device half
# is marked gpu), so that each exists once.
def check_aggregator_attack(name, K, f, kind, dev):
    """The attack tables through ``make_aggregator``: the result stays in the honest rows' range
    and Krum's ``last_selected`` is honest, bad rows at index 0 included."""
    ctx = DistContext()
    if name in ("median", "trimmed_mean"):
        def fn(rows, mode, trim):
            agg = A.make_aggregator(name, trim=trim)
            return agg(ctx, rows, [rows.shape[0]], rows.shape[1])
        check_coord_select_attack(K, kind, dev, fn=fn, modes=("median" if name == "median" else "trimmed",))
        return
    P = 300
    for where in O.PLACEMENTS:
        X, honest, _ = O.attack_rows(K, f, P, kind, where)
        agg = A.make_aggregator(name, f=f, m=K - f)
        out = agg(ctx, O.strided(X, dev), [K], P).cpu()
        tag = f"{name} K={K} f={f} {kind} {where}"
        assert set(agg.last_selected) <= set(honest), f"{tag}: selected {agg.last_selected}"
        if name == "multikrum":
            assert sorted(agg.last_selected) == honest, tag
        lo, hi = X[honest].min(0).values, X[honest].max(0).values
        assert bool(torch.isfinite(out).all()) and bool(((out >= lo) & (out <= hi)).all()), tag


def check_krum_fewer_clients_than_m(dev):
    ctx = DistContext()
    for K in (2, 1):
        X = torch.randn(K, 40, generator=torch.Generator().manual_seed(K))
        agg = A.Krum(f=0, m=3)
        out = agg(ctx, O.strided(X, dev), [K], 40).cpu()
        assert sorted(agg.last_selected) == list(range(K))
        assert O.rel_err(out, X.double().mean(0)) <= 1e-6


def check_krum_fallback(dev):
    """K > 128 (no native selection kernel): the mean of the oracle-selected rows, i.e. len(sel)
    weights of 1 / len(sel) -- also when m exceeds K."""
    K, P, f = 130, 256, 20
    X, honest, bad = O.attack_rows(K, f, P, "nan", "interleaved")
    for t, r in enumerate(bad):  # a mixed population of attackers; row 0 stays a NaN row
        if t % 4 == 1:
            X[r] = float("inf")
        elif t % 4 == 2:
            X[r] = 3e38
        elif t % 4 == 3:
            X[r] = 1.0 + 0.05 * torch.randn(P, generator=torch.Generator().manual_seed(r))
            X[r, r] = float("nan")
    ctx = DistContext()
    nb = K - f - 2
    for m in (5, K + 7):
        agg = A.Krum(f=f, m=m)
        out = agg(ctx, O.strided(X, dev), [K], P).cpu().double()
        sel = agg.last_selected
        want_sel = O.krum(X, nb, m)[1]
        assert len(sel) == min(m, K) and sorted(sel) == sorted(want_sel), f"m={m}: {sel} vs {want_sel}"
        want = X[want_sel].double().mean(0)  # not finite where an attacker is among all K selected
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(out), fin), f"m={m}"
        if m == 5:
            assert set(sel) <= set(honest) and bool(fin.all())
            assert O.rel_err(out, want) <= 1e-6, f"m={m}"
    # m > K on honest rows only, so that the 1 / len(sel) weights show in finite numbers: the same
    # requirement as for m = 5, within 1e-6 of the max-abs
    Xh = X[honest + honest[:K - len(honest)]].clone()
    agg = A.Krum(f=f, m=K + 7)
    out = agg(ctx, O.strided(Xh, dev), [K], P).cpu()
    assert sorted(agg.last_selected) == list(range(K))
    err = O.rel_err(out, Xh.double().mean(0))
    print(f"K > 128, m > K, honest rows: rel err {err:.3e}")
    assert err <= 1e-6


# ------------------------------------------------------------------------------------- 5: Gram
def assert_gram(X, c, dev, tag):
    Xd = O.strided(X, dev)
    cd = None if c is None else c.to(dev)
    g = Fn.gram(Xd, cd)
    err = O.rel_err(g, O.gram(X, c))
    print(f"gram {tag}: rel err {err:.3e}")
    assert err <= 1e-5, f"gram {tag}: rel err {err}"
    assert torch.equal(g, g.t()), f"gram {tag}: not symmetric"
    assert torch.equal(g, Fn.gram(Xd, cd)), f"gram {tag}: not repeatable"


@pytest.mark.parametrize("K", [1, 16, 17, 32, 48, 49, 96, 97])
def test_gram_bucket_edges(cuda, K):
    for n in (1, 63, 257):
        g = torch.Generator().manual_seed(K * 1000 + n)
        X = torch.randn(K, n, generator=g)
        c = torch.randn(n, generator=g)
        assert_gram(X, None, cuda, f"K={K} n={n}")
        assert_gram(X, c, cuda, f"K={K} n={n} centred")


@pytest.mark.parametrize("K,n,tail", [(3, 262144 + 259, 259), (40, 65536 + 67, 67), (97, 32768 + 67, 67)])
def test_gram_second_grid_stride_iteration(cuda, K, n, tail):
    """n just past blocks x chunk (1024 x 256, 1024 x 64, 512 x 64): the first blocks run the
    grid-stride loop, and its register prefetch, a second time, the last of them on a partial
    chunk. The tail columns are scaled by 30 so that a dropped chunk cannot hide in the tolerance."""
    g = torch.Generator().manual_seed(K)
    X = torch.randn(K, n, generator=g)
    X[:, n - tail:] *= 30.0
    assert_gram(X, None, cuda, f"K={K} n={n}")
    assert_gram(X, torch.randn(n, generator=g), cuda, f"K={K} n={n} centred")


# ------------------------------------------------------------------------------- 6: weighted_sum
@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_weighted_sum_vector_and_scalar_paths(cuda, n, G):
    """The float4 path (row stride a multiple of 4, 16-byte aligned pointers) and the scalar path
    (everything offset by one float, odd row stride) give the same bits, and those are the
    documented contract: every product rounded, then added in client order."""
    g = torch.Generator().manual_seed(n * 10 + G)
    src = torch.randn(G, n, generator=g)
    coeff = torch.rand(G, generator=g)
    out0 = torch.randn(n, generator=g)
    ld_v = (n + 3) // 4 * 4 + 4
    ld_s = ld_v + 1
    buf_v = torch.zeros(G, ld_v, device=cuda)
    buf_s = torch.zeros(G, ld_s, device=cuda)
    src_v, src_s = buf_v[:, :n], buf_s[:, 1:1 + n]
    src_v.copy_(src)
    src_s.copy_(src)
    assert src_v.data_ptr() % 16 == 0 and src_v.stride(0) % 4 == 0
    assert src_s.data_ptr() % 16 == 4 and src_s.stride(0) % 2 == 1
    for accumulate in (False, True):
        want = out0.clone() if accumulate else torch.zeros(n)
        for k in range(G):
            want = want + coeff[k] * src[k]  # fp32 product rounded, then fp32 add
        out_v = out0.to(cuda).clone()
        out_s = torch.zeros(n + 5, device=cuda)[1:1 + n]
        out_s.copy_(out0)
        assert out_v.data_ptr() % 16 == 0 and out_s.data_ptr() % 16 == 4
        Fn.weighted_sum(src_v, coeff.to(cuda), out_v, accumulate)
        Fn.weighted_sum(src_s, coeff.to(cuda), out_s, accumulate)
        assert torch.equal(out_v, out_s), f"paths differ (accumulate={accumulate})"
        assert torch.equal(out_v.cpu(), want), f"not the ordered sum (accumulate={accumulate})"


# ------------------------------------------------------------------ 7: broadcast_rows bf16 shadow
def test_broadcast_rows_bf16_shadow(cuda):
    """The bf16 shadow is the round-to-nearest-even conversion of the source, bit for bit, exact
    halfway cases included (fp32 denormals are left out), and the padding columns are untouched."""
    G, pad = 3, 7
    g = torch.Generator().manual_seed(7)
    normal = torch.randn(895, generator=g) * 10.0 ** torch.randint(-8, 9, (895,), generator=g).float()
    hi = torch.arange(0x3F70, 0x3F70 + 64, dtype=torch.int32)  # even and odd bf16 mantissas
    ties = ((hi << 16) | 0x8000).view(torch.float32)           # exactly halfway between two bf16
    src = torch.cat([normal, ties, -ties, torch.tensor([0.0, -0.0, 1.0, -1.0])])
    P = src.numel()
    assert P == 1027 and bool((src.abs()[src != 0] >= 2.0 ** -126).all())
    dst = torch.full((G, P + pad), -7.0, device=cuda)
    sh = torch.full((G, P + pad), -7.0, dtype=torch.bfloat16, device=cuda)
    Fn.broadcast_rows(src.to(cuda), dst[:, :P], sh[:, :P])
    want = src.to(torch.bfloat16)
    up = (want.view(torch.int16).int() & 0xFFFF) != ((src.view(torch.int32) >> 16) & 0xFFFF)
    assert int(up[895:895 + 128].sum()) == 64  # half of the ties round up (to even), half down
    assert torch.equal(dst[:, :P].cpu(), src.expand(G, P))
    assert torch.equal(sh[:, :P].cpu().contiguous().view(torch.int16), want.view(torch.int16).expand(G, P))
    assert bool((dst[:, P:] == -7.0).all()) and bool((sh[:, P:].float() == -7.0).all())
