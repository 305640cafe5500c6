"""Colluding attacks (csrc/kernels/collude.hip: per-coordinate moments of the source updates, ALIE and
IPM vectors written to the colluders' rows) against the float64 oracle of tests/collude_oracle.py.

The ``check_*`` functions take the device, so tests/test_collude_cpu.py runs the same cases on the
torch twin; here they run on the kernel."""
import math

import numpy as np
import pytest
import torch

import collude_oracle as CO
import robust_oracle as O
from test_clipped_agg_gpu import BIG_N, centers
from ddl25spring_amd.fl import attacks as AT
from ddl25spring_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 7, 33, 200)
NN = (1, 3, 4, 5, 255, 1027)
COEFS = (0.31864, 1.5)
MODES = (("alie", CO.ALIE), ("ipm", CO.IPM))


def place(S, extra, dev, strided):
    """The sources in a buffer of ns + extra rows, in a shuffled row order -> (buffer, src_rows)."""
    ns, n = S.shape
    g = torch.Generator().manual_seed(ns * 7919 + n)
    perm = torch.randperm(ns + extra, generator=g)[:ns].tolist()
    buf = torch.full((ns + extra, n), 777.0)
    buf[perm] = S
    return (O.strided(buf, dev) if strided else buf.to(dev)), perm


def assert_rows(S, c, c_dev, buf, src_rows, mode, coef, tag):
    """Out of place into rows 2 and 0 of a 3-row buffer; row 1 stays. -> the written row."""
    dev, n = buf.device, S.shape[1]
    name, m = mode
    dst = torch.full((3, n), -5.0, device=dev)
    Fn.collude_rows(buf, src_rows, c_dev, dst, [2, 0], name, coef)
    assert torch.equal(dst[0], dst[2]) and bool((dst[1] == -5.0).all()), tag
    want, bound = CO.malicious(S, c, m, coef)
    base = 0.0 if c is None else c.double().numpy()
    err = np.abs(dst[0].cpu().double().numpy() - (base + want))
    lim = CO.row_bound(c, want, bound)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    print(f"collude {tag}: worst err / bound = {worst:.3f}")
    assert bool((err <= lim).all()), f"{tag}: err / bound = {worst}"
    return dst[0].clone()


# ------------------------------------------------------------------------ 1: kernel against oracle
def check_against_oracle(ns, dev):
    for n in NN:
        g = torch.Generator().manual_seed(1000 * ns + n)
        c = torch.randn(n, generator=g)
        U = 0.3 * torch.randn(n, generator=g) + torch.randn(n, generator=g).exp() * torch.randn(ns, n, generator=g)
        for tag, c_dev, c_host in centers(c, dev):
            S = U if c_host is None else c + U
            for mode in MODES:
                for coef in COEFS:
                    t = f"ns={ns} n={n} {tag} {mode[0]} coef={coef}"
                    a = assert_rows(S, c_host, c_dev, *place(S, 2, dev, False), mode, coef, t)
                    b = assert_rows(S, c_host, c_dev, *place(S, 2, dev, True), mode, coef, t + " strided")
                    assert torch.equal(a, b), f"{t}: vector and scalar paths differ"


@pytest.mark.parametrize("ns", NS)
def test_collude_against_oracle(cuda, ns):
    check_against_oracle(ns, cuda)


# ------------------------------------------------------------------------------- 2: exact cases
def check_exact(dev):
    n = 1027
    g = torch.Generator().manual_seed(5)
    c = torch.randn(n, generator=g)
    row = c + torch.randn(n, generator=g)
    mu = row - c  # fl32(x - c): the mean of identical rows, exactly
    for ns in (1, 2, 5, 33):
        S = row.repeat(ns, 1).to(dev)
        for c_dev, want in ((c.to(dev), c + mu), (None, row)):
            dst = torch.empty(1, n, device=dev)
            for coef in COEFS:  # sigma == 0 exactly: z does not matter
                Fn.collude_rows(S, list(range(ns)), c_dev, dst, [0], "alie", coef)
                assert torch.equal(dst[0].cpu(), want), f"alie ns={ns} coef={coef}"
            Fn.collude_rows(S, list(range(ns)), c_dev, dst, [0], "ipm", -1.0)
            assert torch.equal(dst[0].cpu(), want), f"ipm ns={ns}"
    # IPM with eps = 0 writes exactly the centre
    S = (c + torch.randn(7, n, generator=g)).to(dev)
    dst = torch.empty(2, n, device=dev)
    Fn.collude_rows(S, list(range(7)), c.to(dev), dst, [0, 1], "ipm", 0.0)
    assert torch.equal(dst[0].cpu(), c) and torch.equal(dst[1].cpu(), c)
    # no source row at all: the centre (zero without one)
    Fn.collude_rows(S, [], c.to(dev), dst, [1], "alie", 1.0)
    assert torch.equal(dst[1].cpu(), c)
    Fn.collude_rows(S, [], None, dst, [1], "alie", 1.0)
    assert not bool(dst[1].any())
    with pytest.raises(ValueError):
        Fn.collude_rows(S, [7], None, dst, [0], "alie", 1.0)  # a source row past the buffer
    with pytest.raises(ValueError):
        Fn.collude_rows(S, [0], None, dst, [2], "alie", 1.0)


def test_exact_cases(cuda):
    check_exact(cuda)


# --------------------------------------------------------------------------- 3: hostile sources
def check_hostile(dev):
    ns, n = 7, 261
    g = torch.Generator().manual_seed(8)
    c = torch.randn(n, generator=g)
    S = c + torch.randn(ns, n, generator=g)
    nan, inf = float("nan"), float("inf")
    S[0, 3] = nan                      # the first row: the shift comes from the second
    S[2, 4], S[5, 4] = inf, -inf
    S[:, 9] = nan                      # no finite source
    S[:, 130] = torch.tensor([nan, inf, -inf, nan, inf, -inf, nan])
    S[:6, 200] = nan                   # one finite source, the last
    S[1:, 260] = inf                   # one finite source, the first; in the scalar tail
    S[3, 100:140] = nan
    for tag, c_dev, c_host in centers(c, dev):
        Sx = S if c_host is not None else S - c
        mu, sigma, m = CO.moments(Sx, c_host)
        assert m[3] == 6 and m[4] == 5 and m[9] == 0 and m[130] == 0 and m[200] == 1 and m[260] == 1
        for mode in MODES:
            for strided in (False, True):
                row = assert_rows(Sx, c_host, c_dev, *place(Sx, 1, dev, strided), mode, 1.5, f"hostile {tag} {mode[0]}")
                assert bool(torch.isfinite(row).all())
                want = c if c_host is not None else torch.zeros(n)
                assert torch.equal(row.cpu()[[9, 130]], want[[9, 130]])  # no finite source: the centre


def test_hostile_sources(cuda):
    check_hostile(cuda)


# ------------------------------------------------------------------------------------ 4: in place
def check_in_place(dev):
    K, n = 9, 1027
    g = torch.Generator().manual_seed(4)
    c = torch.randn(n, generator=g)
    X = c + torch.randn(K, n, generator=g)
    for strided in (False, True):
        buf = lambda: O.strided(X, dev) if strided else X.to(dev)
        for mode, coef in (("alie", 1.5), ("ipm", 0.5)):
            for src_rows, dst_rows in (([0, 2, 3, 5, 8], [1, 6]),      # disjoint (knowledge="benign")
                                       ([6, 1, 4], [6, 1, 4]),         # the same rows (knowledge="own")
                                       ([0, 1, 2, 3], [3, 7])):        # overlapping
                src = buf()
                out = torch.zeros(len(dst_rows), n, device=dev)
                Fn.collude_rows(src, src_rows, c.to(dev), out, list(range(len(dst_rows))), mode, coef)
                before = src.clone()
                Fn.collude_rows(src, src_rows, c.to(dev), src, dst_rows, mode, coef)
                for t, r in enumerate(dst_rows):
                    assert torch.equal(src[r], out[t]), (mode, src_rows, dst_rows)
                rest = [r for r in range(K) if r not in dst_rows]
                assert torch.equal(src[rest], before[rest])


def test_in_place(cuda):
    check_in_place(cuda)


# --------------------------------------------------------------- 5: paths and reproducibility
def check_paths(dev):
    ns, n = 5, 4099
    g = torch.Generator().manual_seed(6)
    c = torch.randn(n, generator=g)
    S = c + torch.randn(ns, n, generator=g)
    for mode in ("alie", "ipm"):
        outs = []
        for shift in (0, 1, 0):  # aligned base, a base one float past a 16-B boundary, aligned again
            src = torch.zeros(ns, n + 5 + shift, device=dev)[:, shift:shift + n]  # n + 5: a multiple of 4
            src.copy_(S)
            dst = torch.zeros(2, n + 5 + shift, device=dev)[:, shift:shift + n]
            if dev.type == "cuda":
                assert src.data_ptr() % 16 == 4 * shift and src.stride(0) % 4 == shift
            Fn.collude_rows(src, list(range(ns)), c.to(dev), dst, [0, 1], mode, 0.7)
            outs.append(dst[0].clone())
        assert torch.equal(outs[0], outs[1]), "16-B path and element path differ"
        assert torch.equal(outs[0], outs[2]), "two calls differ"


def check_second_pass(dev):
    """n just past the streaming kernels' grid cap (8192 blocks x 256 threads x 4): a second
    grid-stride pass that ends on a partial quad. The tail is scaled by 30 so that a dropped element
    cannot hide in the tolerance."""
    g = torch.Generator().manual_seed(3)
    S = torch.randn(2, BIG_N, generator=g)
    S[:, BIG_N - 5:] *= 30.0
    c = torch.randn(BIG_N, generator=g)
    dst = torch.empty(1, BIG_N, device=dev)
    Fn.collude_rows(S.to(dev), [0, 1], c.to(dev), dst, [0], "alie", 1.5)
    want, bound = CO.malicious(S, c, CO.ALIE, 1.5)
    err = np.abs(dst[0].cpu().double().numpy() - (c.double().numpy() + want))
    assert bool((err <= CO.row_bound(c, want, bound)).all())
    assert float(np.abs(want[BIG_N - 5:]).min()) > 0.0


def test_paths_and_two_calls_are_bit_equal(cuda):
    check_paths(cuda)


def test_second_grid_stride_iteration(cuda):
    check_second_pass(cuda)


# ----------------------------------------------------------------------------- 6: attack classes
def check_attack_classes(dev):
    K, P = 8, 1027
    bad = {1, 6}
    g = torch.Generator().manual_seed(12)
    c = torch.randn(P, generator=g)
    X = c + 0.1 * torch.randn(K, P, generator=g)
    clients = [10, 1, 12, 13, 14, 15, 6, 17]  # slot order; clients 1 and 6 are the colluders
    for knowledge in ("benign", "own"):
        srcs = [i for i, cl in enumerate(clients) if (cl in bad) == (knowledge == "own")]
        for atk, mode, coef in ((AT.make_attack("alie", bad, knowledge=knowledge), CO.ALIE, AT.alie_z_max(8, 2)),
                                (AT.make_attack("alie", bad, z=1.5, knowledge=knowledge), CO.ALIE, 1.5),
                                (AT.make_attack("ipm", bad, knowledge=knowledge), CO.IPM, 0.5),
                                (AT.make_attack("ipm", bad, eps=2.0, knowledge=knowledge), CO.IPM, 2.0)):
            assert atk.collective and atk.state_dict() == {}
            rows = O.strided(X, dev)
            atk.poison_updates(rows, c.to(dev), clients)
            got = rows.cpu()
            assert torch.equal(got[1], got[6])
            keep = [i for i in range(K) if clients[i] not in bad]
            assert torch.equal(got[keep], X[keep])
            want, bound = CO.malicious(X[srcs], c, mode, coef)
            err = np.abs(got[1].double().numpy() - (c.double().numpy() + want))
            assert bool((err <= CO.row_bound(c, want, bound)).all()), (knowledge, mode, coef)
    # no colluder in the round: nothing is done
    rows = X.to(dev)
    AT.ALIE({99}).poison_updates(rows, c.to(dev), clients)
    assert torch.equal(rows.cpu(), X)
    # only colluders and knowledge="benign": no source row, they send the centre
    rows = X[:2].to(dev)
    AT.IPM({1, 6}).poison_updates(rows, c.to(dev), [6, 1])
    assert torch.equal(rows.cpu(), c.repeat(2, 1))


def test_attack_classes(cuda):
    check_attack_classes(cuda)
