"""Secure aggregation (csrc/kernels/secagg.hip) against the oracle of tests/secagg_oracle.py, and
through the FL engine.

The ``check_*`` functions take the device, so tests/test_secagg_cpu.py runs the same cases on the
torch twins; here they run on the kernels. Everything is integer arithmetic mod 2^32, so words, sat
and delta are compared bit for bit.

Range: the encode counts every coordinate whose rounded value leaves +-lim, so a +-inf entry of a
row with cs != 0 is counted like 1e30 (it saturates with its sign); a NaN gives q = 0 and is counted."""
import numpy as np
import pytest
import torch

import secagg_oracle as O
from test_compress_gpu import learn_run, make_fed
from test_fedopt_gpu import bits, place
from test_scaffold_gpu import padded, table
from ddl25spring_amd.data.images import synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.aggregate import SecureMean
from ddl25spring_amd.models import mnist_mlp
from ddl25spring_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

SIZES_P, SIZES_G = (1, 5, 1024, 1027), (1, 3)
SLOTS = [4, 0, 2]             # slot -> client: not the identity
COHORT5 = [4, 0, 2, 1, 3]     # the cohort of the dropout cases: clients 1 and 3 never report
N_IDS = 65536
SEED, ROUND = 0x1234567F9ABC, 3
# rows (fp32) / words (int32) layouts, as the bank layouts of test_compress_gpu: row stride P + 4
# with contiguous words, row and word stride P + 1, and both at a multiple of 4 (16-B body and
# scalar tail for any P)
LAYOUTS = ("p4", "p1", "quad")
# the mask launch uses at most 2048 blocks of 256 threads along one row (G = 1), a quad per thread:
# 5 columns more and every thread runs its loop twice, the last one on a partial quad
ROW_BLOCK_CAP = 2048
BIG_P = ROW_BLOCK_CAP * 256 * 4 + 5


def ids(lst, dev):
    return table(lst, dev, N_IDS)


def lay(rows0, dev, layout):
    """-> (rows, words): the fp32 rows and an int32 [G, P] words buffer in the layout."""
    G, P = rows0.shape
    blank = torch.full((G, P), 77, dtype=torch.int32)
    if layout == "quad":
        pad = (-P) % 4 + 4
        return padded(rows0, dev, pad), padded(blank, dev, pad)
    if layout == "p4":
        return padded(rows0, dev, 4), place(blank, dev)
    return padded(rows0, dev, 1), padded(blank, dev, 1)


def case(G, P, seed, scale=0.01):
    g_ = torch.Generator().manual_seed(seed)
    c = torch.randn(P, generator=g_)
    rows = c + scale * torch.randn(G, P, generator=g_) * torch.tensor([[1.0], [3.0], [0.3]])[:G]
    cs = torch.tensor([0.5, 0.3, 0.2])[:G].clone()
    return rows, c, cs


def run_mask(rows0, c0, cs0, slots, cohort, f, dev, layout, seed=SEED, rnd=ROUND):
    rows, words = lay(rows0, dev, layout)
    c = None if c0 is None else place(c0, dev)
    G = rows0.shape[0]
    sat = torch.full((G,), -7, dtype=torch.int32, device=dev)
    out = Fn.secagg_mask(rows, c, place(cs0, dev), ids(slots, dev), ids(cohort, dev), f, seed, rnd, words, sat)
    assert out is words and torch.equal(bits(rows), bits(rows0)), "the rows moved"
    return words, sat


def run_open(words, survivors, dropped, f, dev, seed=SEED, rnd=ROUND):
    delta = torch.full((words.shape[1],), -3.0, dtype=torch.float32, device=dev)
    out = Fn.secagg_open(words, ids(survivors, dev), ids(dropped, dev) if dropped else None, f, seed, rnd, delta)
    assert out is delta
    return delta


def same_words(got, want):
    return np.array_equal(got.detach().cpu().contiguous().numpy(), np.asarray(want, dtype=np.int32))


def same_f32(got, want):
    g = got.detach().cpu().contiguous().numpy()
    return g.shape == want.shape and np.array_equal(g.view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32))


def cohorts(G):
    """name -> (slots, cohort, dropped): the cohort equal to the local rows, and the five-client
    cohort whose other members never report."""
    slots = SLOTS[:G]
    return {"all here": (slots, list(slots), []),
            "dropped": (slots, COHORT5, [c for c in COHORT5 if c not in slots])}


# ------------------------------------------------------------ 1, 2: the oracle's bits, cancellation
def check_bit_equality(G, P, dev):
    rows0, c0, cs0 = case(G, P, 31 * G + P)
    for f in (8, 20, 30):
        for centre in (True, False):
            # without a centre the rows are the updates: small ones, so that nothing saturates at f = 30
            r0, cc = (rows0, c0) if centre else (rows0 - c0, None)
            for name, (slots, cohort, dropped) in cohorts(G).items():
                want_w, want_sat, q = O.mask(r0, cc, cs0, slots, cohort, f, SEED, ROUND)
                want_d = O.open_(want_w, slots, dropped, f, SEED, ROUND)
                assert not want_sat.any()
                for layout in LAYOUTS:
                    tag = f"G={G} P={P} f={f} centre={centre} {name} {layout}"
                    words, sat = run_mask(r0, cc, cs0, slots, cohort, f, dev, layout)
                    assert same_words(words, want_w), f"{tag}: words"
                    assert sat.cpu().tolist() == want_sat.tolist(), f"{tag}: sat"
                    delta = run_open(words, slots, dropped, f, dev)
                    assert same_f32(delta, want_d), f"{tag}: delta"
                    # cancellation: what opens is the sum of the fixed-point updates, no Philox in it
                    assert same_f32(delta, O.plain_sum(q, f)), f"{tag}: the masks did not cancel"
                    if dropped:  # one dropped client forgotten: its pair masks stay in the sum
                        wrong = run_open(words, slots, dropped[1:], f, dev)
                        assert not same_f32(wrong, O.plain_sum(q, f)), f"{tag}: a forgotten client went unnoticed"


def check_zero_weight_row(G, P, dev):
    """cs = 0 in the last row, which holds NaN and Inf: not read, not counted, words = the bare masks."""
    rows0, c0, cs0 = case(G, P, 7 * G + P)
    rows0[G - 1, 0] = float("nan")
    rows0[G - 1, P - 1] = float("inf")
    cs0[G - 1] = 0.0
    for name, (slots, cohort, dropped) in cohorts(G).items():
        want_w, want_sat, q = O.mask(rows0, c0, cs0, slots, cohort, 20, SEED, ROUND)
        assert np.array_equal(want_w[G - 1], O.bare_masks(P, slots[G - 1], cohort, SEED, ROUND))
        assert want_sat[G - 1] == 0 and not q[G - 1].any()
        for layout in LAYOUTS:
            words, sat = run_mask(rows0, c0, cs0, slots, cohort, 20, dev, layout)
            assert same_words(words, want_w) and sat.cpu().tolist() == want_sat.tolist(), (name, layout)
            assert same_f32(run_open(words, slots, dropped, 20, dev), O.plain_sum(q, 20)), (name, layout)


# ------------------------------------------------------------------------------------ 3: placement
def check_placement(P, dev):
    """Clients {4, 2} and {0} masked in separate calls (two ranks), each summed, the two partials
    stacked and opened: the bits of the single call."""
    rows0, c0, cs0 = case(3, P, 5 + P)
    dropped = [1, 3]
    for layout in LAYOUTS:
        words, _ = run_mask(rows0, c0, cs0, SLOTS, COHORT5, 20, dev, layout)
        single = run_open(words, SLOTS, dropped, 20, dev)
        wa, _ = run_mask(rows0[[0, 2]], c0, cs0[[0, 2]], [4, 2], COHORT5, 20, dev, layout)
        wb, _ = run_mask(rows0[[1]], c0, cs0[[1]], [0], COHORT5, 20, dev, layout)
        assert same_words(wa, words.cpu()[[0, 2]]) and same_words(wb, words.cpu()[[1]])
        parts = torch.full((2, P), 5, dtype=torch.int32, device=dev)
        for r, w in enumerate((wa, wb)):
            assert Fn.secagg_sum(w, parts[r]) is not None
        assert same_words(parts[0], O.to_i32(wa.cpu().numpy().astype(np.int64).sum(0)))
        stacked = run_open(parts, SLOTS, dropped, 20, dev)
        assert torch.equal(bits(stacked), bits(single)), layout
        # the strided stack too
        _, pw = lay(torch.zeros(2, P), dev, layout)
        pw.copy_(parts)
        assert torch.equal(bits(run_open(pw, SLOTS, dropped, 20, dev)), bits(single)), layout


# ---------------------------------------------------------------------------------------- 4: range
def check_range(P, dev):
    """1e30, +-inf and NaN: sat counts them in the rows with cs != 0 and nowhere else; three rows
    saturating upward at coordinate 0 open to 3 lim 2^-f, positive: the sum does not wrap."""
    f, n = 20, 3
    lim = (2 ** 31 - 1) // n
    rows0 = torch.zeros(3, P)
    rows0[:, 0] = torch.tensor([1e30, float("inf"), 3e9])
    bad = [1e30, -1e30, float("inf"), float("-inf"), float("nan")]
    expect = [1, 1, 0]  # coordinate 0 of rows 0, 1; row 2 has cs = 0 below
    for k, v in enumerate(bad):
        if 1 + k < P:
            rows0[0, 1 + k] = v
            rows0[2, 1 + k] = v
            expect[0] += 1
    cs0 = torch.tensor([1.0, 0.5, 0.0])
    want_w, want_sat, q = O.mask(rows0, None, cs0, SLOTS, SLOTS, f, SEED, ROUND)
    assert want_sat.tolist() == expect
    for layout in LAYOUTS:
        words, sat = run_mask(rows0, None, cs0, SLOTS, SLOTS, f, dev, layout)
        assert same_words(words, want_w) and sat.cpu().tolist() == expect, layout
    cs0 = torch.ones(3)
    rows0[2] = rows0[0]
    for layout in LAYOUTS:
        words, sat = run_mask(rows0, None, cs0, SLOTS, SLOTS, f, dev, layout)
        delta = run_open(words, SLOTS, [], f, dev).cpu()
        assert delta[0].item() == float(np.float32(3 * lim) * np.float32(2.0 ** -f)) and delta[0].item() > 0, layout
        assert all(s >= 1 for s in sat.cpu().tolist())


# ------------------------------------------------------------------------------------- 5: accuracy
def check_accuracy(G, P, dev):
    """Against float64: one rounding to the grid per client, the two fp32 roundings of d and p, and
    the final conversion."""
    rows0, c0, cs0 = case(G, P, 13 * G + P, scale=0.5)
    for f in (8, 20):
        for name, (slots, cohort, dropped) in cohorts(G).items():
            deltas = [run_open(run_mask(rows0, c0, cs0, slots, cohort, f, dev, layout)[0], slots, dropped, f, dev)
                      for layout in LAYOUTS]
            assert all(torch.equal(bits(d), bits(deltas[0])) for d in deltas)
            delta = deltas[0].cpu().double().numpy()
            u = (rows0.double() - c0.double()).numpy() * cs0.double().numpy()[:, None]
            err = np.abs(delta - u.sum(0))
            bound = G * 2.0 ** -(f + 1) + 2.0 ** -22 * np.abs(u).sum(0) + 2.0 ** -24 * np.abs(delta)
            print(f"accuracy G={G} P={P} f={f} {name}: worst err / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (f, name, float((err / bound).max()))


# ---------------------------------------------------------------------------------- 6: grid stride
def check_second_pass(dev):
    """P just past what one grid covers in one stride, plus 5; G = 1, n = 2. The last 5 columns hold
    the largest updates."""
    g_ = torch.Generator().manual_seed(3)
    rows0 = 0.01 * torch.randn(1, BIG_P, generator=g_)
    rows0[0, -5:] = torch.tensor([3.0, -4.0, 5.0, -6.0, 7.0])
    cs0 = torch.tensor([0.75])
    want_w, want_sat, q = O.mask(rows0, None, cs0, [1], [0, 1], 20, SEED, ROUND)
    rows = place(rows0, dev)
    words = torch.zeros(1, BIG_P, dtype=torch.int32, device=dev)
    sat = torch.zeros(1, dtype=torch.int32, device=dev)
    Fn.secagg_mask(rows, None, place(cs0, dev), ids([1], dev), ids([0, 1], dev), 20, SEED, ROUND, words, sat)
    assert same_words(words, want_w) and sat.cpu().tolist() == [0]
    part = torch.zeros(BIG_P, dtype=torch.int32, device=dev)
    Fn.secagg_sum(words, part)
    assert same_words(part, want_w[0])
    delta = run_open(words, [1], [0], 20, dev)
    assert same_f32(delta, O.plain_sum(q, 20))
    assert delta.cpu()[-5:].tolist() == [2.25, -3.0, 3.75, -4.5, 5.25]
    if torch.device(dev).type == "cuda":
        from ddl25spring_amd.ops import _lib
        assert _lib.kernels().ddl_secagg_row_blocks(1, BIG_P) == ROW_BLOCK_CAP
        assert BIG_P > ROW_BLOCK_CAP * 256 * 4


# -------------------------------------------------------------------------------- 7: odds and ends
def check_deterministic(dev):
    rows0, c0, cs0 = case(3, 1027, 41)
    a, b = [], []
    for outs in (a, b):
        words, sat = run_mask(rows0, c0, cs0, SLOTS, COHORT5, 20, dev, "quad")
        outs += [words.float(), sat.float(), run_open(words, SLOTS, [1, 3], 20, dev)]
    for s, t in zip(a, b):
        assert torch.equal(bits(s), bits(t))


def check_rejects(dev):
    """The op validates its scalars, and the contents of host tables."""
    rows, c, cs = torch.zeros(2, 8, device=dev), torch.zeros(8, device=dev), torch.ones(2, device=dev)
    words = torch.full((2, 8), 9, dtype=torch.int32, device=dev)
    sat = torch.full((2,), 9, dtype=torch.int32, device=dev)
    delta = torch.full((8,), 9.0, device=dev)
    t = ids([0, 2], dev)
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    for f in (7, 31):
        with pytest.raises(ValueError):
            Fn.secagg_mask(rows, c, cs, t, t, f, 0, 0, words, sat)
        with pytest.raises(ValueError):
            Fn.secagg_open(words, t, None, f, 0, 0, delta)
    with pytest.raises(ValueError):
        Fn.secagg_open(words, empty, None, 20, 0, 0, delta)
    for bad in ([0, 65536], [1, 1], [-1, 2]):
        with pytest.raises(ValueError):
            Fn.secagg_ids(bad)
    for kw in (dict(frac_bits=7), dict(frac_bits=31), dict(min_survivors=0), dict(noise_multiplier=1.0, weighting="uniform"),
               dict(clip=0.0)):
        with pytest.raises(ValueError):
            SecureMean(**kw)
    assert not bool((words != 9).any()) and not bool((sat != 9).any()) and not bool((delta != 9.0).any())


@pytest.mark.parametrize("P", SIZES_P)
@pytest.mark.parametrize("G", SIZES_G)
def test_words_sat_and_delta_equal_the_oracle(cuda, G, P):
    check_bit_equality(G, P, cuda)


@pytest.mark.parametrize("P", SIZES_P)
@pytest.mark.parametrize("G", SIZES_G)
def test_zero_weight_row_uploads_bare_masks(cuda, G, P):
    check_zero_weight_row(G, P, cuda)


@pytest.mark.parametrize("P", SIZES_P)
def test_placement_does_not_change_a_bit(cuda, P):
    check_placement(P, cuda)


@pytest.mark.parametrize("P", SIZES_P)
def test_range_saturates_and_counts(cuda, P):
    check_range(P, cuda)


@pytest.mark.parametrize("P", SIZES_P)
@pytest.mark.parametrize("G", SIZES_G)
def test_accuracy_against_float64(cuda, G, P):
    check_accuracy(G, P, cuda)


def test_second_grid_stride_iteration(cuda):
    check_second_pass(cuda)


@pytest.mark.parametrize("G", (2, 3, 8, 9))
def test_pair_shared_and_plain_forms_agree(cuda, G):
    """The mask kernel's two forms (a pair of local clients costs one Philox call in the shared one,
    which takes 2..8 rows; 9 falls back to the plain form) give the oracle's bits, for a cohort of
    local clients only and one with members elsewhere, over the three layouts and a second stride."""
    clients = [7, 1, 12, 3, 65535, 0, 9, 5, 300][:G]
    # the second stride of the shared form's one grid (all rows in a thread) needs BIG_P: at G = 2 only
    for P, layouts in [(1027, LAYOUTS), (5, LAYOUTS)] + ([(BIG_P, ("quad",))] if G == 2 else []):
        g_ = torch.Generator().manual_seed(G + P)
        rows0, c0 = 0.01 * torch.randn(G, P, generator=g_), None
        rows0[G - 1, 0] = 1e30
        cs0 = torch.linspace(0.1, 1.0, G)
        cs0[0] = 0.0 if P == 5 else cs0[0]
        for cohort in (clients, [2, 65534] + clients[::-1]) if P != BIG_P else (clients,):
            want_w, want_sat, _ = O.mask(rows0, c0, cs0, clients, cohort, 20, SEED, ROUND)
            for layout in layouts:
                for shared in (False, True):
                    rows, words = lay(rows0, cuda, layout)
                    sat = torch.full((G,), -7, dtype=torch.int32, device=cuda)
                    Fn.secagg_mask(rows, c0, place(cs0, cuda), ids(clients, cuda), ids(cohort, cuda), 20, SEED, ROUND,
                                   words, sat, pair_shared=shared)
                    assert same_words(words, want_w), (P, layout, shared, len(cohort))
                    assert sat.cpu().tolist() == want_sat.tolist(), (P, layout, shared)


def test_two_calls_are_bit_equal(cuda):
    check_deterministic(cuda)


def test_op_rejects_bad_arguments(cuda):
    check_rejects(cuda)


def test_kernel_rejects_bad_arguments(cuda):
    """Null pointers, G < 1, P < 1, ld < P, frac_bits outside 8..30, n < 1 and n > 65536 come back as
    hipErrorInvalidValue (1); nothing is launched, the buffers stay as they were."""
    from ddl25spring_amd.ops import _lib
    lib = _lib.kernels()
    x = torch.zeros(3, 8, device=cuda)
    w = torch.full((3, 8), 9, dtype=torch.int32, device=cuda)
    i = torch.zeros(4, dtype=torch.int32, device=cuda)
    sat = torch.full((3,), 9, dtype=torch.int32, device=cuda)
    d = torch.full((8,), 9.0, device=cuda)
    xp, wp, ip, sp, dp, s = x.data_ptr(), w.data_ptr(), i.data_ptr(), sat.data_ptr(), d.data_ptr(), _lib.stream()
    #       X   ld  c   cs  slot G  P  cohort n  f   seed rnd words ldw sat shared
    good = [xp, 8, xp, xp, ip, 2, 8, ip, 2, 20, 5, 0, wp, 8, sp, 0, s]
    for shared in (0, 1):
        for pos, bad in ((0, None), (3, None), (4, None), (7, None), (12, None), (14, None), (5, 0), (6, 0), (1, 7),
                         (13, 7), (9, 7), (9, 31), (8, 0), (8, 65537)):
            args = list(good)
            args[pos], args[15] = bad, shared
            assert lib.ddl_secagg_mask(*args) == 1, (pos, shared)
    #       words ldw R  P  out
    good = [wp, 8, 2, 8, wp + 64, s]
    for pos, bad in ((0, None), (4, None), (2, 0), (3, 0), (1, 7)):
        args = list(good)
        args[pos] = bad
        assert lib.ddl_secagg_sum(*args) == 1, pos
    #       words ldw R  P  surv ns drop nd f  seed rnd delta
    good = [wp, 8, 2, 8, ip, 2, ip, 1, 20, 5, 0, dp, s]
    for pos, bad in ((0, None), (4, None), (11, None), (2, 0), (3, 0), (1, 7), (5, 0), (7, -1), (6, None), (8, 7),
                     (8, 31), (5, 65536)):
        args = list(good)
        args[pos] = bad
        assert lib.ddl_secagg_open(*args) == 1, pos
    torch.cuda.synchronize()
    assert not bool((w != 9).any()) and not bool((sat != 9).any()) and not bool((d != 9.0).any()) and not bool(x.any())


# ------------------------------------------------------------------------------------- the engine
def secure_fed(dev, f=20, **kw):
    agg = dict(frac_bits=f)
    agg.update(kw.pop("agg_kwargs", {}))
    return make_fed(dev, aggregator="secagg", agg_kwargs=agg, **kw)


def check_round_one_against_mean(dev, f=20):
    """Round 1 of secagg against round 1 of the plain mean, same seed: no dropout, then one where
    the engine's own RNG drops a client of the cohort."""
    for kw in (dict(), dict(dropout=0.5, seed=7)):
        sec, mean = secure_fed(dev, f, **kw), make_fed(dev, **kw)
        sec.round()
        mean.round()
        K = sec.K - len(sec.dropped[0]) if kw else sec.K
        if kw:
            assert sec.dropped[0] and K >= 2 and sec.dropped == mean.dropped
            assert sorted(sec.cohort) == [0, 1, 2, 3]
        assert sec.aggregator.aborted == [] and sec.aggregator.last_k == K
        up = sec.aggregator.last_uploads
        assert up.dtype == torch.int32 and tuple(up.shape) == (K, sec.w_global.numel())
        assert sec.aggregator.last_saturated == [0] * K
        w_max = float(sec.net.store.data[:K].abs().max())
        err = float((sec.w_global.double() - mean.w_global.double()).abs().max())
        bound = K * 2.0 ** -(f + 1) + (K + 4) * 2.0 ** -23 * w_max
        print(f"secagg vs mean, {kw or 'no dropout'}: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)
        assert bound < 2.0 ** (31 - f) / 1e6  # a wrong reconstruction is off by the order of 2^(31 - f)


def check_abort(dev):
    """dropout = 0.5, seed = 3: round 2 has the lone survivor [3]; nothing is opened."""
    fa = secure_fed(dev, dropout=0.5, seed=3)
    fa.round()
    before = fa.w_global.clone()
    assert fa.aggregator.aborted == []
    fa.round()
    assert sorted(fa.dropped[1]) == [0, 1, 2]
    assert torch.equal(bits(fa.w_global), bits(before))
    assert fa.aggregator.aborted == [1] and fa.aggregator.rounds == 2 and fa.aggregator.last_uploads is None


def test_round_one_tracks_the_plain_mean(cuda):
    check_round_one_against_mean(cuda)


def test_lone_survivor_aborts_the_round(cuda):
    check_abort(cuda)


def test_secagg_device_engine_tracks_cpu_engine(cuda):
    """The criterion of test_compressed_device_engine_tracks_cpu_engine, over two rounds."""
    arr = synthetic_images("mnist", 600, seed=0)
    parts = split(4, True, 1, labels=arr.labels)
    runs = []
    for dev in (torch.device("cpu"), cuda):
        fa = secure_fed(dev, model=mnist_mlp, arr=arr, parts=parts, lr=0.05, client_fraction=0.5, seed=1)
        fa.round()
        fa.round()
        runs.append(fa.w_global.float().cpu())
        assert fa.aggregator.rounds == 2 and fa.aggregator.aborted == []
    cpu, gpu = runs
    rel = ((cpu - gpu).norm() / cpu.norm()).item()
    assert rel < 2e-2, rel


def test_secagg_fedavg_learns_on_device(cuda):
    """10 IID clients, C = 0.5, MnistCnn, 8 rounds with dropout 0.2: >= 80 %, the bar of the codecs."""
    acc, _, _ = learn_run(cuda, aggregator="secagg", agg_kwargs=dict(frac_bits=20), dropout=0.2)
    print(f"secagg: accuracy per round {acc}")
    assert acc[-1] >= 80.0, acc
