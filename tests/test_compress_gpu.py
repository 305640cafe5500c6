"""Compressed client uploads (csrc/kernels/compress.hip) against the oracle of
tests/compress_oracle.py, and through the FL engine.

The ``check_*`` functions take the device, so tests/test_compress_cpu.py runs the same cases on the
torch twins; here they run on the kernels. Top-k is exact, so rows, bank and nnz are compared bit for
bit (a NaN against a NaN). Quantization: scales bit for bit, levels against the float64 a* and the
oracle's Philox draw."""
import numpy as np
import pytest
import torch

import compress_oracle as O
from test_fedopt_gpu import bits, place
from test_scaffold_gpu import padded, table
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.algorithms import FedAvg
from ddl25spring_amd.fl.compress import Quantize, TopK
from ddl25spring_amd.models import mnist_cnn, mnist_mlp
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

TOPK_P, TOPK_G = (1, 5, 1024, 1027), (1, 3)
QUANT_P, QUANT_BITS = (1, 5, 256, 257, 1024, 1027), (2, 4, 8)
TABLE = [4, 0, 2]  # slot -> client: not the identity, 5 bank rows
N_BANK = 5
# the codec's launches use at most 2048 blocks of 256 threads along one row (G = 1), a quad per
# thread: 5 columns more and every thread runs its loop twice, the last one on a partial quad
ROW_BLOCK_CAP = 2048
BIG_P = ROW_BLOCK_CAP * 256 * 4 + 5
BAD_AT = {0: float("nan"), 5: float("inf"), 1023: float("-inf"), 1024: float("nan"), 1026: float("inf")}
# bank / row layouts: the bank as a view of row stride P + 4 and P + 1 (rows contiguous), and rows
# and bank both at a stride that is a multiple of 4 (16-B body and scalar tail for any P)
LAYOUTS = ("p4", "p1", "quad")


def lay(rows0, bank0, dev, layout):
    P = rows0.shape[1]
    if layout == "quad":
        pad = (-P) % 4 + 4
        return padded(rows0, dev, pad), None if bank0 is None else padded(bank0, dev, pad)
    return place(rows0, dev), None if bank0 is None else padded(bank0, dev, 4 if layout == "p4" else 1)


def same_bits(got, want):
    """Bit equality of a tensor and the oracle's float32 array; a NaN matches any NaN."""
    g = got.detach().cpu().contiguous().numpy()
    w = np.asarray(want, dtype=np.float32)
    assert g.shape == w.shape
    nan = np.isnan(w)
    return bool(np.array_equal(np.isnan(g), nan)) and bool(np.array_equal(O.ubits(g)[~nan], O.ubits(w)[~nan]))


# ------------------------------------------------------------------------------------ 1: top-k
def base_case(G, P, seed):
    """x, trained rows at scales 1, 10, 100 x 0.01 (so each row has its own tau) and a 5-row bank."""
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(P, generator=g_)
    scale = torch.tensor([[0.01], [0.1], [1.0]])[:G]
    y = x + scale * torch.randn(G, P, generator=g_)
    bank = 0.005 * torch.randn(N_BANK, P, generator=g_) * torch.arange(1.0, N_BANK + 1)[:, None]
    return y, x, bank


def from_bits(b):
    return torch.from_numpy(np.asarray(b, dtype=np.uint32).view(np.float32).copy())


def exact_case(G, P, mags):
    """x = 0 and a zero bank: u is y itself, so the magnitudes are exactly the bit patterns given
    (signs alternate in pairs, rows rotated against each other)."""
    j = np.arange(P)
    rows = []
    for g in range(G):
        m = np.roll(np.asarray(mags, dtype=np.uint32), g)
        rows.append(from_bits(m | (((j // 2 + g) % 2).astype(np.uint32) << np.uint32(31))))
    return torch.stack(rows), torch.zeros(P), torch.zeros(N_BANK, P)


def topk_cases(G, P):
    """name -> (y, x, bank, k, expectation or None)."""
    j = np.arange(P, dtype=np.uint32)
    y, x, bank = base_case(G, P, 17 * G + P)
    cases = {"random": (y, x, bank, max(1, P // 10), None),
             "k=1": (y, x, bank, 1, None),
             "k=P": (y, x, bank, P, "all")}
    # fewer non-zeros than k: y = x and a zero bank but for two entries per client
    sp_bank = torch.zeros(N_BANK, P)
    sp_bank[:, 0] = torch.arange(1.0, N_BANK + 1)
    sp_bank[:, P - 1] = -0.5
    cases["k > non-zeros"] = (x.repeat(G, 1), x, sp_bank, max(3, P // 2), "sparse")
    zero = y.clone()
    zero[0] = x
    zb = bank.clone()
    zb[TABLE[0]] = 0.0
    cases["all-zero row"] = (zero, x, zb, 2, "row0 empty")
    one, two = np.float32(1.0).view(np.uint32), np.float32(2.0).view(np.uint32)
    cases["ties"] = exact_case(G, P, np.where(j % 2 == 1, two, one)) + (1, "ties")
    cases["lowest digit"] = exact_case(G, P, np.uint32(0x3F800000) + (j * np.uint32(7)) % np.uint32(1024)) \
        + (max(1, P // 3), None)
    cases["highest digit"] = exact_case(G, P, ((j * np.uint32(13)) % np.uint32(2000) + np.uint32(20)) << np.uint32(20)) \
        + (max(1, P // 3), None)
    cases["subnormal"] = exact_case(G, P, (j * np.uint32(2654435761)) % np.uint32(0x7FFFFF) + np.uint32(1)) \
        + (max(1, P // 4), None)
    bad = y.clone()
    for i, v in BAD_AT.items():
        if i < P:
            bad[G - 1, i] = v
    cases["non-finite"] = (bad, x, bank, max(1, P // 10), "non-finite")
    return cases


def run_topk(y0, x0, bank0, ids, k, dev, layout):
    rows, bank = lay(y0, bank0, dev, layout)
    x = place(x0, dev)
    nnz = torch.full((y0.shape[0],), -7, dtype=torch.int32, device=dev)
    out = Fn.topk_compress(rows, x, bank, None if bank is None else table(ids, dev, N_BANK), k, nnz)
    assert out is nnz and torch.equal(bits(x), bits(x0)), "x moved"
    return rows, bank, nnz


def check_topk(G, P, dev):
    ids = TABLE[:G]
    for name, (y0, x0, bank0, k, expect) in topk_cases(G, P).items():
        for with_bank in (True, False):
            b0 = bank0 if with_bank else None
            want_rows, want_bank, want_nnz = O.topk(y0, x0, b0, ids, k)
            for layout in LAYOUTS if with_bank else ("p4", "quad"):
                tag = f"top-k {name} G={G} P={P} k={k} bank={with_bank} {layout}"
                rows, bank, nnz = run_topk(y0, x0, b0, ids, k, dev, layout)
                assert same_bits(rows, want_rows), f"{tag}: rows"
                assert nnz.cpu().tolist() == want_nnz.tolist(), f"{tag}: nnz {nnz.cpu().tolist()} != {want_nnz.tolist()}"
                if with_bank:  # the whole bank: the rows outside the table are bit-unchanged too
                    assert same_bits(bank, want_bank), f"{tag}: bank"
        # what the case is there for, on the oracle's result (which the code equals)
        u = np.stack([O.corrected(y0[g], x0, bank0[ids[g]]) for g in range(G)])
        _, _, counts = O.magnitudes(u.reshape(-1))
        counts = counts.reshape(G, P).sum(1)
        _, _, nnz = O.topk(y0, x0, bank0, ids, k)
        if expect is None and name in ("random", "k=1"):
            assert nnz.tolist() == [min(k, P)] * G
        elif expect == "all":
            assert nnz.tolist() == counts.tolist() == [P] * G
        elif expect == "sparse":
            assert nnz.tolist() == counts.tolist() == [min(2, P)] * G and k > 2
        elif expect == "row0 empty":
            assert nnz[0] == 0 and counts[0] == 0
            r, b, _ = O.topk(y0, x0, bank0, ids, k)
            assert np.array_equal(O.ubits(r[0]), O.ubits(O.f32(x0)))
        elif expect == "ties" and P >= 5:
            assert bool((nnz > k).all()), nnz
            r, _, _ = O.topk(y0, x0, bank0, ids, k)
            assert (r[0] == 2.0).any() and (r[0] == -2.0).any()  # a +- pair at tau, both kept
        elif expect == "non-finite":
            bad = [i for i in BAD_AT if i < P]
            r, b, _ = O.topk(y0, x0, bank0, ids, k)
            assert not np.isfinite(r[G - 1, bad]).any()
            assert np.array_equal(O.ubits(b[ids[G - 1]])[bad], O.ubits(O.f32(bank0[ids[G - 1]]))[bad])
            assert counts[G - 1] == P - len(bad)


def check_topk_without_bank_drops(dev):
    """No bank: the dropped part vanishes. The row holds x but for the kept entries, and a second
    call on the result selects the same entries again (nothing came back)."""
    y0, x0, _ = base_case(3, 1027, 5)
    rows, _, nnz = run_topk(y0, x0, None, TABLE, 100, dev, "quad")
    moved = (rows.cpu() != x0[None, :]).sum(1)
    assert nnz.cpu().tolist() == [100] * 3 and moved.tolist() == [100] * 3
    again = rows.cpu().clone()
    rows2, _, nnz2 = run_topk(again, x0, None, TABLE, 100, dev, "quad")
    assert bool((nnz2.cpu() <= 100).all()) and bool(((rows2.cpu() != x0[None, :]) <= (again != x0[None, :])).all())


def check_topk_second_pass(dev):
    """P just past the row's grid cap; the 5 largest magnitudes sit in the last 5 columns, so a
    dropped tail changes tau and every kept entry."""
    g_ = torch.Generator().manual_seed(3)
    x0 = torch.randn(BIG_P, generator=g_)
    y0 = (x0 + 0.01 * torch.randn(BIG_P, generator=g_))[None, :].clone()
    y0[0, -5:] = x0[-5:] + torch.tensor([3.0, -4.0, 5.0, -6.0, 7.0])
    bank0 = torch.zeros(2, BIG_P)
    bank0[1] = 0.001 * torch.randn(BIG_P, generator=g_)
    want_rows, want_bank, want_nnz = O.topk(y0, x0, bank0, [1], 5)
    assert want_nnz.tolist() == [5] and (want_rows[0, :-5] == x0.numpy()[:-5]).all()
    rows, bank = place(y0, dev), place(bank0, dev)
    nnz = torch.zeros(1, dtype=torch.int32, device=dev)
    Fn.topk_compress(rows, place(x0, dev), bank, table([1], dev, 2), 5, nnz)
    assert nnz.cpu().tolist() == [5]
    assert same_bits(rows, want_rows) and same_bits(bank, want_bank)
    if torch.device(dev).type == "cuda":
        from ddl25spring_amd.ops import _lib
        assert _lib.kernels().ddl_compress_row_blocks(1, BIG_P) == ROW_BLOCK_CAP
        assert BIG_P > ROW_BLOCK_CAP * 256 * 4


# ------------------------------------------------------------------------------- 2: quantization
SEED, ROUND = 0x1234567F9ABC, 3


def run_quant(y0, x0, bank0, ids, bits_, dev, layout, seed=SEED, rnd=ROUND, n_bank=N_BANK):
    rows, bank = lay(y0, bank0, dev, layout)
    G, P = y0.shape
    levels = torch.full((G, P), 99, dtype=torch.int8, device=dev)
    scales = torch.full((G, (P + 255) // 256), -1.0, dtype=torch.float32, device=dev)
    x = place(x0, dev)
    Fn.quantize_compress(rows, x, bank, table(ids, dev, n_bank), bits_, seed, rnd, levels, scales)
    assert torch.equal(bits(x), bits(x0)), "x moved"
    return rows, bank, levels.cpu().numpy().astype(np.int64), scales.cpu().numpy()


def assert_quant(tag, y0, x0, bank0, ids, bits_, out, seed=SEED, rnd=ROUND):
    """One call's outputs against the oracle. -> (ambiguous entries, live entries)."""
    rows, bank, levels, scales = out
    G, P = y0.shape
    L = (1 << (bits_ - 1)) - 1
    x = O.f32(x0)
    n_amb = n_live = 0
    got_rows = rows.detach().cpu().numpy()
    for g in range(G):
        e = None if bank0 is None else bank0[ids[g]]
        u = O.corrected(y0[g], x0, e)
        s, a, r, lv, finite, amb = O.quant_row(u, ids[g], bits_, seed, rnd)
        assert np.array_equal(O.ubits(scales[g]), O.ubits(s)), f"{tag}: scales of slot {g}"
        mag = np.abs(levels[g])
        lo = np.floor(a)
        assert bool(((mag == lo) | (mag == np.minimum(L, lo + 1))).all()), f"{tag}: a level is neither floor nor ceil"
        assert bool((mag <= L).all()) and bool((mag[~finite] == 0).all())
        assert np.array_equal(mag[~amb], lv[~amb]), f"{tag}: a level departs from the oracle's draw"
        neg = O.ubits(u) >> np.uint32(31) == 1
        assert bool((np.sign(levels[g])[mag > 0] == np.where(neg, -1, 1)[mag > 0]).all()), f"{tag}: sign"
        n_amb += int(amb.sum())
        n_live += int((finite & (np.repeat(s, 256)[:P] > 0)).sum())
        # the decode of the kernel's own levels and scales: q = sign * s * (l / L), each rounded
        sj = np.repeat(s, 256)[:P]
        with np.errstate(all="ignore"):
            q = (sj * (mag.astype(np.float32) / np.float32(L))).astype(np.float32)
            q = np.where(levels[g] < 0, -q, q).astype(np.float32)
            exact = levels[g].astype(np.float64) * sj.astype(np.float64) / L
            assert bool((np.abs(q.astype(np.float64) - exact) <= 2.0 ** -22 * np.abs(q.astype(np.float64))).all())
            assert bool((q[mag == 0] == 0).all()) and np.array_equal(np.abs(q[mag == L]), sj[mag == L])
            want_row = np.where(finite, (x + q).astype(np.float32), (x + u).astype(np.float32))
            fin = finite
            err = np.abs(got_rows[g][fin].astype(np.float64) - want_row[fin].astype(np.float64))
            assert bool((err <= O.ulp(want_row[fin])).all()), f"{tag}: row of slot {g}, worst {err.max()}"
            assert bool(np.array_equal(np.isfinite(got_rows[g]), finite & np.isfinite(want_row)))
            # l = 0 and l = L are exact
            top = fin & ((mag == 0) | (mag == L))
            assert np.array_equal(O.ubits(got_rows[g][top]), O.ubits(want_row[top])), f"{tag}: exact levels, row"
            if bank is not None:
                gb = bank.detach().cpu().numpy()[ids[g]]
                want_b = np.where(finite, (u - q).astype(np.float32), O.f32(bank0[ids[g]]))
                errb = np.abs(gb.astype(np.float64) - want_b.astype(np.float64))
                assert bool((errb <= O.ulp(want_b)).all()), f"{tag}: bank of slot {g}, worst {errb.max()}"
                assert np.array_equal(O.ubits(gb[top | ~finite]), O.ubits(want_b[top | ~finite])), f"{tag}: exact, bank"
    if bank is not None:
        rest = [i for i in range(bank0.shape[0]) if i not in ids]
        assert torch.equal(bits(bank[rest]), bits(bank0[rest])), f"{tag}: a bank row outside the table moved"
    return n_amb, n_live


AMBIGUOUS = {"n": 0, "of": 0}  # over every quantization case of the session that ran


def check_quantize(G, P, bits_, dev):
    ids = TABLE[:G]
    # inputs whose oracle a* and draws put no call over the cap on ambiguous entries (checked below
    # from the oracle alone; the window covers ~1.2e-4 of the draws at 8 bits)
    y0, x0, bank0 = base_case(G, P, 41 * G + P + bits_)
    outs = {}
    for with_bank in (True, False):
        b0 = bank0 if with_bank else None
        for layout in LAYOUTS if with_bank else ("p4",):
            out = run_quant(y0, x0, b0, ids, bits_, dev, layout)
            tag = f"quant bits={bits_} G={G} P={P} bank={with_bank} {layout}"
            n_amb, n_live = assert_quant(tag, y0, x0, b0, ids, bits_, out)
            AMBIGUOUS["n"] += n_amb
            AMBIGUOUS["of"] += n_live
            # at most 0.1 % of a call's entries may sit in the window
            assert 1000 * n_amb <= G * P, f"{tag}: {n_amb} ambiguous entries of {G * P}"
            outs[with_bank, layout] = out
    ref = outs[True, "p4"]
    for layout in LAYOUTS:  # 16-B and scalar paths: the same bits everywhere
        rows, bank, levels, scales = outs[True, layout]
        assert torch.equal(bits(rows), bits(ref[0])) and torch.equal(bits(bank), bits(ref[1])), layout
        assert np.array_equal(levels, ref[2]) and np.array_equal(O.ubits(scales), O.ubits(ref[3])), layout
    # a client's levels do not depend on its slot or on G: client ids[-1] alone in slot 0
    g = G - 1
    solo = run_quant(y0[g:g + 1], x0, bank0, ids[g:], bits_, dev, "p1")
    assert np.array_equal(solo[2][0], ref[2][g])
    assert torch.equal(bits(solo[0][0]), bits(ref[0][g]))
    if P >= 256:  # another round, another client id (same error row contents): other draws
        other = run_quant(y0[g:g + 1], x0, bank0, ids[g:], bits_, dev, "p4", rnd=ROUND + 1)
        assert not np.array_equal(other[2][0], ref[2][g])
        swapped = bank0.clone()
        swapped[1] = bank0[ids[g]]
        moved = run_quant(y0[g:g + 1], x0, swapped, [1], bits_, dev, "p4")
        assert np.array_equal(O.ubits(moved[3]), O.ubits(solo[3])) and not np.array_equal(moved[2][0], ref[2][g])


def check_quantize_buckets(dev):
    """P = 700: bucket 0 is all zero, bucket 1 holds only NaN / Inf, bucket 2 (a partial one) is
    ordinary with NaN / Inf sprinkled in; bits = 4."""
    g_ = torch.Generator().manual_seed(8)
    P = 700
    x0 = torch.randn(P, generator=g_)
    y0 = (x0 + 0.1 * torch.randn(P, generator=g_))[None, :].clone()
    bank0 = 0.01 * torch.randn(2, P, generator=g_)
    y0[0, :256] = x0[:256]
    bank0[1, :256] = 0.0
    y0[0, 256:512] = torch.tensor([float("nan"), float("inf"), float("-inf"), float("inf")]).repeat(64)
    y0[0, 600], y0[0, 699] = float("nan"), float("-inf")
    outs = []
    for layout in LAYOUTS:
        out = run_quant(y0, x0, bank0, [1], 4, dev, layout, n_bank=2)
        assert_quant(f"quant buckets {layout}", y0, x0, bank0, [1], 4, out)
        rows, bank, levels, scales = out
        assert scales[0, 0] == 0 and scales[0, 1] == 0 and scales[0, 2] > 0
        assert not levels[0, :512].any() and levels[0, 512:].any() and levels[0, 600] == 0
        assert torch.equal(bits(rows[0, :256]), bits(x0[:256]))  # a zero bucket: exactly x
        assert torch.equal(bits(bank[1, 256:512]), bits(bank0[1, 256:512]))  # passed through: bank bits stay
        assert not bool(torch.isfinite(rows[0, 256:512]).any())
        outs.append(out)
    for o in outs[1:]:
        assert same_bits(o[0], outs[0][0].cpu().numpy()) and same_bits(o[1], outs[0][1].cpu().numpy())
        assert np.array_equal(o[2], outs[0][2])


def check_deterministic(dev):
    y0, x0, bank0 = base_case(3, 1027, 41)
    a, b = [], []
    for outs in (a, b):
        rows, bank, nnz = run_topk(y0, x0, bank0, TABLE, 50, dev, "quad")
        outs += [rows, bank, nnz.float()]
        rows, bank, levels, scales = run_quant(y0, x0, bank0, TABLE, 4, dev, "quad")
        outs += [rows, bank, torch.from_numpy(levels).float(), torch.from_numpy(scales)]
    for s, t in zip(a, b):
        assert torch.equal(bits(s), bits(t))


def check_rejects(dev):
    """The op validates its scalars and a host slot table."""
    rows, x, bank = torch.zeros(2, 8, device=dev), torch.zeros(8, device=dev), torch.zeros(3, 8, device=dev)
    nnz = torch.zeros(2, dtype=torch.int32, device=dev)
    t = table([0, 2], dev, 3)
    with pytest.raises(ValueError):
        Fn.topk_compress(rows, x, bank, t, 0, nnz)
    for b in (1, 9):
        with pytest.raises(ValueError):
            Fn.quantize_compress(rows, x, bank, t, b, 0, 0)
    for ids in ([0, 3], [1, 1]):
        with pytest.raises(ValueError):
            Fn.check_slot_clients(ids, 3)
    with pytest.raises(ValueError):
        TopK(0.0)
    with pytest.raises(ValueError):
        Quantize(1)


@pytest.mark.parametrize("P", TOPK_P)
@pytest.mark.parametrize("G", TOPK_G)
def test_topk_is_bit_exact(cuda, G, P):
    check_topk(G, P, cuda)


def test_topk_without_bank_drops_the_rest(cuda):
    check_topk_without_bank_drops(cuda)


def test_topk_second_grid_stride_iteration(cuda):
    check_topk_second_pass(cuda)


@pytest.mark.parametrize("bits_", QUANT_BITS)
@pytest.mark.parametrize("P", QUANT_P)
@pytest.mark.parametrize("G", TOPK_G)
def test_quantize(cuda, G, P, bits_):
    check_quantize(G, P, bits_, cuda)


def test_quantize_zero_and_nonfinite_buckets(cuda):
    check_quantize_buckets(cuda)


def test_two_calls_are_bit_equal(cuda):
    check_deterministic(cuda)


def test_op_rejects_bad_arguments(cuda):
    check_rejects(cuda)


def test_kernel_rejects_bad_arguments(cuda):
    """G < 1, null pointers, ld < P, k < 1, bits outside 2..8 and a short workspace come back as
    hipErrorInvalidValue (1); nothing is launched."""
    from ddl25spring_amd.ops import _lib
    lib = _lib.kernels()
    t = torch.zeros(3, 8, device=cuda)
    i = torch.zeros(2, dtype=torch.int32, device=cuda)
    cap = lib.ddl_topk_workspace(1)
    w = torch.zeros(cap, dtype=torch.int32, device=cuda)
    p, ip, wp, s = t.data_ptr(), i.data_ptr(), w.data_ptr(), _lib.stream()
    good = [p, 8, p, p, 8, ip, 1, 8, 2, ip, wp, cap, s]
    for pos, bad in ((6, 0), (0, None), (2, None), (5, None), (9, None), (10, None), (4, 7), (8, 0), (11, cap - 1),
                     (7, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.ddl_topk_compress(*args) == 1, pos
    args = list(good)
    args[6], args[1] = 2, 7  # two rows closer than P
    assert lib.ddl_topk_compress(*args) == 1
    good = [p, 8, p, p, 8, ip, 1, 8, 4, 5, 0, None, None, s]
    for pos, bad in ((6, 0), (0, None), (2, None), (5, None), (4, 7), (8, 1), (8, 9), (7, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.ddl_quantize_compress(*args) == 1, pos
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(w.any())


# ------------------------------------------------------------------------------------- the engine
def make_fed(dev, model=mnist_mlp, arr=None, parts=None, cls=FedAvg, **kw):
    if arr is None:
        arr = synthetic_images("mnist", 600, seed=0)
        parts = split(4, True, 3, labels=arr.labels)
    base = dict(lr=0.1, batch_size=50, client_fraction=1.0, seed=3, eval_every=0)
    base.update(kw)
    return cls(model, DeviceImageDataset(arr, dev), parts, ctx=DistContext(device=torch.device(dev)), **base)


CODECS = {"topk": dict(compressor="topk", compressor_kwargs=dict(ratio=0.1)),
          "quant": dict(compressor="quant", compressor_kwargs=dict(bits=4, seed=5))}


@pytest.mark.parametrize("codec", list(CODECS))
def test_compressed_device_engine_tracks_cpu_engine(cuda, codec):
    """The criterion of test_scaffold_device_engine_tracks_cpu_engine, over two rounds so the second
    one adds a non-zero error row back."""
    arr = synthetic_images("mnist", 600, seed=0)
    parts = split(4, True, 1, labels=arr.labels)
    runs = []
    for dev in (torch.device("cpu"), cuda):
        fa = make_fed(dev, mnist_mlp, arr, parts, lr=0.05, client_fraction=0.5, seed=1, **CODECS[codec])
        fa.round()
        fa.round()
        runs.append((fa.w_global.float().cpu(), fa.compressor.bank.float().cpu(), fa.uplink_bytes))
    (cpu, bcpu, up_c), (gpu, bgpu, up_g) = runs
    rel = ((cpu - gpu).norm() / cpu.norm()).item()
    assert rel < 2e-2, rel
    assert bool(bcpu.any()) and bool(bgpu.any()) and len(up_g) == 2
    if codec == "quant":
        assert up_c == up_g


LEARN = dict(lr=0.05, batch_size=50, client_fraction=0.5, seed=10)


def learn_run(dev, rounds=8, **over):
    arr = synthetic_images("mnist", 3000, seed=0)
    tarr = synthetic_images("mnist", 1000, seed=1)
    parts = split(10, True, 10, labels=arr.labels)
    fa = FedAvg(mnist_cnn, DeviceImageDataset(arr, dev), parts, ctx=DistContext(device=torch.device(dev)),
                test_data=DeviceImageDataset(tarr, dev), **{**LEARN, **over})
    return fa.run(rounds).test_accuracy, fa.uplink_bytes, fa.w_global.numel()


@pytest.mark.parametrize("codec", list(CODECS))
def test_compressed_fedavg_learns_on_device(cuda, codec):
    """10 IID clients, C = 0.5, MnistCnn, 8 rounds: top-k 0.1 with error feedback and 4-bit
    quantization each end at >= 80 % (the fp32 CPU engine reaches 100 % for both, as dense does)."""
    acc, up, P = learn_run(cuda, **CODECS[codec])
    print(f"{codec}: accuracy per round {acc}; uplink bytes per round {up}; dense would be {5 * 4 * P}")
    assert acc[-1] >= 80.0, acc
    assert len(up) == 8 and all(0 < b < 5 * 4 * P for b in up)
