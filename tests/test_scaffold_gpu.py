"""SCAFFOLD's local step and round-end update (csrc/kernels/scaffold.hip) against the float64 oracle
and derived error bound of tests/scaffold_oracle.py, and through the FL engine.

The ``check_*`` functions take the device, so tests/test_scaffold_cpu.py runs the same cases on the
torch twins; here they run on the kernels. Multi-step cases compare step by step: the state the code
under test produced in step s is the oracle's input for step s + 1, so the bound stays the
single-step one."""
import ctypes

import numpy as np
import pytest
import torch

import scaffold_oracle as O
from test_fedopt_gpu import BIG_N, PROX_CFGS, bits, emulation_within, place
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.algorithms import Scaffold
from ddl25spring_amd.models import mnist_cnn, mnist_mlp
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.runtime.dist import DistContext

pytestmark = pytest.mark.gpu

LR = 0.05
STEP_G, STEP_P = (1, 3), (5, 16, 48, 1040)
FIN_G, FIN_P = (1, 2, 7), (1, 5, 1024, 1027)
TABLE = [4, 0, 2]  # slot -> client of the local-step cases: not the identity, 5 bank rows


def padded(t, dev, pad):
    """The rows of t as a strided view on ``dev``: row stride = columns + pad, 16-B aligned base."""
    n, P = t.shape
    buf = torch.full((n, P + pad), -12345.0, dtype=t.dtype, device=dev)
    buf[:, :P] = t.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[:, :P]


def table(ids, dev, n_clients=5):
    return torch.tensor(Fn.check_slot_clients(ids, n_clients), dtype=torch.int32, device=dev)


def shadow_is_bf16_of(shadow, p):
    return torch.equal(shadow.cpu().view(torch.int16), p.cpu().to(torch.bfloat16).view(torch.int16))


# --------------------------------------------------------------------------- 1: sgd_scaffold_step
def step_case(G, P, seed):
    g_ = torch.Generator().manual_seed(seed)
    c = torch.randn(P, generator=g_)
    # every client's row at its own scale and offset: a wrong row, or bank[flat index], shows
    bank = torch.randn(5, P, generator=g_) * torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0]]) \
        + torch.arange(5.0)[:, None]
    p = torch.randn(G, P, generator=g_)
    return g_, c, bank, p


def run_scaffold_steps(G, P, cfg_name, with_shadow, dev, pad):
    cfg = PROX_CFGS[cfg_name]
    g_, c0, bank0, p0 = step_case(G, P, 100 * G + P + len(cfg_name))
    c, bank, p = place(c0, dev), padded(bank0, dev, pad), place(p0, dev)
    slots = table(TABLE[:G], dev)
    mom = place(torch.zeros(G, P), dev) if cfg.get("momentum") else None
    shadow = torch.zeros(G, P, dtype=torch.bfloat16, device=dev) if with_shadow else None
    worst = 0.0
    for step in range(4):
        grad = place(torch.randn(G, P, generator=g_), dev)
        first = step == 0
        want_p, want_m = O.scaffold_step(p, grad, mom, c, bank, slots, LR, first_step=first, **cfg)
        emulation_within(f"scaffold {cfg_name}", dev, lambda: O.emulate_scaffold_step(
            p.clone(), grad, None if mom is None else mom.clone(), c, bank, slots, LR, first_step=first,
            **cfg), (want_p, want_m))
        Fn.sgd_scaffold_step(p, grad, mom, shadow, c, bank, slots, LR, first_step=first, **cfg)
        rp, rm = O.ratio(p, want_p), 0.0 if mom is None else O.ratio(mom, want_m)
        worst = max(worst, rp, rm)
        assert rp <= 1.0, f"scaffold {cfg_name} G={G} P={P} pad={pad} step {step}: p err / bound = {rp}"
        assert rm <= 1.0, f"scaffold {cfg_name} G={G} P={P} pad={pad} step {step}: mom err / bound = {rm}"
        if shadow is not None:  # the shadow is f2bf of the new p, exactly
            assert shadow_is_bf16_of(shadow, p)
    assert torch.equal(bits(bank), bits(bank0)) and torch.equal(bits(c), bits(c0))  # read only
    return (p, mom, None if shadow is None else shadow.float()), worst


def check_sgd_scaffold(G, P, cfg_name, with_shadow, dev):
    """The bank is a strided view: row stride P + 4 takes the 16-B path when P % 4 == 0, P + 1 the
    scalar path; the same bits."""
    a, ra = run_scaffold_steps(G, P, cfg_name, with_shadow, dev, 4)
    b, rb = run_scaffold_steps(G, P, cfg_name, with_shadow, dev, 1)
    print(f"sgd_scaffold {cfg_name} G={G} P={P} shadow={with_shadow}: worst err / bound = {max(ra, rb):.3f}")
    for s, t in zip(a, b):
        assert (s is None and t is None) or torch.equal(bits(s), bits(t))


def check_scaffold_identity(P, cfg_name, dev):
    """bank[slot] == c bit for bit: the correction is +0 and the step is sgd_prox_step's with mu = 0."""
    cfg = PROX_CFGS[cfg_name]
    g_, c0, bank0, p0 = step_case(3, P, 7 + P)
    for cl in TABLE:
        bank0[cl] = c0
    c, bank, slots = place(c0, dev), padded(bank0, dev, 4), table(TABLE, dev)
    anchor = place(torch.randn(P, generator=g_), dev)
    state = []
    for _ in range(2):
        mom = place(torch.zeros(3, P), dev) if cfg.get("momentum") else None
        state.append([place(p0, dev), mom, torch.zeros(3, P, dtype=torch.bfloat16, device=dev)])
    for step in range(2):
        grad = place(torch.randn(3, P, generator=g_), dev)
        (p1, m1, s1), (p2, m2, s2) = state
        Fn.sgd_scaffold_step(p1, grad, m1, s1, c, bank, slots, LR, first_step=step == 0, **cfg)
        Fn.sgd_prox_step(p2, grad, m2, s2, anchor, LR, 0.0, first_step=step == 0, **cfg)
        assert torch.equal(bits(p1), bits(p2)) and torch.equal(bits(s1.float()), bits(s2.float()))
        assert m1 is None or torch.equal(bits(m1), bits(m2))
    assert not torch.equal(state[0][0].cpu(), p0)


def check_scaffold_row_slice(P, dev):
    """Rows 1..2 of 3 are stepped with the table sliced alike: row 0, its momentum and its shadow stay
    bit for bit, and rows 1, 2 read the bank rows of THEIR clients."""
    g_, c0, bank0, _ = step_case(3, P, 9 + P)
    p0 = torch.randn(3, P, generator=g_) * torch.tensor([[1.0], [2.0], [3.0]])
    c, bank, slots = place(c0, dev), padded(bank0, dev, 4), table(TABLE, dev)
    p, grad = place(p0, dev), place(torch.randn(3, P, generator=g_), dev)
    mom = place(0.1 * torch.randn(3, P, generator=g_), dev)
    m0 = mom.cpu().clone()
    shadow = torch.full((3, P), 7.0, dtype=torch.bfloat16, device=dev)
    cfg = dict(momentum=0.9)
    want_p, want_m = O.scaffold_step(p[1:3], grad[1:3], mom[1:3], c, bank, slots[1:3], LR, **cfg)
    Fn.sgd_scaffold_step(p[1:3], grad[1:3], mom[1:3], shadow[1:3], c, bank, slots[1:3], LR, **cfg)
    assert torch.equal(bits(p[0]), bits(p0[0])) and torch.equal(bits(mom[0]), bits(m0[0]))
    assert bool((shadow[0].float() == 7.0).all())
    assert O.ratio(p[1:3], want_p) <= 1.0 and O.ratio(mom[1:3], want_m) <= 1.0
    assert shadow_is_bf16_of(shadow[1:3], p[1:3])
    # with zero gradient and momentum off, one step moves every element by -lr * (c[col] -
    # bank[client][col]): |p| < 16, so the rounding of p1 is at most 2^-21 / 2 and the product's is
    # far below; a wrong bank row is off by lr * O(1)
    q = place(p0, dev)
    Fn.sgd_scaffold_step(q[1:3], torch.zeros_like(q[1:3]), None, None, c, bank, slots[1:3], LR)
    assert float(p0.abs().max()) < 16
    move = (p0[1:3] - q[1:3].cpu()).double() - float(np.float32(LR)) * (c0[None, :] - bank0[TABLE[1:3]]).double()
    assert bool((move.abs() < 2e-6).all()), move.abs().max()
    assert torch.equal(bits(q[0]), bits(p0[0]))


# ----------------------------------------------------------------------------- 2: scaffold_finish
def finish_case(G, P, seed, tail_scale=None):
    """N = G + 2 clients; the slots train clients G, G - 1, .., 1 (rows 0 and G + 1 stay out)."""
    g_ = torch.Generator().manual_seed(seed)
    N = G + 2
    x = torch.randn(P, generator=g_)
    drift = 0.02 * torch.randn(G, 1, generator=g_).exp() * torch.randn(G, P, generator=g_)
    if tail_scale is not None:
        drift[:, P - 5:] *= tail_scale
    y = x + drift
    c = 0.1 * torch.randn(P, generator=g_)
    bank = 0.1 * torch.randn(N, P, generator=g_) * torch.arange(1.0, N + 1)[:, None]
    steps = torch.randint(1, 9, (G,), generator=g_).double()
    inv_klr = (1.0 / (steps * LR)).float()
    return y, x, c, bank, list(range(G, 0, -1)), inv_klr, 1.0 / N


def put(t, dev, misaligned):
    """misaligned: contiguous, one float past a 16-B boundary (the scalar path); else 2-D tensors as
    views of row stride = columns rounded up to 4, + 4 (16-B body and scalar tail for any P)."""
    if misaligned or t.dim() == 1:
        return place(t, dev, misaligned)
    return padded(t, dev, (-t.shape[1]) % 4 + 4)


def run_finish(case, dev, misaligned, apply_c, tag, check=True):
    y0, x0, c0, bank0, ids, k0, inv_n = case
    y, x, c, bank = (put(t, dev, misaligned) for t in (y0, x0, c0, bank0))
    slots, k = table(ids, dev, bank0.shape[0]), k0.to(dev)
    dc = put(torch.full_like(x0, 9.0), dev, misaligned)
    Fn.scaffold_finish(y, x, c, bank, slots, k, inv_n, dc, apply_c=apply_c)
    worst = 0.0
    if check:
        want_b, want_dc, want_c, ok = O.finish(y0, x0, c0, bank0, ids, k0, inv_n)
        for name, got, want in (("bank", bank[ids], want_b), ("dc", dc, want_dc)) + \
                ((("c", c, want_c),) if apply_c else ()):
            r = O.ratio(got, want)
            worst = max(worst, r)
            assert r <= 1.0, f"{tag} mis={misaligned}: {name} err / bound = {r}"
        if torch.device(dev).type == "cpu":
            for name, e, want in zip(("bank", "dc", "c"), O.emulate_finish(y0, x0, c0, bank0, ids, k0, inv_n),
                                     (want_b, want_dc, want_c)):
                r = O.ratio(e, want)
                assert r <= 1.0, f"{tag}: the fp32 emulation's {name} misses the bound, err / bound = {r}"
    rest = [i for i in range(bank0.shape[0]) if i not in ids]
    assert torch.equal(bits(bank[rest]), bits(bank0[rest])), f"{tag}: a bank row outside the table moved"
    if not apply_c:
        assert torch.equal(bits(c), bits(c0))
    assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(y), bits(y0))
    return (bank.clone(), dc, c), worst


def check_finish(G, P, dev):
    case = finish_case(G, P, 31 * G + P)
    outs, worst = {}, 0.0
    for mis in (False, True):
        for apply_c in (False, True):
            outs[mis, apply_c], r = run_finish(case, dev, mis, apply_c, f"finish G={G} P={P}")
            worst = max(worst, r)
    print(f"scaffold_finish G={G} P={P}: worst err / bound = {worst:.3f}")
    ref_bank, ref_dc, ref_c = outs[False, True]
    for key, (bank, dc, c) in outs.items():  # aligned and misaligned bases: the same bits
        assert torch.equal(bits(bank), bits(ref_bank)) and torch.equal(bits(dc), bits(ref_dc)), key
    for mis in (False, True):  # apply_c is c + dc, bit for bit
        _, dc, c_off = outs[mis, False]
        assert torch.equal(bits(outs[mis, True][2]), bits(c_off + dc))
    assert bool(ref_dc.any()) and not torch.equal(ref_c.cpu(), case[2])


def check_finish_exact(dev):
    """Small integers, power-of-two 1 / (K lr) and 1 / N: every operation is exact in fp32, so bank,
    dc and c equal the float64 values."""
    G, P, N = 3, 9, 4
    g_ = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 9, (P,), generator=g_).float()
    y = x - torch.randint(-4, 5, (G, P), generator=g_).float()
    c = torch.randint(-3, 4, (P,), generator=g_).float()
    bank = torch.randint(-5, 6, (N, P), generator=g_).float()
    k = torch.tensor([0.5, 2.0, 4.0])
    ids = [3, 1, 0]
    delta = (x[None, :] - y).double() * k[:, None].double() - c[None, :].double()
    want_bank = bank.double().clone()
    want_bank[ids] += delta
    want_dc = delta.sum(0) * 0.25
    assert bool(delta.any())
    for mis in (False, True):
        for apply_c in (False, True):
            (b, dc, c1), _ = run_finish((y, x, c, bank, ids, k, 0.25), dev, mis, apply_c, "exact", check=False)
            assert np.array_equal(b.cpu().double().numpy(), want_bank.numpy())
            assert np.array_equal(dc.cpu().double().numpy(), want_dc.numpy())
            assert np.array_equal(c1.cpu().double().numpy(), (c.double() + (want_dc if apply_c else 0)).numpy())


BAD_AT = {0: float("nan"), 5: float("inf"), 1023: float("-inf"), 1024: float("nan"), 1026: float("inf")}


def check_finish_nonfinite(dev):
    """NaN / +Inf / -Inf in slot 1's trained row (in the 16-B body and in the scalar tail): those
    entries of its bank row are bit-unchanged, and everything else, the other slots' contribution
    to dc at those columns included, is within bound."""
    G, P = 3, 1027
    y, x, c, bank, ids, k, inv_n = finish_case(G, P, 5)
    for i, bad in BAD_AT.items():
        y[1, i] = bad
    case = (y, x, c, bank, ids, k, inv_n)
    ok = O.finish(*case)[3]
    keep = np.ones((G, P), dtype=bool)
    keep[1, list(BAD_AT)] = False
    assert np.array_equal(ok, keep)
    idx = torch.tensor(list(BAD_AT))
    outs = []
    for mis in (False, True):
        (b, dc, c1), r = run_finish(case, dev, mis, True, "non-finite")
        print(f"scaffold_finish non-finite mis={mis}: worst err / bound = {r:.3f}")
        assert torch.equal(bits(b[ids[1]])[idx], bits(bank[ids[1]])[idx]), "a poisoned bank entry moved"
        for t in (b, dc, c1):
            assert bool(torch.isfinite(t).all())
        assert bool((dc.cpu()[idx] != 0).all())  # slots 0 and 2 still count there
        outs.append((b, dc, c1))
    for s, t in zip(*outs):
        assert torch.equal(bits(s), bits(t))


def check_finish_second_pass(dev):
    """P just past 8192 blocks x 256 threads x 4, the grid cap: every thread runs the grid-stride loop
    a second time, the last one on a partial quad. The drift of the last 5 columns is scaled by 30,
    so a dropped tail cannot hide in the tolerance."""
    case = finish_case(2, BIG_N, 3, tail_scale=30.0)
    (b, dc, c1), r = run_finish(case, dev, False, True, "finish big")
    print(f"scaffold_finish second pass: worst err / bound = {r:.3f}")
    assert bool((dc.cpu()[-5:].abs() > 10 * dc.cpu()[:-5].abs().mean()).any())


def check_deterministic(dev):
    case = finish_case(7, 1027, 11)
    outs = []
    for _ in range(2):
        res = list(run_finish(case, dev, False, True, "det", check=False)[0])
        g_, c0, bank0, p0 = step_case(3, 1024, 12)
        p, mom = place(p0, dev), place(0.1 * p0, dev)
        sh = torch.zeros(3, 1024, dtype=torch.bfloat16, device=dev)
        Fn.sgd_scaffold_step(p, place(torch.randn(3, 1024, generator=g_), dev), mom, sh, place(c0, dev),
                             padded(bank0, dev, 4), table(TABLE, dev), LR, momentum=0.9, nesterov=True)
        outs.append(res + [p, mom, sh.float()])
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))


def check_rejects(dev):
    """The slot table is validated on the host where it is built."""
    for ids in ([0, 5], [-1, 2], [1, 1]):
        with pytest.raises(ValueError):
            Fn.check_slot_clients(ids, 5)
    assert Fn.check_slot_clients(np.array([4, 0, 2]), 5) == [4, 0, 2]


@pytest.mark.parametrize("with_shadow", [False, True])
@pytest.mark.parametrize("cfg", list(PROX_CFGS))
@pytest.mark.parametrize("P", STEP_P)
@pytest.mark.parametrize("G", STEP_G)
def test_sgd_scaffold_step(cuda, G, P, cfg, with_shadow):
    check_sgd_scaffold(G, P, cfg, with_shadow, cuda)


@pytest.mark.parametrize("cfg", list(PROX_CFGS))
@pytest.mark.parametrize("P", [5, 48])
def test_sgd_scaffold_equals_prox_mu0_when_bank_is_c(cuda, P, cfg):
    check_scaffold_identity(P, cfg, cuda)


@pytest.mark.parametrize("P", [5, 48])
def test_sgd_scaffold_row_slice_and_client_rows(cuda, P):
    check_scaffold_row_slice(P, cuda)


@pytest.mark.parametrize("P", FIN_P)
@pytest.mark.parametrize("G", FIN_G)
def test_scaffold_finish(cuda, G, P):
    check_finish(G, P, cuda)


def test_scaffold_finish_exact_on_small_integers(cuda):
    check_finish_exact(cuda)


def test_scaffold_finish_nonfinite_leaves_bank_entry(cuda):
    check_finish_nonfinite(cuda)


def test_scaffold_finish_second_grid_stride_iteration(cuda):
    check_finish_second_pass(cuda)


def test_two_calls_are_bit_equal(cuda):
    check_deterministic(cuda)


def test_kernel_rejects_bad_arguments(cuda):
    """G < 1, null pointers and ld < P come back as hipErrorInvalidValue (1), nothing is launched."""
    from ddl25spring_amd.ops import _lib
    lib = _lib.kernels()
    t = torch.zeros(8, device=cuda)
    i = torch.zeros(2, dtype=torch.int32, device=cuda)
    p, ip, s = t.data_ptr(), i.data_ptr(), _lib.stream()
    good = [p, 4, p, p, p, 4, ip, p, 1, 0.5, p, 4, 0, s]
    for pos, bad in ((8, 0), (0, None), (2, None), (3, None), (4, None), (6, None), (7, None), (10, None), (5, 3)):
        args = list(good)
        args[pos] = bad
        assert lib.ddl_scaffold_finish(*args) == 1, pos
    a = _lib.SGDCorrectedArgs()
    a.p, a.g, a.ref, a.bank, a.slot_client = p, p, p, p, ip
    a.rows, a.P, a.ld, a.lr, a.correction = 1, 4, 3, 0.1, _lib.SGD_CONTROL
    assert lib.ddl_sgd_corrected(ctypes.byref(a), s) == 1
    a.ld, a.slot_client = 4, None
    assert lib.ddl_sgd_corrected(ctypes.byref(a), s) == 1


# ------------------------------------------------------------------------------------- the engine
def fl_setup(n=600, clients=4, seed=3):
    arr = synthetic_images("mnist", n, seed=0)
    return arr, split(clients, True, seed, labels=arr.labels)


def make_sc(dev, model=mnist_mlp, arr=None, parts=None, cls=Scaffold, **kw):
    if arr is None:
        arr, parts = fl_setup()
    base = dict(lr=0.1, batch_size=50, client_fraction=1.0, seed=3, eval_every=0)
    base.update(kw)
    return cls(model, DeviceImageDataset(arr, dev), parts, ctx=DistContext(device=torch.device(dev)), **base)


def test_scaffold_graph_replay_equals_eager(cuda):
    """The captured SCAFFOLD steps (gradient-buffer path; c, the bank and the slot table read through
    their pointers) equal eager steps; batch 60 ends every client's 200 samples in a short step of
    20, captured in the same graph. Three rounds of 2 clients in 4: the replayed graph reads a
    changed slot table and a non-zero bank. The criterion of test_fedprox_graph_replay_equals_eager."""
    arr = synthetic_images("mnist", 800, seed=0)
    parts = split(4, True, 3, labels=arr.labels)
    ws, tables = [], []
    for graph in (True, False):
        fa = make_sc(cuda, mnist_cnn, arr, parts, lr=0.05, batch_size=60, use_graph=graph, client_fraction=0.5)
        w0 = fa.w_global.clone()
        seen = []
        for _ in range(3):
            fa.round()
            seen.append(fa.slot_client.cpu().tolist())
        assert fa.trainer.direct is False and fa.trainer.use_graph is graph
        assert bool(fa.c_bank.any()) and bool(fa.c_global.any())
        ws.append((fa.w_global.clone(), fa.c_global.clone(), fa.c_bank.clone()))
        tables.append(seen)
    assert tables[0] == tables[1] and len({tuple(t) for t in tables[0]}) > 1  # the table did change
    step = (ws[1][0] - w0).norm()
    assert step > 0
    assert ((ws[0][0] - ws[1][0]).norm() / step).item() < 1e-2
    for a, b in zip(ws[0][1:], ws[1][1:]):  # the control variates, against their own size
        assert ((a - b).norm() / b.norm()).item() < 1e-2


def test_scaffold_device_engine_tracks_cpu_engine(cuda):
    """As test_fedprox_device_engine_tracks_cpu_engine, over two rounds so the second one trains
    with non-zero control variates."""
    arr = synthetic_images("mnist", 600, seed=0)
    parts = split(4, True, 1, labels=arr.labels)
    runs = []
    for dev in (torch.device("cpu"), cuda):
        fa = make_sc(dev, mnist_mlp, arr, parts, lr=0.05, client_fraction=0.5, seed=1)
        fa.round()
        fa.round()
        runs.append((fa.w_global.float().cpu(), fa.c_global.float().cpu()))
    (cpu, ccpu), (gpu, cgpu) = runs
    rel = ((cpu - gpu).norm() / cpu.norm()).item()
    assert rel < 2e-2, rel
    assert bool(ccpu.any()) and bool(cgpu.any())


# the client lr chosen on the CPU fp32 engine (profiles/scaffold_r10.txt records the sweep and the
# CPU and device accuracies)
LEARN = dict(lr=0.05, batch_size=50, client_fraction=0.5, seed=10)


def learn_run(dev, iid=True, rounds=3, cls=Scaffold, **over):
    arr = synthetic_images("mnist", 3000, seed=0)
    tarr = synthetic_images("mnist", 1000, seed=1)
    parts = split(10, iid, 10, labels=arr.labels)
    fa = cls(mnist_cnn, DeviceImageDataset(arr, dev), parts, ctx=DistContext(device=torch.device(dev)),
             test_data=DeviceImageDataset(tarr, dev), **{**LEARN, **over})
    return fa.run(rounds).test_accuracy


def test_scaffold_learns_on_device(cuda):
    """10 clients, C = 0.5, MnistCnn, IID split, 3 rounds of SCAFFOLD clear the bar of
    test_fedavg_mnist_cnn_learns_on_device: final accuracy > 40 % and not below round 1. The
    non-IID comparison carries no bar: benchmarks/bench_noniid.py reports it."""
    acc = learn_run(cuda)
    print("SCAFFOLD accuracy per round:", acc)
    assert acc[-1] > 40.0 and acc[-1] >= acc[0], acc
