"""SCAFFOLD without a GPU: the torch twins against the float64 oracle (tests/scaffold_oracle.py) on
the cases of tests/test_scaffold_gpu.py (each of which also holds the oracle file's np.float32
emulation to the same bound), and the engine: a hand-driven round, the invariants of the control
variates, two gloo ranks, checkpoints, validation and the CLI."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import scaffold_oracle as O
import test_scaffold_gpu as G
import ddl25spring_amd.ops.reference as R
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import plan_epoch, split
from ddl25spring_amd.fl.algorithms import FedAvg, Scaffold
from ddl25spring_amd.fl.local import LocalTrainer
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
def test_oracle_on_hand_computed_cases():
    # p = 1, g = 2, c = 3, c_i = 5 (client 1), lr = .5: d = 2 + (3 - 5) = 0 -> p stays; client 0: d = 2 + 3
    bank = [[0.0], [5.0]]
    p1, m1 = O.scaffold_step([[1.0]], [[2.0]], None, [3.0], bank, [1], 0.5)
    assert p1.v.tolist() == [[1.0]] and m1 is None
    p1, _ = O.scaffold_step([[1.0]], [[2.0]], None, [3.0], bank, [0], 0.5)
    assert p1.v.tolist() == [[-1.5]]
    p1, m1 = O.scaffold_step([[1.0]], [[2.0]], [[4.0]], [3.0], bank, [0], 0.5, momentum=0.5, nesterov=True)
    assert m1.v.tolist() == [[7.0]] and p1.v.tolist() == [[1.0 - 0.5 * (5.0 + 0.5 * 7.0)]]
    # x = 4, y = (2, 5), k = (.5, 2), c = 1, N = 4: delta = (0, -3); bank rows 2, 0 move; dc = -.75
    b1, dc, c1, ok = O.finish([[2.0], [5.0]], [4.0], [1.0], [[10.0], [20.0], [30.0]], [2, 0], [0.5, 2.0], 0.25)
    assert b1.v.tolist() == [[30.0], [7.0]] and dc.v.tolist() == [-0.75] and c1.v.tolist() == [0.25] and ok.all()
    # u |result| per operation, carried on: slot 0: 2 (x - y) -> 2 * .5 + 1 = 2 (* k) -> 2 + 0 (- c) -> 2 + 30;
    # slot 1: 1 -> 1 * 2 + 2 = 4 -> 4 + 3 = 7 -> 7 + 7
    assert b1.e.tolist() == [[32.0 * O.U], [14.0 * O.U]]
    b1, dc, c1, ok = O.finish([[float("nan")], [5.0]], [4.0], [1.0], [[10.0], [20.0], [30.0]], [2, 0], [0.5, 2.0], 0.25)
    assert b1.v.tolist() == [[30.0], [7.0]] and b1.e[0, 0] == 0 and dc.v.tolist() == [-0.75] and not ok[0, 0]
    e = O.emulate_finish([[2.0], [5.0]], [4.0], [1.0], [[10.0], [20.0], [30.0]], [2, 0], [0.5, 2.0], 0.25)
    assert e[0].tolist() == [[30.0], [7.0]] and e[1].tolist() == [-0.75] and e[2].tolist() == [0.25]


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("with_shadow", [False, True])
@pytest.mark.parametrize("cfg", list(G.PROX_CFGS))
@pytest.mark.parametrize("P_", G.STEP_P)
@pytest.mark.parametrize("K", G.STEP_G)
def test_sgd_scaffold_step_cpu(K, P_, cfg, with_shadow):
    G.check_sgd_scaffold(K, P_, cfg, with_shadow, CPU)


@pytest.mark.parametrize("cfg", list(G.PROX_CFGS))
@pytest.mark.parametrize("P_", [5, 48])
def test_sgd_scaffold_equals_prox_mu0_when_bank_is_c_cpu(P_, cfg):
    G.check_scaffold_identity(P_, cfg, CPU)


@pytest.mark.parametrize("P_", [5, 48])
def test_sgd_scaffold_row_slice_and_client_rows_cpu(P_):
    G.check_scaffold_row_slice(P_, CPU)


@pytest.mark.parametrize("P_", G.FIN_P)
@pytest.mark.parametrize("K", G.FIN_G)
def test_scaffold_finish_cpu(K, P_):
    G.check_finish(K, P_, CPU)


def test_scaffold_finish_exact_on_small_integers_cpu():
    G.check_finish_exact(CPU)


def test_scaffold_finish_nonfinite_leaves_bank_entry_cpu():
    G.check_finish_nonfinite(CPU)


def test_scaffold_finish_second_grid_stride_iteration_cpu():
    G.check_finish_second_pass(CPU)


def test_two_calls_are_bit_equal_cpu():
    G.check_deterministic(CPU)


def test_slot_table_is_validated_on_the_host():
    G.check_rejects(CPU)
    c, bank = torch.zeros(4), torch.zeros(3, 4)
    rows = torch.zeros(2, 4)
    for ids in ([0, 3], [1, 1]):  # a host table is checked by the op itself
        t = torch.tensor(ids, dtype=torch.int32)
        with pytest.raises(ValueError):
            Fn.sgd_scaffold_step(rows, rows.clone(), None, None, c, bank, t, 0.1)
        with pytest.raises(ValueError):
            Fn.scaffold_finish(rows, c.clone(), c, bank, t, torch.ones(2), 0.5, torch.zeros(4))


# ------------------------------------------------------------------------------------- the engine
def test_scaffold_matches_a_hand_driven_round(fp32):
    """Two rounds of the engine against a loop driven by hand on the same plans: the engine's seeds ->
    plan_epoch -> net.train_step -> Fn.sgd_scaffold_step on the rows -> Fn.scaffold_finish ->
    Fn.weighted_sum, with c, the bank and the table held outside the class. Batch 60 on 150 samples:
    K_i = 3 with a short last step. Bit for bit."""
    lr, B = 0.1, 60
    fa = G.make_sc(CPU, lr=lr, batch_size=B, use_graph=False, client_fraction=0.5)
    fa.round()
    fa.round()
    assert fa.trainer.direct is False
    c_, bank_, table_ = fa.trainer.opt.control
    assert c_ is fa.c_global and bank_ is fa.c_bank and table_ is fa.slot_client  # the tensors themselves

    fb = G.make_sc(CPU, cls=FedAvg, lr=lr, batch_size=B, use_graph=False, client_fraction=0.5)
    st = fb.net.store
    n_par = fb.w_global.numel()
    c, bank, dc = torch.zeros(n_par), torch.zeros(fb.N, n_par), torch.zeros(n_par)
    for r in range(2):
        chosen = fb._sample()
        mine, _ = fb._assign(chosen)
        K = len(mine)
        assert K == 2
        fb._download(K)
        slots = torch.tensor(mine, dtype=torch.int32)
        seeds = [fb.seed + cl + 1 + r * fb.K for cl in mine]
        plan = plan_epoch([fb.client_indices[cl] for cl in mine], B, [int(s) for s in seeds], True, "native")
        assert plan.shape[0] == 3 and (plan[-1, :, 30:] < 0).all()
        for s in range(plan.shape[0]):
            n = int((plan[s, 0] >= 0).sum())
            x, y = fb.data.batch(torch.from_numpy(np.ascontiguousarray(plan[s, :, :n], dtype=np.int32)))
            with st.select(0, K):
                st.grad[:K].zero_()
                fb.net.train_step(x, y)
            Fn.sgd_scaffold_step(st.data[:K], st.grad[:K], None, None, c, bank, slots, lr)
            st.sync_shadow()
        inv_klr = torch.tensor([1.0 / (3 * lr)] * K, dtype=torch.float32)
        Fn.scaffold_finish(st.data[:K], fb.w_global, c, bank, slots, inv_klr, 1.0 / fb.N, dc, apply_c=True)
        total = float(sum(fb.counts[cl] for cl in mine))
        coeff = torch.tensor([fb.counts[cl] / total for cl in mine], dtype=torch.float32)
        Fn.weighted_sum(st.data[:K], coeff, fb.w_global)
        fb.round_idx += 1
    assert bool(c.any()) and bool(bank.any())
    assert torch.equal(fa.w_global, fb.w_global)
    assert torch.equal(fa.c_global, c) and torch.equal(fa.c_bank, bank)
    assert [fa.local_steps(cl) for cl in range(fa.N)] == [3] * fa.N


def test_first_round_from_zero_control_equals_fedavg(fp32):
    """The correction of round 1 is c - c_i = +0: the same bits as FedAvg on the CPU engine."""
    a, b = G.make_sc(CPU, use_graph=False), G.make_sc(CPU, cls=FedAvg, use_graph=False)
    a.round()
    b.round()
    assert torch.equal(G.bits(a.w_global), G.bits(b.w_global))
    assert bool(a.c_global.any())
    a.round()
    b.round()
    assert not torch.equal(a.w_global, b.w_global)  # from round 2 on the control variates act


def test_control_variate_invariants(fp32):
    """After 3 rounds with C = 0.5: c is the mean of the bank rows (both are sums of the same dc_i,
    c's scaled by 1 / N) within the oracle's arithmetic bound, and a never-sampled client's row is
    still all-zero."""
    arr = synthetic_images("mnist", 600, seed=0)
    parts = split(10, True, 3, labels=arr.labels)
    fa = G.make_sc(CPU, arr=arr, parts=parts, lr=0.05, client_fraction=0.5, seed=3, use_graph=False)
    rng = np.random.default_rng(3)
    sampled = set()
    P_ = fa.w_global.numel()
    mass, c_abs, bank_abs = np.zeros(P_), np.zeros(P_), np.zeros(P_)
    for _ in range(3):
        before = fa.c_bank.clone()
        fa.round()
        mass += (fa.c_bank - before).double().abs().sum(0).numpy() / fa.N  # sum_g |delta_g| / N of the round
        c_abs += fa.c_global.double().abs().numpy()
        bank_abs += fa.c_bank.double().abs().sum(0).numpy() / fa.N
        sampled |= {int(c) for c in rng.choice(fa.N, fa.K, replace=False)}
    never = sorted(set(range(fa.N)) - sampled)
    assert never, "choose a seed that leaves a client out"
    for cl in never:
        assert not bool(fa.c_bank[cl].any())
    assert all(bool(fa.c_bank[cl].any()) for cl in sampled)
    # In exact arithmetic c = sum_r sum_g delta_rg / N = mean of the bank rows, from the same fp32
    # deltas. The fp32 code differs from that by, per round and to first order in u (the oracle's
    # allowances: u |result| per multiply and add):
    #   c    : G products delta / N               <= u mass_r
    #          G adds into acc, partial sums      <= G u mass_r
    #          c + dc                             <= u |c_r|
    #   bank : one add per reporting client, / N  <= u sum_i |bank_r[i]| / N   (over all rows: an upper bound)
    # the float64 mean below adds nothing at this order.
    bound = O.U * ((fa.K + 1) * mass + c_abs + bank_abs)
    mean = fa.c_bank.double().mean(0).numpy()
    err = np.abs(fa.c_global.double().numpy() - mean)
    print("c vs mean of the bank: worst err / bound =", O.ratio(fa.c_global, O.Q(mean, bound)),
          " max |c| / max bound =", float(np.abs(mean).max() / bound.max()))
    assert float(np.abs(mean).max()) > 100 * float(bound.max())  # the bound is no tautology
    assert bool((err <= bound).all())


def test_scaffold_trainer_is_not_direct():
    from ddl25spring_amd.models import mnist_cnn
    arr = synthetic_images("mnist", 100, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    net = mnist_cnn(groups=1).to(CPU, seed=0)
    data.set_input_spec(net.input_spec)
    n_par = net.store.data.shape[1]
    control = (torch.zeros(n_par), torch.zeros(3, n_par), torch.zeros(1, dtype=torch.int32))
    assert LocalTrainer(net, data, 0.1, 50, direct=True).direct is True
    lt = LocalTrainer(net, data, 0.1, 50, direct=True, control=control)
    assert lt.direct is False and all(a is b for a, b in zip(lt.opt.control, control))
    with pytest.raises(ValueError):
        LocalTrainer(net, data, 0.1, 50, prox_mu=0.1, anchor=control[0], control=control)
    with pytest.raises(AssertionError):
        lt.opt.step_direct()
    with pytest.raises(ValueError):  # one table entry per slot
        lt.opt.set_control(control[0], control[1], torch.zeros(2, dtype=torch.int32))


def test_validation():
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(2, True, 1, labels=arr.labels)
    with pytest.raises(ValueError):
        Scaffold(mnist_mlp, data, parts, lr=0.1, prox_mu=0.1)
    fa = Scaffold(mnist_mlp, data, parts, lr=0.1, server_opt="fedavgm", server_opt_kwargs=dict(lr=0.5, beta1=0.0))
    fa.round()  # the paper's global step size: a FedOpt server optimizer behind it
    assert fa.server_opt.steps == 1 and bool(fa.c_global.any())
    assert fa.c_bank.shape == (2, fa.w_global.numel()) and fa.slot_client.shape == (fa.slots,)


def test_dropped_clients_keep_their_control_variate(fp32):
    arr, parts = G.fl_setup()
    fa = G.make_sc(CPU, arr=arr, parts=parts, dropout=0.5, seed=2, use_graph=False)
    for _ in range(2):
        before = fa.c_bank.clone()
        n = len(fa.dropped)
        fa.round()
        for cl in fa.dropped[n]:
            assert torch.equal(fa.c_bank[cl], before[cl])
    assert any(fa.dropped) and bool(fa.c_bank.any())


# --------------------------------------------------------------------------- distributed (gloo)
DIST_KW = dict(lr=0.1, batch_size=50, client_fraction=0.5, seed=7)


def _dist_fed(ctx):
    """4 clients of 80, 90, 100 and 110 samples: K_i = 2, 2, 2, 3 at B = 50, and the single process
    trains its two unequal slots one by one, as each rank trains its one (the CPU engine's batched
    GEMM over equal-sized slots rounds differently from two single ones; that is not under test)."""
    arr = synthetic_images("mnist", 400, seed=0)
    perm = np.random.default_rng(7).permutation(400)
    parts = [perm[a:b] for a, b in ((0, 80), (80, 170), (170, 270), (270, 380))]
    return Scaffold(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, ctx=ctx, **DIST_KW)


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    torch.set_num_threads(1)  # as the single-process run: the CPU GEMMs' bits depend on the thread count
    fa = _dist_fed(ctx)
    for _ in range(3):
        fa.round()
    torch.save({"w": fa.w_global, "c": fa.c_global, "bank": fa.c_bank}, os.path.join(out_dir, f"s{rank}.pt"))
    rdist.shutdown()


def test_distributed_scaffold_matches_single_process(fp32):
    """2 gloo ranks, K = 2, one client per rank, against one process holding both slots, 3 rounds:
    dc's rank-ordered sum adds the slots' terms in the single process's order, and the all-gathered
    rows land in every rank's bank by client id. Bit for bit, with every process on one CPU thread:
    the thread count changes the bits of the CPU engine's GEMMs, and the ranks do not inherit the
    parent's."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        single = _dist_fed(DistContext())
        for _ in range(3):
            single.round()
    finally:
        torch.set_num_threads(nthreads)
    with tempfile.TemporaryDirectory() as d:
        port = 29600 + (os.getpid() % 150)
        mp.spawn(_dist_worker, args=(2, port, d), nprocs=2, join=True)
        s0 = torch.load(os.path.join(d, "s0.pt"), weights_only=True)
        s1 = torch.load(os.path.join(d, "s1.pt"), weights_only=True)
    for k in ("w", "c", "bank"):
        assert torch.equal(s0[k], s1[k]), k  # replicated state stays identical on every rank
    assert bool(s0["bank"].any()) and {single.local_steps(c) for c in range(4)} == {2, 3}
    for k, t in (("w", single.w_global), ("c", single.c_global), ("bank", single.c_bank)):
        assert torch.equal(s0[k], t), (k, (s0[k] - t).abs().max())


# ----------------------------------------------------------------------------------- checkpoints
CKPT_KW = dict(lr=0.05, batch_size=50, client_fraction=0.5, seed=4)


def test_checkpoint_resume_is_identical(fp32):
    """2 rounds, save, 2 more in a fresh server: w_global, c and the bank bit-equal to 4 uninterrupted."""
    from ddl25spring_amd.fl import checkpoint as ckpt
    arr = synthetic_images("mnist", 400, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(6, True, 10, labels=arr.labels)
    ref = Scaffold(mnist_mlp, data, parts, **CKPT_KW)
    ref.run(4)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fl.pt")
        ckpt.run_with_checkpoints(Scaffold(mnist_mlp, data, parts, **CKPT_KW), 2, path)
        b = Scaffold(mnist_mlp, data, parts, **CKPT_KW)  # fresh process-equivalent: rebuild, then resume
        ckpt.run_with_checkpoints(b, 4, path)
    assert b.round_idx == 4
    assert torch.equal(b.w_global, ref.w_global)
    assert torch.equal(b.c_global, ref.c_global) and torch.equal(b.c_bank, ref.c_bank)
    with pytest.raises(ValueError):  # another algorithm's checkpoint is not reinterpreted
        FedAvg(mnist_mlp, data, parts, **CKPT_KW).load_state_dict(ref.state_dict())


def test_checkpoint_layout_remap_moves_the_bank_rows(fp32):
    """A checkpoint whose flat rows use another parameter layout (here: reversed order) has c and
    every bank row remapped by parameter name, as w_global."""
    from ddl25spring_amd.models import mnist_cnn
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(2, True, 10, labels=arr.labels)
    kw = dict(lr=0.05, batch_size=50, client_fraction=1.0, seed=4)
    fa = Scaffold(mnist_cnn, data, parts, **kw)
    fa.run(1)
    st = fa.net.store
    sd = fa.state_dict()
    other = dict(sd)
    rows = {"w_global": sd["w_global"], "c_global": sd["c_global"], "c0": sd["c_bank"][0], "c1": sd["c_bank"][1]}
    flat = {k: torch.zeros_like(t) for k, t in rows.items()}
    layout, off = [], 0
    for name, o, n in reversed(st.param_layout()):
        for k in rows:
            flat[k][off:off + n] = rows[k][o:o + n]
        layout.append([name, off, n])
        off += (n + 15) // 16 * 16
    other["w_global"], other["c_global"], other["param_layout"] = flat["w_global"], flat["c_global"], layout
    other["c_bank"] = torch.stack([flat["c0"], flat["c1"]])
    assert not torch.equal(other["c_bank"], sd["c_bank"]) and bool(sd["c_bank"].any())
    for ck in (sd, other):
        fb = Scaffold(mnist_cnn, data, parts, **kw)
        fb.load_state_dict(ck)
        assert torch.equal(fb.w_global, fa.w_global)
        for name, o, n in st.param_layout():  # every parameter's entries (padding holds no state)
            assert torch.equal(fb.c_global[o:o + n], fa.c_global[o:o + n]), name
            assert torch.equal(fb.c_bank[:, o:o + n], fa.c_bank[:, o:o + n]), name


# --------------------------------------------------------------------------------------- the CLI
def test_cli_scaffold(tmp_path, capsys):
    from ddl25spring_amd.cli import main
    log = tmp_path / "scaffold.jsonl"
    args = ["--device", "cpu", "fl", "--algorithm", "scaffold", "--model", "mnist_mlp", "--clients", "4",
            "--client-fraction", "0.5", "--rounds", "2", "--train-size", "200", "--test-size", "100",
            "--batch-size", "50", "--lr", "0.1", "--server-opt", "fedavgm", "--server-beta1", "0",
            "--server-lr", "1.0", "--iid", "false", "--jsonl", str(log)]
    assert main(args) == 0
    assert "Test accuracy" in capsys.readouterr().out
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert [r["round"] for r in recs] == [1, 2] and np.isfinite(recs[-1]["test_accuracy"])
    with pytest.raises(ValueError):
        main(args + ["--prox-mu", "0.1"])


def test_build_server_passes_the_settings_on():
    from ddl25spring_amd.apps.fl import FLConfig, build_server
    cfg = FLConfig(algorithm="scaffold", model="mnist_mlp", clients=4, train_size=200, test_size=100,
                   batch_size=40, local_epochs=2, lr=0.03, server_opt="fedavgm", server_lr=0.7, server_beta1=0.0,
                   aggregator="median", dropout=0.1)
    srv = build_server(cfg, DistContext())
    assert type(srv) is Scaffold and srv.algorithm == "Scaffold"
    assert (srv.B, srv.E, srv.lr, srv.dropout) == (40, 2, 0.03, 0.1)
    assert (srv.server_opt.kind, srv.server_opt.lr, srv.server_opt.beta1) == ("sgdm", 0.7, 0.0)
    assert srv.aggregator.name == "median"
    assert srv.local_steps(0) == 2 * -(-srv.counts[0] // 40)
