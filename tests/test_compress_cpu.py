"""Compressed uploads without a GPU: the torch twins on the cases of tests/test_compress_gpu.py
against the oracle (tests/compress_oracle.py), and the engine: defaults, a hand-driven round,
conservation of the error feedback, dropped clients, two gloo ranks, checkpoints, the CLI and the
rejected combinations."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import compress_oracle as O
import test_compress_gpu as G
import ddl25spring_amd.ops.reference as R
from ddl25spring_amd.data.images import DeviceImageDataset, synthetic_images
from ddl25spring_amd.data.split import split
from ddl25spring_amd.fl.algorithms import FedAvg, FedSGD, FedSgdWeight, Scaffold
from ddl25spring_amd.fl.compress import Quantize, TopK, dense_bytes, make_compressor
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
    # x = 1, y = (4, 1, -2, 1.5), e = (0, 0.5, 0, -0.5): u = (3, 0.5, -3, 0). k = 1: tau = 3, the +-3
    # tie is kept whole (nnz 2); the zero is never kept, 0.5 goes to the bank
    x, y, e = [1.0] * 4, [4.0, 1.0, -2.0, 1.5], [0.0, 0.5, 0.0, -0.5]
    row, bank, nnz, tau = O.topk_row(y, x, e, 1)
    assert row.tolist() == [4.0, 1.0, -2.0, 1.0] and bank.tolist() == [0.0, 0.5, 0.0, 0.0] and nnz == 2
    assert tau == np.float32(3.0).view(np.uint32)
    # k = 3 and k = 9 (more than the 3 non-zeros): tau is the smallest, 0.5
    for k in (3, 9):
        row, bank, nnz, _ = O.topk_row(y, x, e, k)
        assert row.tolist() == [4.0, 1.5, -2.0, 1.0] and not bank.any() and nnz == 3
    # without a bank u = y - x = (3, 0, -3, 0.5)
    row, bank, nnz, _ = O.topk_row(y, x, None, 3)
    assert row.tolist() == [4.0, 1.0, -2.0, 1.5] and bank is None and nnz == 3
    # a NaN passes through and keeps its bank entry; the rest selects as before
    row, bank, nnz, _ = O.topk_row([float("nan"), 1.0, -2.0, 1.5], x, [7.0, 0.5, 0.0, -0.5], 1)
    assert np.isnan(row[0]) and row[1:].tolist() == [1.0, -2.0, 1.0] and bank.tolist() == [7.0, 0.5, 0.0, 0.0]
    assert nnz == 1
    # quantization, bits = 3 (L = 3): u = (3, -1.5, 0, inf): s = 3, a* = (3, 1.5, 0, -), levels 3, 1 or 2, 0, 0
    u = np.array([3.0, -1.5, 0.0, np.inf], dtype=np.float32)
    s, a, r, lv, finite, amb = O.quant_row(u, 2, 3, 9, 0)
    assert s.tolist() == [3.0] and a.tolist() == [3.0, 1.5, 0.0, 0.0] and finite.tolist() == [True, True, True, False]
    assert lv[0] == 3 and lv[1] == (2 if 0.5 >= r[1] else 1) and lv[2] == 0 and lv[3] == 0
    assert bool(((r > 0) & (r <= 1)).all()) and not amb[0]
    # the draws are a function of (seed, round, client, column) and of nothing else
    assert np.array_equal(O.draws(9, 2, 9, 0)[:5], O.draws(5, 2, 9, 0))
    for other in (O.draws(9, 3, 9, 0), O.draws(9, 2, 10, 0), O.draws(9, 2, 9, 1)):
        assert not np.array_equal(other, O.draws(9, 2, 9, 0))
    assert O.bucket_scales(np.zeros(300, dtype=np.float32)).tolist() == [0.0, 0.0]


def test_uplink_byte_counts():
    assert TopK(0.1).k(1000) == 100 and TopK(1e-9).k(1000) == 1
    assert TopK(0.1).uplink_bytes(1000, 103) == 8 * 103
    assert Quantize(4).uplink_bytes(1000) == 500 + 4 * 4 and Quantize(2).uplink_bytes(257) == 65 + 8
    assert dense_bytes(1000) == 4000
    assert isinstance(make_compressor("topk", ratio=0.5), TopK) and make_compressor("quant", bits=2).bits == 2
    with pytest.raises(ValueError):
        make_compressor("sign")


# -------------------------------------------------------------------------- CPU twins in ``Fn``
@pytest.mark.parametrize("P_", G.TOPK_P)
@pytest.mark.parametrize("K", G.TOPK_G)
def test_topk_is_bit_exact_cpu(K, P_):
    G.check_topk(K, P_, CPU)


def test_topk_without_bank_drops_the_rest_cpu():
    G.check_topk_without_bank_drops(CPU)


def test_topk_second_grid_stride_iteration_cpu():
    G.check_topk_second_pass(CPU)


@pytest.mark.parametrize("bits_", G.QUANT_BITS)
@pytest.mark.parametrize("P_", G.QUANT_P)
@pytest.mark.parametrize("K", G.TOPK_G)
def test_quantize_cpu(K, P_, bits_):
    G.check_quantize(K, P_, bits_, CPU)


def test_quantize_zero_and_nonfinite_buckets_cpu():
    G.check_quantize_buckets(CPU)


def test_two_calls_are_bit_equal_cpu():
    G.check_deterministic(CPU)


def test_op_rejects_bad_arguments_cpu():
    G.check_rejects(CPU)
    rows, x, bank = torch.zeros(2, 8), torch.zeros(8), torch.zeros(3, 8)
    nnz = torch.zeros(2, dtype=torch.int32)
    for ids in ([0, 3], [1, 1]):  # a host table is checked by the op itself
        t = torch.tensor(ids, dtype=torch.int32)
        with pytest.raises(ValueError):
            Fn.topk_compress(rows, x, bank, t, 1, nnz)
        with pytest.raises(ValueError):
            Fn.quantize_compress(rows, x, bank, t, 4, 0, 0)


# ------------------------------------------------------------------------------------- the engine
TOPK = dict(compressor="topk", compressor_kwargs=dict(ratio=0.1))
QUANT = dict(compressor="quant", compressor_kwargs=dict(bits=4, seed=5))


def test_compressor_none_changes_no_bit(fp32):
    a, b = G.make_fed(CPU, use_graph=False), G.make_fed(CPU, use_graph=False, compressor=None)
    for _ in range(2):
        a.round()
        b.round()
    assert torch.equal(G.bits(a.w_global), G.bits(b.w_global))
    assert b.compressor is None and b.uplink_bytes == [] and "compressor" not in b.state_dict()


def test_compressed_round_matches_a_hand_driven_round(fp32):
    """Two rounds of the engine against a loop driven by hand on a plain FedAvg: its trainer's local
    epochs, Fn.topk_compress on the rows with a bank and table held outside the class, Fn.weighted_sum.
    Bit for bit, the second round with a non-zero bank."""
    kw = dict(lr=0.1, batch_size=60, use_graph=False, client_fraction=0.5)
    fa = G.make_fed(CPU, **kw, **TOPK)
    fa.round()
    fa.round()
    fb = G.make_fed(CPU, **kw)
    st = fb.net.store
    n_par = fb.w_global.numel()
    bank, up = torch.zeros(fb.N, n_par), []
    k = max(1, round(0.1 * n_par))
    for r in range(2):
        chosen = fb._sample()
        mine, _ = fb._assign(chosen)
        K = len(mine)
        fb._download(K)
        seeds = [fb.seed + cl + 1 + r * fb.K for cl in mine]
        fb._trainer(mine).run([fb.client_indices[cl] for cl in mine], seeds, fb.E, None)
        nnz = torch.zeros(K, dtype=torch.int32)
        Fn.topk_compress(st.data[:K], fb.w_global, bank, torch.tensor(mine, dtype=torch.int32), k, nnz)
        up.append(8 * int(nnz.sum()) + 4 * fb.b_global.numel() * K)
        total = float(sum(fb.counts[cl] for cl in mine))
        coeff = torch.tensor([fb.counts[cl] / total for cl in mine], dtype=torch.float32)
        Fn.weighted_sum(st.data[:K], coeff, fb.w_global)
        fb.round_idx += 1
    assert bool(bank.any())
    assert torch.equal(fa.w_global, fb.w_global) and torch.equal(fa.compressor.bank, bank)
    assert fa.uplink_bytes == up and fa.compressor.round == 2


class Recording(FedAvg):
    """FedAvg that records what the codec saw and made of it."""

    def _compress(self, mine, chosen):
        st, K = self.net.store, len(mine)
        y, x, e0 = st.data[:K].clone(), self.w_global.clone(), self.compressor.bank[mine].clone()
        super()._compress(mine, chosen)
        self.__dict__.setdefault("seen", []).append((list(mine), x, y, e0, st.data[:K].clone(),
                                                      self.compressor.bank[mine].clone()))


@pytest.mark.parametrize("codec", [TOPK, QUANT], ids=["topk", "quant"])
def test_error_feedback_conserves_the_updates(fp32, codec):
    """3 rounds, no attack: for every client and column, what was transmitted plus what the bank
    still holds is what the client's raw updates add up to."""
    arr = synthetic_images("mnist", 600, seed=0)
    parts = split(6, True, 3, labels=arr.labels)
    fa = G.make_fed(CPU, arr=arr, parts=parts, cls=Recording, lr=0.05, client_fraction=0.5, use_graph=False, **codec)
    for _ in range(3):
        fa.round()
    n_par = fa.w_global.numel()
    raw, sent, bound = (np.zeros((fa.N, n_par)) for _ in range(3))
    U = 2.0 ** -24
    for mine, x, y, e0, row, e1 in fa.seen:
        for g, cl in enumerate(mine):
            d = (y[g] - x).double().numpy()              # the raw update, as the codec forms it (fp32)
            q = row[g].double().numpy() - x.double().numpy()  # what the server decodes, x taken off exactly
            raw[cl] += d
            sent[cl] += q
            # per round: u = fl32(d + e0) is one rounding of |u|; the row fl32(x + q) one of |row|; the
            # new error fl32(u - q) one of |e1| (exact for top-k); to first order in U, with 2 % slack
            u_abs = np.abs(d + e0[g].double().numpy())
            bound[cl] += 1.02 * U * (u_abs + np.abs(row[g].double().numpy()) + np.abs(e1[g].double().numpy()))
    err = np.abs(sent + fa.compressor.bank.double().numpy() - raw)
    print("conservation: worst err / bound =", float((err / np.maximum(bound, 1e-300)).max()))
    assert bool((err <= bound).all())
    assert float(np.abs(raw).max()) > 100 * float(bound.max())  # the bound is no tautology
    assert bool(fa.compressor.bank.any()) and len({c for s in fa.seen for c in s[0]}) >= 4


def test_dropped_clients_keep_their_error_row(fp32):
    fa = G.make_fed(CPU, dropout=0.5, seed=2, use_graph=False, **TOPK)
    for _ in range(2):
        before = fa.compressor.bank.clone()
        n = len(fa.dropped)
        fa.round()
        for cl in fa.dropped[n]:
            assert torch.equal(fa.compressor.bank[cl], before[cl])
    assert any(fa.dropped) and bool(fa.compressor.bank.any()) and len(fa.uplink_bytes) == 2


def test_rejected_combinations():
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(2, True, 1, labels=arr.labels)
    for cls in (Scaffold, FedSGD):
        with pytest.raises(ValueError):
            cls(mnist_mlp, data, parts, lr=0.1, **TOPK)
    with pytest.raises(ValueError):
        FedAvg(mnist_mlp, data, parts, lr=0.1, compressor="sign")
    with pytest.raises(ValueError):
        FedAvg(mnist_mlp, data, parts, lr=0.1, compressor="quant", compressor_kwargs=dict(bits=9))
    fw = FedSgdWeight(mnist_mlp, data, parts, lr=0.1, **QUANT)  # one full-batch step per client, then the codec
    fw.round()
    assert fw.uplink_bytes == [2 * (Quantize(4).uplink_bytes(fw.w_global.numel()) + 4 * fw.b_global.numel())]
    nb = FedAvg(mnist_mlp, data, parts, lr=0.1, compressor=TopK(0.5, error_feedback=False))
    nb.round()
    assert nb.compressor.bank is None and len(nb.uplink_bytes) == 1


# --------------------------------------------------------------------------- distributed (gloo)
DIST_KW = dict(lr=0.1, batch_size=50, client_fraction=0.5, seed=7)


def _dist_fed(ctx, codec):
    """As test_scaffold_cpu._dist_fed: 4 clients of unequal size, so the single process trains its
    two slots one by one, as each rank trains its one."""
    arr = synthetic_images("mnist", 400, seed=0)
    perm = np.random.default_rng(7).permutation(400)
    parts = [perm[a:b] for a, b in ((0, 80), (80, 170), (170, 270), (270, 380))]
    return FedAvg(mnist_mlp, DeviceImageDataset(arr, "cpu"), parts, ctx=ctx, **DIST_KW, **codec)


def _dist_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    R._bf = lambda t: t.float()
    P.CPU_SHADOW_DTYPE = torch.float32
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu")
    torch.set_num_threads(1)  # as the single-process run: the CPU GEMMs' bits depend on the thread count
    out = {}
    for name, codec in (("topk", TOPK), ("quant", QUANT)):
        fa = _dist_fed(ctx, codec)
        for _ in range(3):
            fa.round()
        out[name] = {"w": fa.w_global, "bank": fa.compressor.bank, "up": torch.tensor(fa.uplink_bytes)}
    torch.save(out, os.path.join(out_dir, f"s{rank}.pt"))
    rdist.shutdown()


def test_distributed_compression_matches_single_process(fp32):
    """2 gloo ranks, K = 2, one client per rank, against one process holding both slots, 3 rounds, by
    the criterion of test_distributed_scaffold_matches_single_process: bit for bit, the replicated
    bank included, and the same uplink bytes."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        single = {}
        for name, codec in (("topk", TOPK), ("quant", QUANT)):
            single[name] = _dist_fed(DistContext(), codec)
            for _ in range(3):
                single[name].round()
    finally:
        torch.set_num_threads(nthreads)
    with tempfile.TemporaryDirectory() as d:
        port = 29250 + (os.getpid() % 150)
        mp.spawn(_dist_worker, args=(2, port, d), nprocs=2, join=True)
        s0 = torch.load(os.path.join(d, "s0.pt"), weights_only=True)
        s1 = torch.load(os.path.join(d, "s1.pt"), weights_only=True)
    for name, fa in single.items():
        for k in ("w", "bank", "up"):
            assert torch.equal(s0[name][k], s1[name][k]), (name, k)  # replicated state stays identical
        assert bool(s0[name]["bank"].any())
        assert torch.equal(s0[name]["w"], fa.w_global), (name, (s0[name]["w"] - fa.w_global).abs().max())
        assert torch.equal(s0[name]["bank"], fa.compressor.bank), name
        assert s0[name]["up"].tolist() == fa.uplink_bytes, name


# ----------------------------------------------------------------------------------- checkpoints
CKPT_KW = dict(lr=0.05, batch_size=50, client_fraction=0.5, seed=4)


@pytest.mark.parametrize("codec", [TOPK, QUANT], ids=["topk", "quant"])
def test_checkpoint_resume_is_identical(fp32, codec):
    """2 rounds, save, 2 more in a fresh server: w_global, the bank, the codec's round and the uplink
    bytes equal 4 uninterrupted rounds."""
    from ddl25spring_amd.fl import checkpoint as ckpt
    arr = synthetic_images("mnist", 400, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(6, True, 10, labels=arr.labels)
    ref = FedAvg(mnist_mlp, data, parts, **CKPT_KW, **codec)
    ref.run(4)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fl.pt")
        ckpt.run_with_checkpoints(FedAvg(mnist_mlp, data, parts, **CKPT_KW, **codec), 2, path)
        b = FedAvg(mnist_mlp, data, parts, **CKPT_KW, **codec)  # fresh process-equivalent: rebuild, then resume
        ckpt.run_with_checkpoints(b, 4, path)
    assert b.round_idx == 4 and b.compressor.round == ref.compressor.round == 4
    assert torch.equal(b.w_global, ref.w_global) and torch.equal(b.compressor.bank, ref.compressor.bank)
    assert b.uplink_bytes == ref.uplink_bytes and len(b.uplink_bytes) == 4
    other = QUANT if codec is TOPK else TOPK
    with pytest.raises(ValueError):  # another codec's state is not reinterpreted
        FedAvg(mnist_mlp, data, parts, **CKPT_KW, **other).load_state_dict(ref.state_dict())


def test_checkpoint_layout_remap_moves_the_bank_rows(fp32):
    """A checkpoint whose flat rows use another parameter layout (here: reversed order) has every
    error row remapped by parameter name, as w_global."""
    from ddl25spring_amd.models import mnist_cnn
    arr = synthetic_images("mnist", 200, seed=0)
    data = DeviceImageDataset(arr, "cpu")
    parts = split(2, True, 10, labels=arr.labels)
    kw = dict(lr=0.05, batch_size=50, client_fraction=1.0, seed=4, **TOPK)
    fa = FedAvg(mnist_cnn, data, parts, **kw)
    fa.run(1)
    st = fa.net.store
    sd = fa.state_dict()
    bank = sd["compressor"]["bank"]
    rows = {"w_global": sd["w_global"], "e0": bank[0], "e1": bank[1]}
    flat = {k: torch.zeros_like(t) for k, t in rows.items()}
    layout, off = [], 0
    for name, o, n in reversed(st.param_layout()):
        for k in rows:
            flat[k][off:off + n] = rows[k][o:o + n]
        layout.append([name, off, n])
        off += (n + 15) // 16 * 16
    other = dict(sd, w_global=flat["w_global"], param_layout=layout,
                 compressor=dict(sd["compressor"], bank=torch.stack([flat["e0"], flat["e1"]])))
    assert not torch.equal(other["compressor"]["bank"], bank) and bool(bank.any())
    for ck in (sd, other):
        fb = FedAvg(mnist_cnn, data, parts, **kw)
        fb.load_state_dict(ck)
        assert torch.equal(fb.w_global, fa.w_global) and fb.compressor.round == 1
        for name, o, n in st.param_layout():  # every parameter's entries (padding holds no state)
            assert torch.equal(fb.compressor.bank[:, o:o + n], fa.compressor.bank[:, o:o + n]), name


# --------------------------------------------------------------------------------------- the CLI
def test_cli_compress(tmp_path, capsys):
    from ddl25spring_amd.cli import main
    base = ["--device", "cpu", "fl", "--model", "mnist_mlp", "--clients", "4", "--client-fraction", "0.5",
            "--rounds", "2", "--train-size", "200", "--test-size", "100", "--batch-size", "50", "--lr", "0.1"]
    log = tmp_path / "topk.jsonl"
    assert main(base + ["--compress", "topk", "--compress-ratio", "0.05", "--jsonl", str(log)]) == 0
    assert "Test accuracy" in capsys.readouterr().out
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    assert [r["round"] for r in recs] == [1, 2] and all(r["uplink_bytes"] > 0 for r in recs)
    dense = tmp_path / "dense.jsonl"
    assert main(base + ["--jsonl", str(dense)]) == 0
    assert all("uplink_bytes" not in json.loads(ln) for ln in dense.read_text().splitlines())
    with pytest.raises(ValueError):
        main(base + ["--compress", "topk", "--algorithm", "scaffold"])
    with pytest.raises(ValueError):
        main(base + ["--compress", "sign"])


def test_build_server_passes_the_settings_on():
    from ddl25spring_amd.apps.fl import FLConfig, build_server
    base = dict(model="mnist_mlp", clients=4, train_size=200, test_size=100, batch_size=40, seed=6)
    srv = build_server(FLConfig(compress="topk", compress_ratio=0.02, error_feedback=False, **base), DistContext())
    assert type(srv.compressor) is TopK and srv.compressor.ratio == 0.02 and srv.compressor.bank is None
    srv = build_server(FLConfig(compress="quant", compress_bits=2, algorithm="fedsgd_weight", **base), DistContext())
    assert type(srv.compressor) is Quantize and (srv.compressor.bits, srv.compressor.seed) == (2, 6)
    assert srv.compressor.bank.shape == (4, srv.w_global.numel())
    assert build_server(FLConfig(**base), DistContext()).compressor is None
