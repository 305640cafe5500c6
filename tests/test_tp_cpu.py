"""Tensor parallelism on the CPU gloo backend: the sharding rule and its inverse, sharded models
against the single-process model, the dp x tp grid, determinism, checkpoint / resume and the CLI."""
import hashlib
import json
import os
import sys
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from ddl25spring_amd.models.llama import LLama, causalLLMLoss
from ddl25spring_amd.parallel.tp import gather_llama, shard_llama, vocab_range

TINY = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=4, ctx_size=16)
TINY3 = dict(vocab_size=100, dmodel=48, num_heads=3, n_layers=2, ctx_size=16, ffn_hidden=96)
PG_TIMEOUT_S = 60  # a mismatched collective fails the test instead of waiting out the default


def test_vocab_range():
    assert [vocab_range(100, 3, t) for t in range(3)] == [(0, 48), (48, 96), (96, 100)]
    assert [vocab_range(32000, 3, t) for t in range(3)] == [(0, 10672), (10672, 21344), (21344, 32000)]
    assert vocab_range(96, 1, 0) == (0, 96)
    with pytest.raises(ValueError, match="without any"):
        vocab_range(96, 4, 0)  # shards of 32 rows: the fourth would be empty


@pytest.mark.parametrize("cfg,tp", [(TINY, 2), (TINY3, 3)])
def test_shard_gather_round_trip(cfg, tp):
    torch.manual_seed(0)
    full = {n: p.detach().clone() for n, p in LLama(**cfg).named_parameters()}
    shards = []
    for t in range(tp):
        torch.manual_seed(0)
        m = shard_llama(LLama(**cfg), tp, t)
        assert m.first.layers[0].h == cfg["num_heads"] // tp
        shards.append({n: p.detach() for n, p in m.named_parameters()})
    assert shards[0]["first.layers.0.wqkv"].shape == (3 * cfg["dmodel"] // tp, cfg["dmodel"])
    assert shards[0]["first.layers.0.wo"].shape == (cfg["dmodel"], cfg["dmodel"] // tp)
    assert shards[tp - 1]["last.head"].shape[0] == cfg["vocab_size"] - vocab_range(cfg["vocab_size"], tp, tp - 1)[0]
    back = gather_llama(shards, {n: p.shape for n, p in full.items()})
    assert back.keys() == full.keys()
    for n in full:
        assert torch.equal(back[n], full[n]), n


def test_configuration_errors():
    from ddl25spring_amd.apps.llm import LLMConfig, train_llm
    from ddl25spring_amd.runtime.dist import DistContext
    with pytest.raises(ValueError, match="num_heads"):
        shard_llama(LLama(**TINY), 4, 0)  # 2 heads over 4 ranks
    with pytest.raises(ValueError, match="FFN"):
        shard_llama(LLama(**dict(TINY3, ffn_hidden=100)), 3, 0)
    with pytest.raises(ValueError, match="without any"):
        shard_llama(LLama(**dict(TINY, vocab_size=30, num_heads=4)), 4, 0)  # 16-row shards: 16 + 14 + 0
    tiny = dict(TINY, batch_size=2, iters=1)
    for kw, world, msg in [(dict(tp=2, pp=2), 4, "pp"), (dict(tp=2, precision="bf16"), 2, "fp32"),
                           (dict(tp=2, dp=2, dp_mode="wa"), 4, "dp_mode"), (dict(tp=2), 4, "world"),
                           (dict(tp=4), 4, "num_heads")]:
        with pytest.raises(ValueError, match=msg):  # raised before any group is created
            train_llm(LLMConfig(**tiny, **kw), DistContext(rank=0, world=world), log=None)


# ----------------------------------------------------------- sharded model vs single process
def _tp_model_worker(rank, world, port, cfg, out_dir, micro):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from ddl25spring_amd.parallel.tp import TPHandle
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu", timeout_s=PG_TIMEOUT_S)
    tph = TPHandle(ctx, None, world, rank)
    torch.manual_seed(0)
    model = shard_llama(LLama(**cfg), world, rank, tph)
    torch.manual_seed(123)
    x = torch.randint(0, cfg["vocab_size"], (6, cfg["ctx_size"]))
    loss = 0.0
    for m in torch.chunk(x, micro):
        l = causalLLMLoss(model(m), m, cfg["vocab_size"], scale=1.0 / micro, tp=tph)
        l.backward()
        loss = loss + l.detach()
    torch.save({"loss": loss, "grads": {n: p.grad.clone() for n, p in model.named_parameters()}},
               os.path.join(out_dir, f"r{rank}.pt"))
    rdist.shutdown()


@pytest.mark.parametrize("cfg,tp,port", [(TINY, 2, 29801), (TINY3, 3, 29803)])
def test_tp_matches_single_process(cfg, tp, port):
    micro = 2
    torch.manual_seed(123)
    x = torch.randint(0, cfg["vocab_size"], (6, cfg["ctx_size"]))
    torch.manual_seed(0)
    model = LLama(**cfg)
    loss_ref = sum(causalLLMLoss(model(m), m) for m in torch.chunk(x, micro)) / micro
    loss_ref.backward()
    ref = {n: p.grad for n, p in model.named_parameters()}
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_tp_model_worker, args=(tp, port, cfg, d, micro), nprocs=tp, join=True)
        res = [torch.load(os.path.join(d, f"r{r}.pt"), weights_only=True) for r in range(tp)]
    for r in res:
        assert torch.equal(r["loss"], res[0]["loss"])  # the same bits on every rank
        assert abs(r["loss"].item() - loss_ref.item()) < 1e-5
    for n in ref:  # replicated parameters: the same gradient bits on every rank
        if res[0]["grads"][n].shape == ref[n].shape:
            for r in res[1:]:
                assert torch.equal(r["grads"][n], res[0]["grads"][n]), n
    full = gather_llama([r["grads"] for r in res], {n: g.shape for n, g in ref.items()})
    assert full.keys() == ref.keys()
    for n, g in ref.items():
        assert torch.allclose(full[n], g, atol=1e-5, rtol=1e-4), n


# ------------------------------------------------------------------------------ dp x tp grid
def _grid_worker(rank, world, port, out_dir, tp=2):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from ddl25spring_amd.parallel.dp import GradBucketer
    from ddl25spring_amd.parallel.tp import TPHandle
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu", timeout_s=PG_TIMEOUT_S)
    dp = world // tp
    pipe, t = divmod(rank, tp)  # the program's layout: tp groups are consecutive ranks
    dp_group = ctx.new_groups("dp", [[p * tp + k for p in range(dp)] for k in range(tp)])
    tp_group = ctx.new_groups("tp", [[p * tp + k for k in range(tp)] for p in range(dp)])
    tph = TPHandle(ctx, tp_group, tp, t)
    torch.manual_seed(0)
    model = shard_llama(LLama(**TINY), tp, t, tph)
    bk = GradBucketer(model, ctx, group=dp_group, bucket_mb=0.01)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    torch.manual_seed(99)
    x = torch.randint(0, TINY["vocab_size"], (4, TINY["ctx_size"]))
    mine = x[pipe * 2:(pipe + 1) * 2]
    for _ in range(2):
        bk.zero_grad()
        causalLLMLoss(model(mine), mine, TINY["vocab_size"], tp=tph).backward()
        bk.finish()
        opt.step()
    torch.save({n: p.detach().clone() for n, p in model.named_parameters()}, os.path.join(out_dir, f"r{rank}.pt"))
    rdist.shutdown()


def test_dp2_x_tp2_equals_large_batch():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_grid_worker, args=(4, 29811, d), nprocs=4, join=True)
        w = [torch.load(os.path.join(d, f"r{r}.pt"), weights_only=True) for r in range(4)]
    for t in range(2):  # replicas (rank t and rank 2 + t) agree bit for bit
        for n in w[t]:
            assert torch.equal(w[t][n], w[2 + t][n]), (t, n)
    torch.manual_seed(0)
    ref = LLama(**TINY)
    opt = torch.optim.SGD(ref.parameters(), lr=0.1)
    torch.manual_seed(99)
    x = torch.randint(0, TINY["vocab_size"], (4, TINY["ctx_size"]))
    for _ in range(2):
        opt.zero_grad()
        ((causalLLMLoss(ref(x[:2]), x[:2]) + causalLLMLoss(ref(x[2:]), x[2:])) / 2).backward()
        opt.step()
    full = gather_llama([w[0], w[1]], {n: p.shape for n, p in ref.named_parameters()})
    for n, p in ref.named_parameters():
        assert torch.allclose(full[n], p.detach(), atol=1e-5), n


# ------------------------------------------------- the program: determinism, resume, the CLI
LLM = dict(TINY, batch_size=4, micro_batches=2, log_every=1)


def _llm_worker(rank, world, port, cfg_kw, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from ddl25spring_amd.apps.llm import LLMConfig, train_llm
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cpu", timeout_s=PG_TIMEOUT_S)
    res = train_llm(LLMConfig(**cfg_kw), ctx, log=None)
    torch.save({"losses": res["losses"], "resumed_from": res["resumed_from"]}, os.path.join(out, f"res{rank}.pt"))
    rdist.shutdown()


def _run(world, port, cfg_kw, out):
    os.makedirs(out, exist_ok=True)
    mp.spawn(_llm_worker, args=(world, port, cfg_kw, out), nprocs=world, join=True)
    return [torch.load(os.path.join(out, f"res{r}.pt"), weights_only=True) for r in range(world)]


def _shards(d, step, world):
    return [torch.load(os.path.join(d, f"step{step:08d}", f"rank{r:05d}.pt"), weights_only=True)["state"]
            for r in range(world)]


def _hash(state):
    h = hashlib.sha256()
    for n in sorted(state["model"]):
        h.update(state["model"][n].numpy().tobytes())
    return h.hexdigest()


def test_tp2_run_is_repeatable():
    cfg = dict(LLM, tp=2, iters=3)
    with tempfile.TemporaryDirectory() as d:
        runs = []
        for i in range(2):
            ck = os.path.join(d, f"ck{i}")
            res = _run(2, 29821 + i, dict(cfg, ckpt_dir=ck), os.path.join(d, f"o{i}"))
            assert res[0]["losses"] == res[1]["losses"] and len(res[0]["losses"]) == 3  # bit-equal across ranks
            runs.append(([_hash(s) for s in _shards(ck, 3, 2)], res[0]["losses"]))
    assert runs[0] == runs[1]
    assert runs[0][0][0] != runs[0][0][1]  # two different shards


def _assert_identical(a, b, path=""):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _assert_identical(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_identical(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


def test_dp2_tp2_resume_is_bit_identical():
    """Checkpoint at step 2 of 4, restart: the dp = 2 x tp = 2 job ends as the uninterrupted one."""
    cfg = dict(LLM, dp=2, tp=2)
    with tempfile.TemporaryDirectory() as d:
        full, part = os.path.join(d, "full"), os.path.join(d, "part")
        r_full = _run(4, 29831, dict(cfg, iters=4, ckpt_dir=full), os.path.join(d, "o1"))
        _run(4, 29832, dict(cfg, iters=2, ckpt_dir=part), os.path.join(d, "o2"))
        meta = json.load(open(os.path.join(part, "latest.json")))
        assert meta["step"] == 2
        r_res = _run(4, 29833, dict(cfg, iters=4, ckpt_dir=part), os.path.join(d, "o3"))
        assert all(r["resumed_from"] == 2 for r in r_res)
        a, b = _shards(full, 4, 4), _shards(part, 4, 4)
        for r in range(4):
            _assert_identical(a[r], b[r], f"rank{r}")
            assert r_res[r]["losses"] == [x for x in r_full[r]["losses"] if x[0] >= 2]
        for t in range(2):  # the two pipelines' replicas of shard t
            _assert_identical(a[t]["model"], a[2 + t]["model"], f"shard{t}")


def test_run_tag_names_tp_only_when_sharded():
    from ddl25spring_amd.apps.llm import LLMConfig, _run_tag
    assert "tp" not in _run_tag(LLMConfig())  # checkpoints written before the tp axis still resume
    assert _run_tag(LLMConfig(tp=2)).endswith(",tp=2")


def test_cli_accepts_tp_via_launcher():
    from ddl25spring_amd.runtime.launch import launch
    args = ["llm", "--dp", "2", "--tp", "2", "--iters", "2", "--dmodel", "32", "--num-heads", "2", "--n-layers", "2",
            "--ctx-size", "16", "--vocab-size", "96", "--batch-size", "2", "--log-every", "1"]
    with tempfile.TemporaryDirectory() as d:
        res = launch([sys.executable, "-m", "ddl25spring_amd", "--device", "cpu"] + args, 4, log_dir=d, timeout=240)
        logs = [open(os.path.join(d, f"out{r}.txt")).read() for r in range(4)]
    assert res["returncode"] == 0, "\n".join(logs)
    summary = json.loads(logs[0].strip().splitlines()[-1])
    assert summary["config"]["tp"] == 2 and summary["tokens_per_s"] > 0
    assert all("iter 1 loss" in lg for lg in logs)  # every tp rank holds the loss
