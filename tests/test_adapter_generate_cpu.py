"""Per-sequence LoRA adapters in generation, on the CPU: the torch references of the two ops
(ops/llama_decode.py: lora_rows_u, lin_rows(lora=...)) against the float64 oracle and its derived
bound (tests/lora_decode_oracle.py), the argument checks, ``generate(adapters=..., adapter_ids=...)``
against ``merge_lora`` + ``generate``, and ``FedLoRA`` with ``sample_adapters="clients"``."""
import pytest
import torch

import adapter_fixture as F
import decode_oracle as O
import lora_decode_oracle as LO
from ddl25spring_amd.models.llama import KVCache
from ddl25spring_amd.models.lora import adapter_bank, merge_lora, unmerge_lora
from ddl25spring_amd.ops import llama_decode as D

_rel = O.rel


def _run_case(case, shared, ids, dev="cpu"):
    """(u, y, plain y) of one case through the ops on ``dev``, outputs pre-filled with NaN."""
    T, C, K, r = case["dims"]
    to = lambda t: None if t is None else t.to(dev)  # noqa: E731
    x, w, res, gain = to(case["x"]), to(case["w"]), to(case["res"]), to(case["gain"])
    rows = case["rows"].to(dev)
    a, b, a_shared = F.views(rows, case)
    a = a_shared if shared else a
    idt = torch.tensor(ids, dtype=torch.int32, device=dev)
    u = torch.full((T, r), float("nan"), device=dev)
    y = torch.full((T, K), float("nan"), device=dev)
    D.lora_rows_u(x, a, idt, u, case["pro"], gain)
    D.lin_rows(x, w, y, res, case["pro"], gain, lora=(u, b, idt, 2.0))
    plain = torch.full((T, K), float("nan"), device=dev)
    D.lin_rows(x, w, plain, res, case["pro"], gain)
    return u, y, plain, a, b


def check_case(args, shared, dev="cpu"):
    """Every element of u and y within the oracle's bound; rows without an adapter equal plain
    ``lin_rows``; with every id -1 the whole output does."""
    case = F.op_case(*args)
    ids = case["ids"]
    u, y, plain, a, b = _run_case(case, shared, ids, dev)
    qu = LO.shrink(case["x"], a, ids, case["pro"], case["gain"])
    qy = LO.expand(case["x"], case["w"], u, b, ids, 2.0, case["res"], case["pro"], case["gain"])
    ru, ry = LO.ratio(u, qu), LO.ratio(y, qy)
    print(f"{args} shared={shared} on {dev}: worst error / bound: u {ru:.3f}, y {ry:.3f}")
    assert ru <= 1.0 and ry <= 1.0
    for t, k in enumerate(ids):
        if k < 0:
            assert torch.equal(y[t], plain[t]) and bool((u[t] == 0).all())
    u0, y0, plain0, _, _ = _run_case(case, shared, [-1] * len(ids), dev)
    assert torch.equal(y0, plain0) and bool((u0 == 0).all())


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("args", F.OP_CASES)
def test_references_meet_the_oracle_bound(args, shared):
    check_case(args, shared)


def test_ids_out_of_range_mean_no_adapter():
    case = F.op_case(*F.OP_CASES[1])  # T = 3
    _, y, plain, _, _ = _run_case(case, False, [F.R, -7, 1 << 30])
    assert torch.equal(y, plain)
    _, y, plain, _, _ = _run_case(case, False, [0, 1, 2])
    assert not bool((y == plain).all(1).any())


def test_shared_a_is_one_adapter_for_every_slot():
    case = F.op_case(*F.OP_CASES[1])
    a, _, a_shared = F.views(case["rows"], case)
    assert a_shared.stride(0) == 0
    u, want = torch.empty(3, 4), torch.empty(3, 4)
    D.lora_rows_u(case["x"], a_shared, torch.tensor([0, 1, 2], dtype=torch.int32), u)
    D.lora_rows_u(case["x"], a, torch.tensor([1, 1, 1], dtype=torch.int32), want)
    assert torch.equal(u, want) and _rel(u, case["x"].double() @ a[1].double().t()) < 1e-6


def bad_argument_calls(dev="cpu"):
    """[(label, call)]: each must raise ValueError; the calls share ``out``, filled with 7."""
    case = F.op_case(*F.OP_CASES[1])  # T 3, C 96, K 160, r 4
    rows = case["rows"].to(dev)
    a, b, _ = F.views(rows, case)
    x, w = case["x"].to(dev), case["w"].to(dev)
    ids = torch.tensor([0, 1, -1], dtype=torch.int32, device=dev)
    out = dict(u=torch.full((17, 16), 7.0, device=dev), y=torch.full((17, 160), 7.0, device=dev))
    u, y = out["u"].view(-1)[:12].view(3, 4), out["y"][:3]
    x17 = torch.randn(17, 96, device=dev)
    ids17 = torch.zeros(17, dtype=torch.int32, device=dev)
    a5 = torch.randn(F.R, 5, 96, device=dev)
    b5 = torch.randn(F.R, 160, 5, device=dev)
    off = F.OFFSET + case["na"] + 1  # one float past an aligned offset
    b_mis = rows[:, off:off + 160 * 4].view(F.R, 160, 4)
    calls = [
        ("T = 17 (shrink)", lambda: D.lora_rows_u(x17, a, ids17, out["u"].view(-1)[:68].view(17, 4))),
        ("T = 17 (expand)", lambda: D.lin_rows(x17, w, out["y"], lora=(out["u"].view(-1)[:68].view(17, 4), b, ids17, 2.0))),
        ("rank 5 (shrink)", lambda: D.lora_rows_u(x, a5, ids, out["u"].view(-1)[:15].view(3, 5))),
        ("rank 5 (expand)", lambda: D.lin_rows(x, w, y, lora=(out["u"].view(-1)[:15].view(3, 5), b5, ids, 2.0))),
        ("misaligned B", lambda: D.lin_rows(x, w, y, lora=(u, b_mis, ids, 2.0))),
        ("int64 ids (shrink)", lambda: D.lora_rows_u(x, a, ids.long(), u)),
        ("int64 ids (expand)", lambda: D.lin_rows(x, w, y, lora=(u, b, ids.long(), 2.0))),
    ]
    return calls, out


def test_bad_arguments_raise():
    calls, out = bad_argument_calls()
    for label, call in calls:
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{label} was accepted")
    assert bool((out["u"] == 7).all()) and bool((out["y"] == 7).all())


# ------------------------------------------------------------------------------ the whole model
@pytest.mark.parametrize("name", ["A", "B"])
def test_fixture_adapters_change_the_tokens(name):
    """Each sequence's float64 greedy tokens under its own adapter differ from those under every
    other choice in at least half the positions: the model tests cannot pass on the base model."""
    s = F.setup(name)
    for b, k in enumerate(F.IDS):
        for j, other in s["alt"][b].items():
            if j != k:
                diff = sum(x != y for x, y in zip(s["toks"][b], other))
                print(f"config {name} sequence {b}: adapter {k} against {j}: {diff} of {F.STEPS} tokens differ")
                assert 2 * diff >= F.STEPS
    ties = sum(O.exempt64(s["logs"][b][i]) for b in range(len(F.IDS)) for i in range(F.STEPS))
    print(f"config {name}: {ties} near ties of {len(F.IDS) * F.STEPS} steps")


def check_generate_against_merge(name, dev="cpu"):
    """``generate(adapters=bank, adapter_ids=[k] * B)`` against ``merge_lora(row k)`` + ``generate``:
    logits within 1e-4 relative while the prefixes agree, tokens equal except at float64 near ties."""
    s = F.setup(name)
    m, ad, rows = F.model_with_adapters(name, dev)
    x = s["prompts"].to(dev)
    B = len(F.PLENS)
    kw = dict(max_new_tokens=F.STEPS, return_logits=True)
    for k in range(F.R):
        bank = adapter_bank(m, rows)
        tb, lb = m.generate(x, F.PLENS, adapters=bank, adapter_ids=[k] * B, **kw)
        merge_lora(m, rows[k])
        try:
            with pytest.raises(RuntimeError):
                adapter_bank(m, rows)
            with pytest.raises(RuntimeError):
                m.generate(x, F.PLENS, adapters=bank, adapter_ids=[k] * B, **kw)
            tm, lm = m.generate(x, F.PLENS, **kw)
        finally:
            unmerge_lora(m)
        tb, lb, tm, lm = tb.cpu(), lb.cpu(), tm.cpu(), lm.cpu()
        worst = 0.0
        for b, n in enumerate(F.PLENS):
            seq = s["prompts"][b, :n].tolist()
            for i in range(F.STEPS):
                worst = max(worst, _rel(lb[b, i], lm[b, i]))
                if int(tb[b, i]) != int(tm[b, i]):
                    assert O.exempt64(O.last_logits64(s["twins"][k], seq)), (name, k, b, i)
                    break  # past a near tie the two runs continue different prefixes
                seq.append(int(tb[b, i]))
        print(f"config {name} adapter {k} on {dev}: worst relative logit difference to the merged run {worst:.2e}")
        assert worst < 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_generate_with_adapters_matches_merged_generate(name):
    check_generate_against_merge(name)


def test_mixed_ids_match_the_float64_twins_and_leave_the_base_alone():
    s = F.setup("A")
    m, ad, rows = F.model_with_adapters("A")
    bank = adapter_bank(m, rows)
    base = m.generate(s["prompts"], F.PLENS, max_new_tokens=F.STEPS, return_logits=True)
    toks, logits = m.generate(s["prompts"], F.PLENS, max_new_tokens=F.STEPS, return_logits=True, adapters=bank,
                              adapter_ids=torch.tensor(F.IDS))
    exempt, bad = F.judge_tokens(s, toks.tolist())
    print(f"{exempt} exempt, {bad} wrong of {len(F.IDS) * F.STEPS}")
    assert bad == 0 and exempt <= 0.05 * len(F.IDS) * F.STEPS
    for b, k in enumerate(F.IDS):
        if toks[b].tolist() == s["toks"][b]:  # the oracle's own prefix: its logits apply
            assert max(_rel(logits[b, i], s["logs"][b][i]) for i in range(F.STEPS)) < 1e-4
        if k < 0:
            assert torch.equal(logits[b], base[1][b])
    # a model with adapters attached and no ``adapters`` argument generates the base model's text
    assert base[0][0].tolist() == s["alt"][0][-1]


def test_adapter_arguments_are_checked_on_the_host():
    s = F.setup("A")
    m, ad, rows = F.model_with_adapters("A")
    bank = adapter_bank(m, rows)
    kw = dict(max_new_tokens=2, adapters=bank)
    for ids in ([0, 1, 2, 3], [0, 1, -2, 0], [0, 1], None):
        with pytest.raises(ValueError):
            m.generate(s["prompts"], F.PLENS, adapter_ids=ids, **kw)
    with pytest.raises(ValueError):
        m.generate(s["prompts"], F.PLENS, max_new_tokens=2, adapter_ids=F.IDS)
    with pytest.raises(ValueError):
        adapter_bank(m, rows[:, :-4])
    other, _, _ = F.model_with_adapters("A")
    with pytest.raises(ValueError):
        other.generate(s["prompts"], F.PLENS, adapter_ids=F.IDS, **kw)
    cache = KVCache(m, 4, 48)
    assert cache.aid.tolist() == [-1] * 4 and cache.aid.dtype == torch.int32 and cache.u.shape == (4, 16)


def test_frozen_a_bank_shares_one_a():
    m, ad, rows = F.model_with_adapters("A", freeze_a=True)
    bank = adapter_bank(m, rows)
    a, b = bank.pair(0, "wqkv")
    assert a.stride(0) == 0 and a.shape == (F.R, F.RANK, 96) and b.shape == (F.R, 288, F.RANK)
    prompts = F.setup("A")["prompts"]
    toks, logits = m.generate(prompts, F.PLENS, max_new_tokens=4, return_logits=True, adapters=bank,
                              adapter_ids=[1, 1, 1, 1])
    merge_lora(m, rows[1])
    try:
        tm, lm = m.generate(prompts, F.PLENS, max_new_tokens=4, return_logits=True)
    finally:
        unmerge_lora(m)
    assert _rel(logits[:, 0], lm[:, 0]) < 1e-4


# ------------------------------------------------------------------------------------- FedLoRA
def test_fedlora_samples_every_client_without_merging(tmp_path):
    from ddl25spring_amd.fl.lora import FedLoRA, FedLoRAConfig
    from ddl25spring_amd.runtime.dist import DistContext
    kw = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=2, ctx_size=16, clients=4, client_fraction=0.75,
              slots=2, local_steps=2, batch_size=2, lr=1e-2, rounds=1, lora_rank=4, lora_alpha=8.0, dialects=2,
              sub_vocab=64, branching=4, eval_batches=1, pretrain_iters=5)
    ctx = DistContext(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="sample_adapters"):
        FedLoRA(FedLoRAConfig(sample_adapters="all", **kw), ctx)
    ref = FedLoRA(FedLoRAConfig(**kw), ctx)
    ref.run()
    eng = FedLoRA(FedLoRAConfig(sample_adapters="clients", **kw), ctx)
    eng.run()
    strip = lambda recs: [{k: v for k, v in r.items() if k != "round_time"} for r in recs]  # noqa: E731
    assert strip(eng.records) == strip(ref.records) and torch.equal(eng.global_row, ref.global_row)
    g0 = eng.global_row.clone()
    base_w = [blk.wqkv.detach().clone() for blk in eng.model.blocks()]
    samples = eng.sample(5, 4)
    clients = eng.records[-1]["clients"]
    assert len(clients) == 3 and len(samples) == 3 * len(clients)
    assert [(s["client"], s["adapter"]) for s in samples] == \
        [(c, a) for c in clients for a in ("base", "global", "client")]
    for s in samples:
        assert s["dialect"] == s["client"] % 2 and len(s["tokens"]) == 5 and all(0 <= t < 96 for t in s["tokens"])
    assert not eng.adapters.merged and torch.equal(eng.global_row, g0)
    assert all(torch.equal(blk.wqkv, w) for blk, w in zip(eng.model.blocks(), base_w))
    # the labels mean what they say: each continuation is the merged model's
    for s in samples:
        j = clients.index(s["client"])
        row = {"base": None, "global": eng.global_row, "client": eng.client_rows[j]}[s["adapter"]]
        prompt = eng.heldout_batch(s["dialect"], 1)[j % 2, :4][None]
        if row is not None:
            merge_lora(eng.model, row)
        try:
            want, wl = eng.model.generate(prompt, max_new_tokens=5, return_logits=True)
        finally:
            if row is not None:
                unmerge_lora(eng.model)
        top = torch.topk(wl[0], 2).values
        if bool(((top[:, 0] - top[:, 1]) > 1e-3 * wl[0].abs().amax(-1)).all()):
            assert s["tokens"] == want[0].tolist(), s
    assert ref.sample(5, 4) and isinstance(ref.sample(5, 4)[0], list)


def test_cli_sample_adapters_clients(tmp_path):
    import json
    from ddl25spring_amd.cli import main
    out = tmp_path / "run.jsonl"
    kw = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=2, ctx_size=16, clients=2, slots=2, local_steps=1,
              batch_size=2, lora_rank=4, dialects=2, sub_vocab=64, branching=4, eval_batches=1, pretrain_iters=2)
    args = ["--device", "cpu", "fedlora", "--jsonl", str(out), "--rounds", "1", "--sample-tokens", "3",
            "--sample-prompt-len", "4", "--sample-adapters", "clients"]
    for k, v in kw.items():
        args += ["--" + k.replace("_", "-"), str(v)]
    assert main(args) == 0
    recs = [json.loads(line) for line in out.read_text().splitlines()]
    samples = recs[-1]["samples"]
    assert len(samples) == 6
    assert all(set(s) == {"client", "dialect", "adapter", "tokens"} for s in samples)
    assert {s["adapter"] for s in samples} == {"base", "global", "client"}
