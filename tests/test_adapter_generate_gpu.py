"""Per-sequence LoRA adapters in generation, on the device: ddl_lora_rows_u and ddl_lin_rows_lora_f32
(csrc/kernels/llama_decode.hip) against the float64 oracle and its derived bound
(tests/lora_decode_oracle.py), and prefill / decode_step / generate with an adapter bank against
the merged float64 twins of tests/adapter_fixture.py. Whole-model tolerance: 1e-4 relative, as
test_generate_gpu.py."""
import pytest
import torch

import adapter_fixture as F
import decode_oracle as O
import test_adapter_generate_cpu as C
from ddl25spring_amd.models.llama import KVCache
from ddl25spring_amd.models.lora import adapter_bank
from ddl25spring_amd.ops import llama_decode as D

pytestmark = pytest.mark.gpu
_rel = O.rel


# -------------------------------------------------------------------------------------- the ops
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("args", F.OP_CASES)
def test_kernels_meet_the_oracle_bound(cuda, args, shared):
    C.check_case(args, shared, cuda)


def test_bad_arguments_are_refused_without_a_launch(cuda):
    calls, out = C.bad_argument_calls(cuda)
    for label, call in calls:
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{label} was accepted")
    # the launchers themselves: a non-zero return code, nothing launched
    case = F.op_case(*F.OP_CASES[1])
    rows = case["rows"].to(cuda)
    a, b, _ = F.views(rows, case)
    x, w = case["x"].to(cuda), case["w"].to(cuda)
    ids = torch.tensor([0, 1, -1], dtype=torch.int32, device=cuda)
    u, y = out["u"].view(-1)[:12].view(3, 4), out["y"][:3]
    x17, ids17 = torch.randn(17, 96, device=cuda), torch.zeros(17, dtype=torch.int32, device=cuda)
    off = F.OFFSET + case["na"] + 1
    b_mis = rows[:, off:off + 160 * 4].view(F.R, 160, 4)
    assert D.lora_rows_u_launch(x17, a, ids17, out["u"], T=17) != 0
    assert D.lora_rows_u_launch(x, a, ids, u, rank=5) != 0
    assert D.lora_rows_u_launch(x, a, None, u) != 0
    assert D.lin_rows_launch(x17, w, out["y"], T=17, lora=(out["u"], b, ids17, 2.0)) != 0
    assert D.lin_rows_launch(x, w, y, lora=(u, b, ids, 2.0), rank=5) != 0
    assert D.lin_rows_launch(x, w, y, lora=(u, b_mis, ids, 2.0)) != 0
    assert D.lin_rows_launch(x, w, y, lora=(u, b, None, 2.0)) != 0
    torch.cuda.synchronize()
    assert bool((out["u"] == 7).all()) and bool((out["y"] == 7).all())


# ------------------------------------------------------------------------------ the whole model
def _forced(m, prompts, toks, cuda, fused, bank=None, ids=None):
    """Prefill, then the oracle's tokens forced through decode_step -> logits [STEPS + 1][B, V]."""
    cache = KVCache(m, len(F.PLENS), max(F.PLENS) + F.STEPS)
    kw = {} if bank is None else dict(adapters=bank)
    got = [m.prefill(prompts, F.PLENS, cache, adapter_ids=ids, **kw).cpu()]
    for i in range(F.STEPS):
        got.append(m.decode_step(cache, torch.tensor([t[i] for t in toks]), fused=fused, **kw).cpu())
    assert cache.lens.tolist() == [n + F.STEPS for n in F.PLENS]
    return got


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["A", "B"])
def test_forced_decoding_matches_the_merged_float64_twins(cuda, name, fused):
    s = F.setup(name)
    m, ad, rows = F.model_with_adapters(name, cuda)
    x = s["prompts"].to(cuda)
    got = _forced(m, x, s["toks"], cuda, fused, adapter_bank(m, rows), F.IDS)
    plain = _forced(m, x, s["toks"], cuda, fused)
    worst = max(_rel(got[i][b], s["logs"][b][i]) for i in range(F.STEPS + 1) for b in range(len(F.IDS)))
    print(f"config {name} fused={fused}: worst relative logit error against the merged twins {worst:.2e}")
    assert worst < 1e-4
    for b, k in enumerate(F.IDS):
        same = all(torch.equal(got[i][b], plain[i][b]) for i in range(F.STEPS + 1))
        assert same == (k < 0), (b, k)


@pytest.mark.parametrize("name", ["A", "B"])
def test_generate_greedy_matches_the_twins(cuda, name):
    s = F.setup(name)
    m, ad, rows = F.model_with_adapters(name, cuda)
    toks = m.generate(s["prompts"].to(cuda), F.PLENS, max_new_tokens=F.STEPS, adapters=adapter_bank(m, rows),
                      adapter_ids=F.IDS).cpu()
    exempt, bad = F.judge_tokens(s, toks.tolist())
    print(f"config {name}: {exempt} exempt, {bad} wrong of {len(F.IDS) * F.STEPS}")
    assert bad == 0 and exempt <= 0.05 * len(F.IDS) * F.STEPS


def test_graph_replay_reads_ids_and_rows_from_the_device(cuda):
    s = F.setup("A")
    m, ad, rows = F.model_with_adapters("A", cuda)
    x = s["prompts"].to(cuda)
    bank = adapter_bank(m, rows)
    kw = dict(max_new_tokens=F.STEPS, return_logits=True, adapters=bank)
    cache = KVCache(m, len(F.PLENS), max(F.PLENS) + F.STEPS)
    tg, lg = m.generate(x, F.PLENS, graph=True, adapter_ids=F.IDS, cache=cache, **kw)
    te, le = m.generate(x, F.PLENS, graph=False, adapter_ids=F.IDS, **kw)
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert len(cache._graphs) == 1
    # the same captured step under another assignment and a row rewritten in place
    ids2 = [2, -1, 1, 0]
    rows[1].copy_(rows[1].flip(0).contiguous() * 0.5 + rows[0])
    tg2, lg2 = m.generate(x, F.PLENS, graph=True, adapter_ids=ids2, cache=cache, **kw)
    te2, le2 = m.generate(x, F.PLENS, graph=False, adapter_ids=ids2, **kw)
    assert len(cache._graphs) == 1
    assert torch.equal(tg2, te2) and torch.equal(lg2, le2)
    assert not torch.equal(tg2, tg)


def test_more_than_sixteen_sequences(cuda):
    """B = 17 takes the wide path: the training linears and ``lora_fwd`` on gathered pairs."""
    s = F.setup("A")
    m, ad, rows = F.model_with_adapters("A", cuda)
    B, T, steps = 17, 5, 3
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, F.CFG_A["vocab_size"], (B, T), generator=g)
    ids = [(b % 4) - 1 for b in range(B)]
    toks, logits = m.generate(prompts.to(cuda), max_new_tokens=steps, return_logits=True,
                              adapters=adapter_bank(m, rows), adapter_ids=ids)
    toks, logits = toks.cpu(), logits.cpu()
    worst = 0.0
    for b in range(B):
        seq = prompts[b].tolist()
        for i in range(steps):  # forced: the prefix is generate's own
            worst = max(worst, _rel(logits[b, i], O.last_logits64(s["twins"][ids[b]], seq)))
            seq.append(int(toks[b, i]))
    print(f"B = 17: worst relative logit error against the merged twins {worst:.2e}")
    assert worst < 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_generate_with_adapters_matches_merged_generate(cuda, name):
    C.check_generate_against_merge(name, cuda)
