"""Text generation without a GPU: the float64 oracle's own checks (tests/decode_oracle.py), the
CPU references of the generation ops against it (ops/llama_decode.py), ``LLama.generate`` on the
CPU against the full-forward argmax loop, its argument checks, and the ``sample_tokens`` option of
apps.llm."""
import copy

import numpy as np
import pytest
import torch

import decode_oracle as O
from ddl25spring_amd.apps.llm import LLMConfig, train_llm, validate
from ddl25spring_amd.models.llama import KVCache, LLama
from ddl25spring_amd.ops import autograd_ops as A
from ddl25spring_amd.ops import llama_decode as D
from ddl25spring_amd.runtime.dist import DistContext

CFG = dict(vocab_size=512, dmodel=96, num_heads=2, n_layers=2, ctx_size=64)
PLENS, STEPS = [1, 17, 40], 24


def _state(B, steps, lens=0):
    z = lambda: torch.zeros(B, dtype=torch.int32)  # noqa: E731
    return dict(next_tok=z(), out=torch.full((B, steps), -1, dtype=torch.int32), lens=z() + lens, finished=z(),
                step=z())


# ----------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("S", [1, 5, 70])
def test_oracle_decode_is_last_row_of_causal_attention(S):
    B, H, hd = 2, 3, 16
    torch.manual_seed(S)
    qkv = torch.randn(B, S + 1, 3 * H * hd, dtype=torch.float64)
    full = O.causal_attention64(qkv, H, hd)
    q, k, v = qkv.view(B, S + 1, 3, H, hd).unbind(2)
    pos = torch.arange(S)[None, :, None].expand(B, S, H)
    kc = torch.zeros(B, H, S + 4, hd, dtype=torch.float64)
    vc = torch.zeros_like(kc)
    kc[:, :, :S], vc[:, :, :S] = O.rope64(k[:, :S], pos).transpose(1, 2), v[:, :S].transpose(1, 2)
    out, kn, vn = O.attn_decode64(qkv[:, S], kc, vc, [S] * B)
    assert O.rel(out, full[:, S]) < 1e-13
    assert O.rel(kn, O.rope64(k[:, S], S)) < 1e-15 and torch.equal(vn, v[:, S])
    # a full cache: zeros, by definition
    assert bool((O.attn_decode64(qkv[:, S], kc, vc, [S + 4] * B)[0] == 0).all())
    # the oracle's training attention agrees with the library's float64 CPU path
    assert O.rel(A.causal_attention(qkv, H, hd), full) < 1e-6  # fp32 RoPE tables on that side


def test_oracle_sampler_edge_cases():
    row = torch.tensor([1.0, 3.0, 3.0, -2.0, 3.0, 0.5])
    assert O.sample64(row, 0, 0, None) == 1  # lowest index among equal maxima
    assert O.kept64(row, 2).tolist() == [False, True, True, False, False, False]  # ties by lowest index
    assert O.kept64(row, 4).tolist() == [True, True, True, False, True, False]
    assert bool(O.kept64(row, 0).all()) and bool(O.kept64(row, 6).all()) and bool(O.kept64(row, 99).all())
    keep, cdf = O.cdf64(row, 1.0, 3)
    assert abs(float(cdf[-1]) - 1) < 1e-15 and np.allclose(cdf.numpy(), [0, 1 / 3, 2 / 3, 2 / 3, 1, 1])
    assert O.sample64(row, 1.0, 3, 1e-9) == 1 and O.sample64(row, 1.0, 3, 1 / 3 + 1e-9) == 2
    assert O.sample64(row, 1.0, 3, 1.0) == 4 and O.sample64(row, 1.0, 3, 0.9) == 4
    assert O.sample64(row, 1.0, 1, 0.7) == 1  # top-1 is greedy
    cold = O.cdf64(row, 1e-3, 0)[1]
    assert abs(float(cold[1]) - 1 / 3) < 1e-12  # a low temperature leaves the maxima only


# ----------------------------------------------------------------- CPU references vs the oracle
@pytest.mark.parametrize("T,C,K,pro,res", [(1, 288, 64, "none", False), (3, 96, 160, "none", True),
                                           (16, 64, 48, "swiglu", True), (5, 100, 52, "rmsnorm", False)])
def test_lin_rows_reference(T, C, K, pro, res):
    torch.manual_seed(0)
    x = torch.randn(T, 2 * C if pro == "swiglu" else C)
    w, r, g = torch.randn(K, C) * 0.05, torch.randn(T, K), torch.rand(C) + 0.5
    out = torch.empty(T, K)
    D.lin_rows(x, w, out, r if res else None, pro, g if pro == "rmsnorm" else None)
    assert O.rel(out, O.lin_rows64(x, w, r if res else None, pro, g)) < 1e-5
    with pytest.raises(ValueError):
        D.lin_rows(x, w, out, pro="gelu")


def test_attn_decode_and_kv_append_reference():
    B, H, hd, Smax = 3, 2, 16, 40
    torch.manual_seed(1)
    qkv, kc, vc = torch.randn(B, 3 * H * hd), torch.randn(B, H, Smax, hd), torch.randn(B, H, Smax, hd)
    lens = [0, 17, 40]
    cos, sin = A.rope_tables(Smax, hd, "cpu")
    k0, v0 = kc.clone(), vc.clone()
    out = torch.full((B, H * hd), float("nan"))
    lt = torch.tensor(lens, dtype=torch.int32)
    D.attn_decode(qkv, kc, vc, lt, cos, sin, out)
    o64, k64, _ = O.attn_decode64(qkv, k0, v0, lens)
    assert O.rel(out, o64) < 1e-5 and lt.tolist() == lens
    assert O.rel(kc[1, :, 17], k64[1]) < 1e-6 and torch.equal(vc[1, :, 17], qkv.view(B, 3, H, hd)[1, 2])
    assert torch.equal(kc[2], k0[2]) and torch.equal(vc[2], v0[2]) and bool((out[2] == 0).all())
    rows = torch.arange(Smax) != 17
    assert torch.equal(kc[1][:, rows], k0[1][:, rows])
    # prefill append, clamped at the capacity
    p = torch.randn(B, 6, 3 * H * hd)
    kc2, vc2 = torch.zeros(B, H, Smax, hd), torch.zeros(B, H, Smax, hd)
    D.kv_append(p, kc2, vc2, cos, sin, 36)
    _, k, v = p.view(B, 6, 3, H, hd).unbind(2)
    want = O.rope64(k[:, :4], (36 + torch.arange(4))[None, :, None].expand(B, 4, H)).transpose(1, 2)
    assert O.rel(kc2[:, :, 36:], want) < 1e-6 and torch.equal(vc2[:, :, 36:], v[:, :4].transpose(1, 2))
    assert bool((kc2[:, :, :36] == 0).all())


@pytest.mark.parametrize("V", [50, 512])
def test_sampler_reference(V):
    torch.manual_seed(V)
    lg = torch.randn(4, V) * 3
    lg[1, V - 3] = lg[1, 7] = lg[1].max() + 1
    st = _state(4, 1)
    D.sample(lg, **st, max_len=99)
    assert st["out"][:, 0].tolist() == [O.sample64(lg[b], 0, 0, None) for b in range(4)] and st["out"][1, 0] == 7
    steps, seed = 64, 11
    u = np.stack([D.sample_uniforms(seed, s, 4) for s in range(steps)], 1).astype(np.float64)
    assert u.min() > 0 and u.max() <= 1 and len(np.unique(u)) == u.size
    for temp in (0.7, 1.5):
        for k in (0, 1, 5, 64):
            st = _state(4, steps)
            for _ in range(steps):
                D.sample(lg, **st, max_len=99, temperature=temp, top_k=k, seed=seed)
            for b in range(4):
                keep, cdf = O.cdf64(lg[b], temp, k)
                t = st["out"][b].long()
                assert bool(keep[t].all())
                lo = np.where(t.numpy() > 0, cdf[(t - 1).clamp(min=0)].numpy(), 0.0)
                assert float(np.max(np.maximum(lo - u[b], u[b] - cdf[t].numpy()))) <= 1e-5
    with pytest.raises(ValueError):
        D.sample(lg, **_state(4, 1), max_len=99, top_k=1025)
    with pytest.raises(ValueError):
        D.sample(lg, **_state(4, 1), max_len=99, temperature=-1.0)


def test_sampler_reference_frequencies():
    """The committed seed of the GPU frequency test: the same uniforms, so the same counts."""
    p = torch.tensor([0.30, 0.05, 0.20, 0.10, 0.02, 0.13, 0.15, 0.05], dtype=torch.float64)
    u = np.stack([D.sample_uniforms(2024, s, 4) for s in range(1024)], 1).astype(np.float64).reshape(-1)
    cnt = torch.bincount(torch.bucketize(torch.from_numpy(u), torch.cumsum(p, 0)).clamp(max=7), minlength=8).double()
    assert bool(((cnt - 4096 * p).abs() <= 4 * torch.sqrt(4096 * p * (1 - p))).all())


# --------------------------------------------------------------------------------- generate
def _model(scale=8.0, seed=0):
    torch.manual_seed(seed)
    m = LLama(**CFG)
    with torch.no_grad():
        for blk in m.blocks():
            blk.wqkv.mul_(scale)
    ids = torch.randint(0, CFG["vocab_size"], (len(PLENS), max(PLENS)))
    return m, ids


def test_generate_cpu_matches_full_forward_loop():
    m, ids = _model()
    m64 = copy.deepcopy(m).double()
    toks, logits = m.generate(ids, PLENS, max_new_tokens=STEPS, return_logits=True)
    assert toks.shape == (3, STEPS) and toks.dtype == torch.int64 and logits.shape == (3, STEPS, 512)
    assert torch.equal(toks, m.generate(ids, torch.tensor(PLENS), max_new_tokens=STEPS, fused=False))
    exempt = 0
    for b, n in enumerate(PLENS):  # ragged prompts: every sequence against its own un-padded forward
        seq = ids[b, :n].tolist()
        for i in range(STEPS):
            with torch.no_grad():
                row = m(torch.tensor([seq]))[0, -1]
            assert O.rel(logits[b, i], row) < 1e-4
            if int(toks[b, i]) != int(row.argmax()):
                assert O.exempt64(O.last_logits64(m64, seq)), (b, i)
                exempt += 1
            seq.append(int(toks[b, i]))
    assert exempt <= 0.05 * 3 * STEPS


def test_generate_sampling_is_a_function_of_the_seed():
    m, ids = _model()
    kw = dict(max_new_tokens=12, temperature=0.8, top_k=20)
    a, b, c = (m.generate(ids, PLENS, seed=s, **kw) for s in (7, 7, 8))
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_generate_eos_cpu():
    m, ids = _model()
    base = m.generate(ids, PLENS, max_new_tokens=STEPS)
    eos = int(base[1, 5])
    cache = KVCache(m, 3, max(PLENS) + STEPS)
    got = m.generate(ids, PLENS, max_new_tokens=STEPS, eos_id=eos, cache=cache)
    for b in range(3):
        row = base[b].tolist()
        if eos in row:
            cut = row.index(eos)
            assert got[b].tolist() == row[:cut + 1] + [eos] * (STEPS - cut - 1)
            assert int(cache.lens[b]) == PLENS[b] + cut
        else:
            assert got[b].tolist() == row and int(cache.lens[b]) == PLENS[b] + STEPS - 1
    assert int(cache.finished[1]) == 1


def test_generate_argument_checks():
    m, ids = _model()
    with pytest.raises(ValueError, match="ctx_size"):
        m.generate(ids, PLENS, max_new_tokens=25)  # 40 + 25 > 64
    m.generate(ids, PLENS, max_new_tokens=2)
    bad = ids.clone()
    bad[0, 0] = 512
    with pytest.raises(ValueError, match="token"):
        m.generate(bad, PLENS, max_new_tokens=2)
    bad[0, 0] = -1
    with pytest.raises(ValueError, match="token"):
        m.generate(bad, PLENS, max_new_tokens=2)
    with pytest.raises(ValueError):
        m.generate(ids, [1, 17, 41], max_new_tokens=2)
    with pytest.raises(ValueError):
        m.generate(ids, PLENS, max_new_tokens=2, top_k=2000, temperature=1.0)
    with pytest.raises(ValueError):
        KVCache(m, 3, 65)
    with pytest.raises(NotImplementedError):
        LLama(precision="bf16", **CFG).generate(ids, PLENS, max_new_tokens=2)
    from ddl25spring_amd.parallel.tp import TPHandle, shard_llama
    sharded = shard_llama(copy.deepcopy(m), 2, 0, TPHandle(DistContext(), None, 2, 0))
    with pytest.raises(NotImplementedError):
        sharded.generate(ids, PLENS, max_new_tokens=2)


# --------------------------------------------------------------------------------- apps.llm
TINY = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=2, ctx_size=16, batch_size=4, iters=2, log_every=1)


def test_train_llm_sample_tokens():
    plain = train_llm(LLMConfig(**TINY), DistContext(), log=None)
    assert sorted(plain) == ["config", "losses", "ms_per_iter", "resumed_from", "seconds", "tokens_per_s"]
    lines = []
    out = train_llm(LLMConfig(sample_tokens=8, sample_prompt_len=4, **TINY), DistContext(), log=lines.append)
    assert sorted(set(out) - set(plain)) == ["samples"]
    s = out["samples"]
    assert len(s) == 4 and all(len(r) == 8 and all(isinstance(t, int) and 0 <= t < 96 for t in r) for r in s)
    assert any("sample" in ln for ln in lines)
    assert [v for _, v in out["losses"]] == [v for _, v in plain["losses"]]


def test_validate_rejects_sampling_across_ranks():
    with pytest.raises(ValueError, match="sample_tokens"):
        validate(LLMConfig(sample_tokens=8, pp=2), 2)
    with pytest.raises(ValueError, match="sample_tokens"):
        validate(LLMConfig(sample_tokens=8, tp=2), 2)
    with pytest.raises(ValueError, match="sample_tokens"):
        validate(LLMConfig(sample_tokens=8, precision="bf16"), 1)
    with pytest.raises(ValueError, match="sample_tokens"):
        validate(LLMConfig(sample_tokens=8, sample_prompt_len=250), 1)
    validate(LLMConfig(sample_tokens=8), 1)
