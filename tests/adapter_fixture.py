"""Shared inputs of tests/test_adapter_generate_cpu.py and tests/test_adapter_generate_gpu.py: the op
cases of the per-sequence adapter kernels, and two small models with three random adapters, their
merged float64 twins and the twins' greedy continuations. Everything is built once on the CPU, shared,
and never modified (the tests copy what they change)."""
import functools

import torch

import decode_oracle as O
import lora_decode_oracle as LO
from ddl25spring_amd.models.llama import LLama
from ddl25spring_amd.models.lora import LoRAConfig, attach_lora

# (T, C, K, r, prologue, residual); the last one is the wide column layout (K > 4096) with a ragged tail
OP_CASES = [(1, 288, 864, 8, "rmsnorm", False), (3, 96, 160, 4, "none", True), (16, 768, 288, 16, "swiglu", True),
            (5, 100, 52, 8, "rmsnorm", False), (2, 96, 4100, 8, "none", False)]
R = 3
OFFSET = 68  # floats: the adapters start at a non-zero, 16-byte aligned offset of their [R, P] rows


def _mixed_ids(T):
    """Every slot where T allows, exactly one -1 (the last row when T > 1)."""
    ids = [(2 * t + 1) % R for t in range(T)]
    ids[-1] = -1
    if T == 1:
        ids = [2]
    return ids


@functools.lru_cache(None)
def op_case(T, C, K, r, pro, res):
    """CPU operands of one case: x, w, residual, gain, the [R, P] rows with the views A [R, r, C],
    B [R, K, r] into them, one shared A for the stride-0 variant, and the ids."""
    g = torch.Generator().manual_seed(1000 * T + C + K + r)
    x = torch.randn(T, 2 * C if pro == "swiglu" else C, generator=g)
    w = torch.randn(K, C, generator=g) * 0.05
    resid = torch.randn(T, K, generator=g) if res else None
    gain = torch.rand(C, generator=g) + 0.5 if pro == "rmsnorm" else None
    na, nb = (r * C + 63) // 64 * 64, (K * r + 63) // 64 * 64
    rows = torch.zeros(R, OFFSET + na + nb + 60)
    rows[:, OFFSET:OFFSET + r * C] = torch.randn(R, r * C, generator=g) / C ** 0.5
    rows[:, OFFSET + na:OFFSET + na + K * r] = torch.randn(R, K * r, generator=g) * 0.05
    ids = _mixed_ids(T)
    return dict(x=x, w=w, res=resid, gain=gain, rows=rows, ids=ids, na=na, dims=(T, C, K, r), pro=pro)


def views(rows, case):
    """(A [R, r, C], B [R, K, r], shared A [R, r, C] of slot stride 0) as views of ``rows``."""
    T, C, K, r = case["dims"]
    a = rows[:, OFFSET:OFFSET + r * C].view(R, r, C)
    b = rows[:, OFFSET + case["na"]:OFFSET + case["na"] + K * r].view(R, K, r)
    return a, b, a[1].unsqueeze(0).expand(R, r, C)


# --------------------------------------------------------------------------------- the models
CFG_A = dict(vocab_size=512, dmodel=96, num_heads=2, n_layers=2, ctx_size=64)
CFG_B = dict(vocab_size=2048, dmodel=96, num_heads=6, n_layers=2, ctx_size=200)
PLENS, IDS, STEPS, RANK, ALPHA = [1, 17, 40, 9], [0, 2, -1, 1], 24, 8, 16.0


def base_model(name):
    """The seeded fp32 base (wqkv x 8 so the attention is not near-uniform) and the prompts."""
    cfg = dict(A=CFG_A, B=CFG_B)[name]
    torch.manual_seed(0)
    m = LLama(**cfg)
    with torch.no_grad():
        for blk in m.blocks():
            blk.wqkv.mul_(8)
    prompts = torch.randint(0, cfg["vocab_size"], (len(PLENS), max(PLENS)))
    return m, prompts


def adapted(m, freeze_a=False):
    """``attach_lora`` + the optimizer rows filled with the three adapters of ``Generator(1)``:
    A ~ N(0, 1 / D), B ~ N(0, 0.05^2). -> (adapters, rows [3, P])."""
    ad = attach_lora(m, R, LoRAConfig(rank=RANK, alpha=ALPHA, freeze_a=freeze_a), seed=0)
    opt = ad.make_optimizer()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k in range(R):
            for n, v in ad.row_views(opt.data[k]).items():
                D = v.shape[1]
                v.copy_(torch.randn(v.shape, generator=g) * (1.0 / D ** 0.5 if n.endswith(".A") else 0.05))
    return ad, opt.data


def model_with_adapters(name, device="cpu", freeze_a=False):
    """A fresh copy of the fixture's model on ``device`` with its three adapters -> (m, ad, rows)."""
    m, _ = base_model(name)
    m = m.to(device)
    ad, rows = adapted(m, freeze_a)
    return m, ad, rows


def twin64(name, m, ad, row):
    """The float64 model with ``row``'s adapter merged in float64 (``row`` None: the base)."""
    m64 = LLama(**dict(A=CFG_A, B=CFG_B)[name]).double()
    m64.load_state_dict({k: v.detach().double() for k, v in m.state_dict().items()})
    if row is not None:
        with torch.no_grad():
            for i, blk in enumerate(m64.blocks()):
                for t in ad.cfg.targets:
                    a, b = ad.pair(row, i, t)
                    getattr(blk, t).copy_(torch.from_numpy(LO.merged64(getattr(blk, t), a, b, ad.cfg.scale)))
    return m64


def judge_tokens(s, toks, ids=None):
    """Greedy tokens [B, STEPS] of a run with adapter ids ``ids`` against the twins, as a forced
    continuation (the prefix is the run's own): -> (exempt, bad) = mismatches at float64 near ties
    (``decode_oracle.exempt64``) and elsewhere."""
    ids = IDS if ids is None else ids
    exempt = bad = 0
    for b, (n, k) in enumerate(zip(PLENS, ids)):
        seq, on_path = s["prompts"][b, :n].tolist(), ids == IDS
        for i in range(STEPS):
            lo = s["logs"][b][i] if on_path else O.last_logits64(s["twins"][k], seq)
            if int(toks[b][i]) != int(lo.argmax()):
                if O.exempt64(lo):
                    exempt += 1
                else:
                    bad += 1
                on_path = False
            seq.append(int(toks[b][i]))
    return exempt, bad


@functools.lru_cache(None)
def setup(name):
    """dict: m (fp32, adapters attached), rows [3, P], prompts, twins {-1, 0, 1, 2}, and per sequence
    the twin greedy tokens / logits under its own adapter (``toks``, ``logs``) and the tokens under
    every choice (``alt[b][k]``)."""
    m, prompts = base_model(name)
    ad, rows = adapted(m)
    twins = {k: twin64(name, m, ad, None if k < 0 else rows[k]) for k in (-1, 0, 1, 2)}
    toks, logs, alt = [], [], []
    for b, (n, k) in enumerate(zip(PLENS, IDS)):
        p = prompts[b, :n].tolist()
        per = {j: O.greedy64(twins[j], [p], STEPS) for j in twins}
        toks.append(per[k][0][0])
        logs.append(per[k][1][0])
        alt.append({j: per[j][0][0] for j in twins})
    return dict(m=m, ad=ad, rows=rows, prompts=prompts, twins=twins, toks=toks, logs=logs, alt=alt)
