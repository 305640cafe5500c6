"""The LoRA oracle (tests/lora_oracle.py) against torch float64 autograd, its fp32 emulation against
its own bound, the CPU ops of ops/lora.py against it, and the model-level contract of
models/lora.py on the CPU."""
import numpy as np
import pytest
import torch

import lora_oracle as O
from ddl25spring_amd.ops import lora as L

# (S, T, D, N, r): the GPU suite's shapes (tests/test_lora_gpu.py) with T over the chunk boundary
SHAPES = [(1, 16, 16, 16, 4), (3, 37, 96, 288, 8), (2, 69, 288, 96, 16), (2, L.CHUNK, 96, 512, 4),
          (2, 3 * L.CHUNK + 5, 96, 512, 4)]
SCALE = 1.7


def make(shape, seed=0):
    S, T, D, N, r = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=rn(S, T, D), A=rn(S, r, D) / D ** 0.5, B=rn(S, N, r) * 0.3, y0=rn(S, T, N), dy=rn(S, T, N),
                dx0=rn(S, T, D), dA0=rn(S, r, D), dB0=rn(S, N, r))


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_oracle_matches_float64_autograd(shape):
    d = make(shape)
    x, A, B = (d[k].double().requires_grad_(True) for k in ("x", "A", "B"))
    s = O.s32(SCALE)
    y = d["y0"].double() + s * torch.bmm(torch.bmm(x, A.transpose(1, 2)), B.transpose(1, 2))
    y.backward(d["dy"].double())
    u, yq = O.fwd(d["x"], d["A"], d["B"], d["y0"], SCALE)
    v, dxq = O.bwd_x(d["dy"], d["A"], d["B"], None, SCALE)
    z = torch.zeros
    dAq, dBq = O.bwd_w(d["x"], d["dy"], u.v, v.v, z(A.shape), z(B.shape), SCALE, L.CHUNK)
    for got, want in ((yq.v, y), (dxq.v, x.grad), (dAq.v, A.grad), (dBq.v, B.grad)):
        want = want.detach().numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_and_cpu_ops_meet_the_bound(shape):
    d = make(shape, 1)
    uq, yq = O.fwd(d["x"], d["A"], d["B"], d["y0"], SCALE)
    ue, ye = O.emulate_fwd(d["x"], d["A"], d["B"], d["y0"], SCALE)
    y = d["y0"].clone()
    u = L.lora_fwd(d["x"], d["A"], d["B"], y, SCALE)
    for got in ((ue, ye), (u, y)):
        assert O.ratio(got[0], uq) <= 1.0 and O.ratio(got[1], yq) <= 1.0

    vq, dxq = O.bwd_x(d["dy"], d["A"], d["B"], d["dx0"], SCALE)
    ve, dxe = O.emulate_bwd_x(d["dy"], d["A"], d["B"], d["dx0"], SCALE)
    dx = d["dx0"].clone()
    v = L.lora_bwd_x(d["dy"], d["A"], d["B"], SCALE, dx=dx, accumulate=True)
    for got in ((ve, dxe), (v, dx)):
        assert O.ratio(got[0], vq) <= 1.0 and O.ratio(got[1], dxq) <= 1.0
    dx2 = torch.full_like(dx, 7.0)
    L.lora_bwd_x(d["dy"], d["A"], d["B"], SCALE, dx=dx2)  # not accumulating: dx0 = 0
    assert O.ratio(dx2, O.bwd_x(d["dy"], d["A"], d["B"], None, SCALE)[1]) <= 1.0

    dAq, dBq = O.bwd_w(d["x"], d["dy"], u, v, d["dA0"], d["dB0"], SCALE, L.CHUNK)
    dAe, dBe = O.emulate_bwd_w(d["x"], d["dy"], u, v, d["dA0"], d["dB0"], SCALE, L.CHUNK)
    dA, dB = d["dA0"].clone(), d["dB0"].clone()
    L.lora_bwd_w(d["x"], d["dy"], u, v, dA, dB, SCALE)
    for got in ((dAe, dBe), (dA, dB)):
        assert O.ratio(got[0], dAq) <= 1.0 and O.ratio(got[1], dBq) <= 1.0
    dB2 = d["dB0"].clone()
    L.lora_bwd_w(d["x"], d["dy"], u, None, None, dB2, SCALE)  # A frozen
    assert torch.equal(dB2, dB)


def test_bound_is_tight_enough_to_catch_a_wrong_scale():
    """A result off by one part in 10^4 (a wrong scale, a dropped term) is far outside the bound."""
    d = make(SHAPES[1], 2)
    _, yq = O.fwd(d["x"], d["A"], d["B"], d["y0"], SCALE)
    _, ye = O.emulate_fwd(d["x"], d["A"], d["B"], d["y0"], SCALE * (1 + 1e-4))
    assert O.ratio(ye, yq) > 1.0


BAD = [dict(r=5), dict(r=32), dict(D=24), dict(N=40), dict(D=0)]


@pytest.mark.parametrize("bad", BAD)
def test_unsupported_shapes_raise(bad):
    S, T, D, N, r = 2, 8, 32, 48, 4
    D, N, r = bad.get("D", D), bad.get("N", N), bad.get("r", r)
    x, A, B, y = torch.zeros(S, T, D), torch.zeros(S, r, D), torch.zeros(S, N, r), torch.zeros(S, T, N)
    with pytest.raises(ValueError):
        L.lora_fwd(x, A, B, y, 1.0)
    with pytest.raises(ValueError):
        L.lora_bwd_x(y, A, B, 1.0)
    with pytest.raises(ValueError):
        L.lora_bwd_w(x, y, torch.zeros(S, T, r), torch.zeros(S, T, r), torch.zeros_like(A), torch.zeros_like(B), 1.0)


def test_operand_layout_is_checked():
    S, T, D, N, r = 2, 8, 32, 48, 4
    x, A, B, y = torch.zeros(S, T, D), torch.zeros(S, r, D), torch.zeros(S, N, r), torch.zeros(S, T, N)
    with pytest.raises(ValueError):
        L.lora_fwd(x.transpose(0, 1).contiguous().transpose(0, 1), A, B, y, 1.0)  # x not contiguous
    with pytest.raises(ValueError):
        L.lora_fwd(x, A.double(), B, y, 1.0)
    with pytest.raises(ValueError):
        L.lora_fwd(x, torch.zeros(S, D, r).transpose(1, 2), B, y, 1.0)  # A not packed inside a slot
    with pytest.raises(ValueError):
        L.lora_fwd(x, A, B, torch.zeros(S, T + 1, N), 1.0)


# ------------------------------------------------------------------------------------ model level
CFG = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=2, ctx_size=16)


def _model(seed=0):
    from ddl25spring_amd.models.llama import LLama
    torch.manual_seed(seed)
    return LLama(**CFG)


def _randomise_b(ad, seed=3, std=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ad.named.items():
            if n.endswith(".B"):
                p.copy_(torch.randn(p.shape, generator=g) * std)


def test_attach_freezes_base_and_fresh_adapters_change_no_bit():
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    m = _model()
    x = torch.randint(3, 96, (4, 16))
    base = m(x).detach().clone()
    ad = attach_lora(m, 2, LoRAConfig(rank=4, alpha=8.0), seed=1)
    assert not any(p.requires_grad for p in m.parameters())
    assert all(torch.equal(p[0], p[1]) for p in ad.parameters())  # the same init in every slot
    a = ad.named["0.wqkv.A"]
    assert abs(a.std().item() - 32 ** -0.5) < 0.05 and not ad.named["0.wqkv.B"].any()
    assert torch.equal(m(x), base)
    with pytest.raises(ValueError):
        m(x[:3])  # not slot-major over 2 slots


def test_model_step_matches_float64_merged_weights():
    """One fwd + bwd with per-slot adapters against float64 torch on W + scale B A per slot."""
    import copy

    from ddl25spring_amd.models.llama import causalLLMLoss
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    S, b = 2, 2
    m = _model()
    m64 = copy.deepcopy(m).double()
    cfg = LoRAConfig(rank=4, alpha=8.0)
    ad = attach_lora(m, S, cfg, seed=1)
    opt = ad.make_optimizer(lr=1e-2)
    _randomise_b(ad)
    x = torch.randint(3, 96, (S * b, 16))
    opt.zero_grad()
    loss = causalLLMLoss(m(x), x, scale=float(S))
    loss.backward()
    assert all(p.grad is None for p in m.parameters())
    want_loss, grads = 0.0, {}
    for s in range(S):
        ms = copy.deepcopy(m64)
        leaves = {}
        for i, blk in enumerate(ms.blocks()):
            for t in cfg.targets:
                A = ad.named[f"{i}.{t}.A"].detach()[s].double().requires_grad_(True)
                B = ad.named[f"{i}.{t}.B"].detach()[s].double().requires_grad_(True)
                leaves[f"{i}.{t}.A"], leaves[f"{i}.{t}.B"] = A, B
                w = getattr(blk, t).detach()
                delattr(blk, t)
                setattr(blk, t, w + cfg.scale * B @ A)
        ls = causalLLMLoss(ms(x[s * b:(s + 1) * b]), x[s * b:(s + 1) * b])
        ls.backward()
        want_loss += ls.item()
        grads[s] = {n: v.grad for n, v in leaves.items()}
    assert abs(loss.item() - want_loss) < 1e-5 * abs(want_loss)
    for n, p in ad.named.items():
        for s in range(S):
            g, w = p.grad[s].double(), grads[s][n]
            assert ((g - w).norm() / w.norm()).item() < 1e-4, (n, s)


def test_merge_unmerge_and_state_dict():
    from ddl25spring_amd.models.lora import (LoRAConfig, attach_lora, load_lora_state_dict, lora_state_dict,
                                             merge_lora, unmerge_lora)
    m = _model()
    ad = attach_lora(m, 2, LoRAConfig(rank=4, alpha=8.0), seed=1)
    opt = ad.make_optimizer()
    _randomise_b(ad)
    x = torch.randint(3, 96, (2, 16))
    with torch.no_grad():
        want = m(torch.cat([x, x]))[2:]  # slot 1's adapter on x
    w0 = [p.detach().clone() for p in m.parameters()]
    merge_lora(m, opt.data[1])
    with pytest.raises(RuntimeError):
        merge_lora(m, opt.data[1])
    with torch.no_grad():
        got = m(x)  # any batch size: the merged model is a plain model
    assert ((got - want).norm() / want.norm()).item() < 1e-5
    assert m.generate(x[:, :4], max_new_tokens=3).shape == (2, 3)
    unmerge_lora(m)
    assert all(torch.equal(a, b) for a, b in zip(w0, m.parameters()))
    sd = lora_state_dict(m, opt.data[1])
    assert set(sd) == set(ad.named) and sd["0.wo.B"].shape == (32, 4)
    load_lora_state_dict(m, sd, opt.data[0])
    assert torch.equal(opt.data[0], opt.data[1])
    bad = dict(sd)
    bad.pop("0.wo.B")
    with pytest.raises(KeyError):
        load_lora_state_dict(m, bad)


def test_freeze_a_keeps_a_out_of_the_rows():
    from ddl25spring_amd.models.llama import causalLLMLoss
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    m = _model()
    ad = attach_lora(m, 2, LoRAConfig(rank=4, alpha=8.0, freeze_a=True), seed=1)
    opt = ad.make_optimizer()
    assert all(n.endswith(".B") for n, _ in ad.trainable())
    a0 = ad.named["1.w2.A"].detach().clone()
    _randomise_b(ad)
    x = torch.randint(3, 96, (4, 16))
    for _ in range(2):
        opt.zero_grad()
        causalLLMLoss(m(x), x).backward()
        opt.step()
    assert torch.equal(ad.named["1.w2.A"], a0) and ad.named["1.w2.A"].grad is None


def test_unsupported_models_are_refused():
    from ddl25spring_amd.models.llama import LLama, LLamaStage
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    with pytest.raises(NotImplementedError, match="fp32"):
        attach_lora(LLama(precision="bf16", **CFG), 2)
    with pytest.raises(NotImplementedError, match="pipeline"):
        attach_lora(LLamaStage(dmodel=32, num_heads=2, n_layers=1, ctx_size=16), 2)
    m = _model()
    m.blocks()[0].tp = object()
    with pytest.raises(NotImplementedError, match="tensor-parallel"):
        attach_lora(m, 2)
    with pytest.raises(ValueError):
        attach_lora(_model(), 2, LoRAConfig(rank=5))


def test_slot_adam_reset_state():
    from ddl25spring_amd.optim import SlotAdam
    p = torch.nn.Parameter(torch.ones(3, 5))
    opt = SlotAdam([p], 3, lr=0.1)
    opt.grad.fill_(1.0)
    opt.step()
    first = p.detach().clone()
    opt.step()
    opt.reset_state(2)
    assert not opt.m[:2].any() and not opt.v[:2].any() and opt.t == [0, 0, 2] and opt.m[2].any()
    with torch.no_grad():
        p.fill_(1.0)
    opt.step(rows=2)
    assert torch.equal(p[:2], first[:2])  # a fresh Adam's first step again
