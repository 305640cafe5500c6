"""The LoRA kernels (csrc/kernels/lora.hip) against the float64 oracle within its derived bound
(tests/lora_oracle.py), their memory discipline and determinism, and the adapters in the fp32 LLaMA
and the FedLoRA engine on the device."""
import copy

import pytest
import torch

import lora_oracle as O
from ddl25spring_amd.ops import lora as L

pytestmark = pytest.mark.gpu

SCALE = 1.7
CHUNK = L.CHUNK  # tokens per reduction chunk of lora_bwd_w (LORA_CHUNK in lora.hip; ops/lora.py checks it)
# (S, T, D, N, r); the last three: inside one chunk, exactly on the chunk boundary, three chunks and a ragged tail
SHAPES = [(1, 16, 16, 16, 4), (3, 37, 96, 288, 8), (2, 69, 288, 96, 16),
          (2, CHUNK - 11, 96, 512, 4), (2, CHUNK, 96, 512, 4), (2, 3 * CHUNK + 5, 96, 512, 4)]
GUARD = 64  # floats on either side of every output
OFF = 128   # the adapters' offset inside the wide [S, P] buffer (a multiple of 64 floats, not 0)


def make(shape, seed=0):
    S, T, D, N, r = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=rn(S, T, D), A=rn(S, r, D) / D ** 0.5, B=rn(S, N, r) * 0.3, y0=rn(S, T, N), dy=rn(S, T, N),
                dx0=rn(S, T, D), dA0=rn(S, r, D), dB0=rn(S, N, r))


class Guarded:
    """A contiguous device tensor with GUARD floats of a sentinel on either side."""
    SENTINEL = -1234.5

    def __init__(self, init, dev):
        n = init.numel()
        self.buf = torch.full((n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)

    def intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        return bool((g == self.SENTINEL).all())


class Rows:
    """A and B (or dA and dB) of every slot as views of a wide [S, P] buffer, as SlotAdam lays them
    out: A at OFF, B after it at the next multiple of 64; everything else is sentinel."""
    SENTINEL = 4321.25

    def __init__(self, A, B, dev):
        S, r, D = A.shape
        N = B.shape[1]
        self.na, self.nb = r * D, N * r
        self.offb = OFF + (self.na + 63) // 64 * 64
        P = self.offb + (self.nb + 63) // 64 * 64 + 64
        self.buf = torch.full((S, P), self.SENTINEL, dtype=torch.float32, device=dev)
        self.A = self.buf[:, OFF:OFF + self.na].view(S, r, D)
        self.B = self.buf[:, self.offb:self.offb + self.nb].view(S, N, r)
        self.A.copy_(A)
        self.B.copy_(B)

    def intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[:, OFF:OFF + self.na] = False
        mask[:, self.offb:self.offb + self.nb] = False
        return bool((self.buf[mask] == self.SENTINEL).all())


def run_all(d, dev, freeze_a=False):
    """fwd, bwd_x (accumulating) and bwd_w on guarded buffers -> the outputs and the guards."""
    w, gw = Rows(d["A"], d["B"], dev), Rows(d["dA0"], d["dB0"], dev)
    assert w.A.stride(0) != w.A[0].numel() or w.A.shape[0] == 1
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    S, T, _ = x.shape
    r = d["A"].shape[1]
    y, dx = Guarded(d["y0"], dev), Guarded(d["dx0"], dev)
    u, v = Guarded(torch.zeros(S, T, r), dev), Guarded(torch.zeros(S, T, r), dev)
    L.lora_fwd_out(x, w.A, w.B, y.t, u.t, SCALE)
    L.lora_bwd_x(dy, w.A, w.B, SCALE, dx=dx.t, accumulate=True, v=v.t)
    L.lora_bwd_w(x, dy, u.t, v.t, None if freeze_a else gw.A, gw.B, SCALE)
    torch.cuda.synchronize()
    guards = all(g.intact() for g in (y, dx, u, v, w, gw))
    return dict(y=y.t, dx=dx.t, u=u.t, v=v.t, dA=gw.A, dB=gw.B), guards


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_within_the_derived_bound(cuda, shape):
    d = make(shape, 1)
    out, guards = run_all(d, cuda)
    assert guards, "a kernel wrote outside its output"
    uq, yq = O.fwd(d["x"], d["A"], d["B"], d["y0"], SCALE)
    vq, dxq = O.bwd_x(d["dy"], d["A"], d["B"], d["dx0"], SCALE)
    # bwd_w is judged on the u, v it was given (the kernels' own)
    dAq, dBq = O.bwd_w(d["x"], d["dy"], out["u"], out["v"], d["dA0"], d["dB0"], SCALE, CHUNK)
    ratios = {k: O.ratio(out[k], q) for k, q in dict(u=uq, y=yq, v=vq, dx=dxq, dA=dAq, dB=dBq).items()}
    print(shape, {k: f"{v:.3f}" for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert float(out["dA"].sub(d["dA0"].to(cuda)).abs().max()) > 0  # B != 0: dA is not trivially its old value


def test_dx_is_optional_and_overwrites_without_accumulate(cuda):
    d = make(SHAPES[1], 2)
    A, B, dy = d["A"].to(cuda), d["B"].to(cuda), d["dy"].to(cuda)
    dx = torch.full(d["dx0"].shape, 7.0, device=cuda)
    v1 = L.lora_bwd_x(dy, A, B, SCALE, dx=dx)
    v2 = L.lora_bwd_x(dy, A, B, SCALE)  # the input needs no gradient: v alone
    assert torch.equal(v1, v2)
    vq, dxq = O.bwd_x(d["dy"], d["A"], d["B"], None, SCALE)
    assert O.ratio(dx, dxq) <= 1.0 and O.ratio(v2, vq) <= 1.0


def test_slot_is_independent_of_the_batch_and_runs_are_bitwise_equal(cuda):
    d = make(SHAPES[1], 3)
    out3, _ = run_all(d, cuda)
    again, _ = run_all(d, cuda)
    one, _ = run_all({k: t[1:2].contiguous() for k, t in d.items()}, cuda)
    for k in out3:
        assert torch.equal(out3[k], again[k]), k
        assert torch.equal(out3[k][1], one[k][0]), k


def test_freeze_a_leaves_da_untouched(cuda):
    d = make(SHAPES[2], 4)
    out, guards = run_all(d, cuda, freeze_a=True)
    ref, _ = run_all(d, cuda)
    assert guards and torch.equal(out["dA"].cpu(), d["dA0"]) and torch.equal(out["dB"], ref["dB"])


@pytest.mark.parametrize("bad", [dict(r=5), dict(r=32), dict(D=24), dict(N=40)])
def test_unsupported_shapes_raise_before_a_launch(cuda, bad):
    S, T, D, N, r = 2, 8, 32, 48, 4
    D, N, r = bad.get("D", D), bad.get("N", N), bad.get("r", r)
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    y = torch.full((S, T, N), 3.0, device=cuda)
    with pytest.raises(ValueError):
        L.lora_fwd(z(S, T, D), z(S, r, D), z(S, N, r), y, 1.0)
    with pytest.raises(ValueError):
        L.lora_bwd_x(y, z(S, r, D), z(S, N, r), 1.0)
    with pytest.raises(ValueError):
        L.lora_bwd_w(z(S, T, D), y, z(S, T, r), z(S, T, r), z(S, r, D), z(S, N, r), 1.0)
    with pytest.raises(ValueError):
        L.lora_fwd(z(S, T, D), z(S, r, D), z(S, N, r)[:, :, :].transpose(1, 2).contiguous().transpose(1, 2), y, 1.0)
    assert bool((y == 3.0).all())


# ------------------------------------------------------------------------------------ model level
CFG = dict(vocab_size=512, dmodel=96, num_heads=2, n_layers=2, ctx_size=64)
S_, B_ = 2, 2


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _model(dev, seed=0):
    from ddl25spring_amd.models.llama import LLama
    torch.manual_seed(seed)
    return LLama(**CFG).to(dev)


def _randomise_b(ad, seed=3, std=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in ad.named.items():
            if n.endswith(".B"):
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))


def test_fresh_adapters_change_no_bit_of_the_logits(cuda):
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    m = _model(cuda)
    x = torch.randint(0, 512, (S_ * B_, 64), device=cuda)
    with torch.no_grad():
        base = m(x).clone()
    attach_lora(m, S_, LoRAConfig(rank=8), seed=1)
    with torch.no_grad():
        assert torch.equal(m(x), base)


def test_model_step_matches_float64_merged_weights(cuda):
    """One fwd + bwd with per-slot adapters against float64 torch on W + scale B A per slot: loss
    within 1e-5 relative, every adapter gradient within 1e-4 relative; no base gradient."""
    from ddl25spring_amd.models.llama import causalLLMLoss
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora
    m = _model(cuda)
    m64 = copy.deepcopy(m).cpu().double()
    cfg = LoRAConfig(rank=8, alpha=16.0)
    ad = attach_lora(m, S_, cfg, seed=1)
    opt = ad.make_optimizer()
    _randomise_b(ad)
    x = torch.randint(0, 512, (S_ * B_, 64))
    opt.zero_grad()
    loss = causalLLMLoss(m(x.to(cuda)), x.to(cuda), scale=float(S_))
    loss.backward()
    assert all(p.grad is None for p in m.parameters())
    want_loss, grads = 0.0, {}
    for s in range(S_):
        ms = copy.deepcopy(m64)
        leaves = {}
        for i, blk in enumerate(ms.blocks()):
            for t in cfg.targets:
                A = ad.named[f"{i}.{t}.A"].detach()[s].cpu().double().requires_grad_(True)
                B = ad.named[f"{i}.{t}.B"].detach()[s].cpu().double().requires_grad_(True)
                leaves[f"{i}.{t}.A"], leaves[f"{i}.{t}.B"] = A, B
                w = getattr(blk, t).detach()
                delattr(blk, t)
                setattr(blk, t, w + cfg.scale * B @ A)
        xs = x[s * B_:(s + 1) * B_]
        ls = causalLLMLoss(ms(xs), xs)
        ls.backward()
        want_loss += ls.item()
        grads[s] = {n: v.grad for n, v in leaves.items()}
    assert abs(loss.item() - want_loss) < 1e-5 * abs(want_loss)
    worst = 0.0
    for n, p in ad.named.items():
        for s in range(S_):
            e = _rel(p.grad[s], grads[s][n])
            worst = max(worst, e)
            assert e < 1e-4, (n, s, e)
    print(f"worst relative adapter gradient error {worst:.2e}")


def test_merge_generate_unmerge(cuda):
    """merge_lora then generate == generate on a model built with the merged weights; unmerge_lora
    restores the base bits."""
    from ddl25spring_amd.models.lora import LoRAConfig, attach_lora, merge_lora, merged_weight, unmerge_lora
    m = _model(cuda)
    cfg = LoRAConfig(rank=8, alpha=16.0)
    ad = attach_lora(m, S_, cfg, seed=1)
    opt = ad.make_optimizer()
    _randomise_b(ad, std=0.2)
    built = _model(cuda)
    with torch.no_grad():
        for i, blk in enumerate(built.blocks()):
            for t in cfg.targets:
                a, b = ad.pair(opt.data[1], i, t)
                getattr(blk, t).copy_(merged_weight(getattr(blk, t).detach(), a, b, cfg.scale))
    prompt = torch.randint(0, 512, (2, 8), device=cuda)
    w0 = [p.detach().clone() for p in m.parameters()]
    base_toks = m.generate(prompt, max_new_tokens=6, graph=False)
    merge_lora(m, opt.data[1])
    toks = m.generate(prompt, max_new_tokens=6, graph=False)
    assert torch.equal(toks, built.generate(prompt, max_new_tokens=6, graph=False))
    unmerge_lora(m)
    assert all(torch.equal(a, b) for a, b in zip(w0, m.parameters()))
    assert torch.equal(m.generate(prompt, max_new_tokens=6, graph=False), base_toks)


def test_fedlora_round_matches_the_cpu_reference_ops(cuda):
    """One round, 4 clients in 2 waves of 2 slots, on the device against the same round through the
    CPU ops: the global adapter rows agree to the model-level tolerance."""
    from ddl25spring_amd.fl.lora import FedLoRA, FedLoRAConfig
    from ddl25spring_amd.runtime.dist import DistContext
    cfg = FedLoRAConfig(clients=4, client_fraction=1.0, slots=2, local_steps=2, batch_size=2, lr=1e-3, rounds=1,
                        lora_rank=8, lora_alpha=16.0, dialects=2, sub_vocab=256, eval_batches=1, **CFG)
    rows = []
    for dev in (torch.device("cpu"), cuda):
        eng = FedLoRA(cfg, DistContext(device=dev))
        res = eng.run()
        assert len(res.heldout_loss) == 2 and eng.waves_last_round == 2
        rows.append(eng.global_row.detach().cpu())
    assert rows[1].abs().sum() > 0
    e = _rel(rows[1], rows[0])
    print(f"global row, device vs CPU: {e:.2e}")
    assert e < 1e-4
