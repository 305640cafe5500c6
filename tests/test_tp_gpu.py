"""Tensor parallelism on the device: the vocabulary-parallel cross-entropy kernels
(ddl_cevp_stats / ddl_cevp_grad, csrc/kernels/llama_f32.hip) against the float64 full-row oracle of
tests/vocab_parallel_oracle.py, and a tp = 2 LLaMA (two gloo ranks sharing the GPU) against a
float64 copy of the unsharded model.

The kernel tests run in one process: the W shards are column slices of ONE [R, V] fp32 tensor
(row stride V), so misaligned bases and strided rows are read in place; the records of the W
"ranks" are stacked in rank order as the all-gather would leave them.

Tolerance: the project's own CE bound (1e-6 relative, tests/test_llama_f32_gpu.py::test_vocab_ce_f32)."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import vocab_parallel_oracle as O
from ddl25spring_amd.ops import autograd_ops as A
from ddl25spring_amd.ops import llama_f32 as L32
from ddl25spring_amd.parallel.tp import vocab_range

pytestmark = pytest.mark.gpu
TOL = 1e-6
IGNORE = -100


def _bounds(V, tp):
    return tuple(vocab_range(V, tp, t)[0] for t in range(tp)) + (V,)


# (V, shard bounds). Shard widths at every dispatch boundary of ddl_cevp_stats (register tiers of
# 8192 / 16384 / 32768 columns, mirrored from ddl_cevf): 8192 | 8196, 16384 | 16388, 32768 | 32772
# (the last one streams, 16-byte path); 333 / 334 columns stream on the scalar path.
CASES = [
    (36, (0, 20, 36)),
    (1000, (0, 333, 667, 1000)),
    (8200, (0, 8196, 8200)),
    (16388, (0, 8192, 16388)),
    (32772, (0, 16384, 32772)),
    (65540, (0, 32768, 65540)),
    (32000, _bounds(32000, 2)),
    (32000, _bounds(32000, 3)),
]
R = 5


def _rows(V, bounds, j, seed):
    """Logits and labels of the pass that puts the labels into shard j: row 0 / 1 the shard's first
    / last column, row 2 ignored, row 3 out of range, row 4 a middle column. Row 0's maximum (+80)
    lies in the next shard, row 4's next shard is -inf throughout. With a single shard there is no
    other shard to hold either, and the rows stay as drawn."""
    W = len(bounds) - 1
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R, V, generator=g) * 2
    a, b = bounds[j], bounds[j + 1]
    lab = torch.tensor([a, b - 1, IGNORE, V + 3, (a + b) // 2], dtype=torch.int32)
    if W > 1:
        o = (j + 1) % W
        z[0, bounds[o]] += 80.0
        z[4, bounds[o]:bounds[o + 1]] = float("-inf")
    return z, lab


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _sharded_ce(zc, labc, bounds, V, scale):
    """The W ranks' work in one process -> per rank (loss, rowloss, dz), all from the same records."""
    W = len(bounds) - 1
    inv = (labc != IGNORE).sum(dtype=torch.float32).clamp_min_(1.0).reciprocal_().reshape(1) * scale
    views = [zc[:, bounds[t]:bounds[t + 1]] for t in range(W)]
    stats = torch.stack([L32.cevp_stats(v, labc, bounds[t], IGNORE) for t, v in enumerate(views)])
    return [L32.cevp_grad(v, labc, stats, bounds[t], V, inv, IGNORE) for t, v in enumerate(views)], stats


@pytest.mark.parametrize("V,bounds", CASES, ids=[f"V{v}-" + "_".join(map(str, b)) for v, b in CASES])
def test_cevp_kernels_match_float64_oracle(cuda, V, bounds):
    W = len(bounds) - 1
    for j in range(W):
        z, lab = _rows(V, bounds, j, seed=100 + j)
        loss64, rowloss64, grad64 = O.full_ce(z.numpy(), lab.numpy(), IGNORE, scale=0.5)
        zc, labc = z.to(cuda), lab.to(cuda)
        outs, stats = _sharded_ce(zc, labc, bounds, V, 0.5)
        # the -inf shard of row 4: an empty record, not a NaN
        o = (j + 1) % W
        assert stats[o, 4, 0].item() == float("-inf") and stats[o, 4, 1].item() == 0.0
        for t, (loss, rowloss, dz) in enumerate(outs):
            e_loss = abs(loss.item() - loss64) / abs(loss64)
            e_row = _rel(rowloss.cpu().numpy(), rowloss64)
            e_dz = _rel(dz.cpu().numpy(), O.shard(grad64, bounds, t))
            print(f"V={V} labels in shard {j}, rank {t}: loss {e_loss:.2e} rowloss {e_row:.2e} dz {e_dz:.2e}")
            assert np.isfinite(loss.item()) and e_loss < TOL and e_row < TOL and e_dz < TOL, (j, t)
            assert torch.equal(loss, outs[0][0]) and torch.equal(rowloss, outs[0][1])  # same bits on every rank
            # ignored / out-of-range rows: zero loss, zero gradient; the -inf shard: zero gradient
            assert rowloss[2].item() == 0 and rowloss[3].item() == 0
            assert dz[2].abs().max().item() == 0 and dz[3].abs().max().item() == 0
        assert outs[o][2][4].abs().max().item() == 0


@pytest.mark.parametrize("V", [36, 1000, 8200, 32000, 32772])
def test_single_shard_matches_cross_entropy_vocab(cuda, V):
    """W = 1 (no process group): the same rows through the new pair and through ddl_cevf."""
    z, lab = _rows(V, (0, V), 0, seed=7)
    za = z.to(cuda).requires_grad_(True)
    zb = z.to(cuda).requires_grad_(True)
    labc = lab.to(cuda)
    a = A.cross_entropy_vocab_parallel(za, labc, 0, V, None, None, IGNORE, scale=0.5)
    b = A.cross_entropy_vocab(zb, labc, IGNORE, scale=0.5)
    assert abs(a.item() - b.item()) < TOL * abs(b.item())
    a.backward(); b.backward()
    assert _rel(za.grad.cpu().numpy(), zb.grad.cpu().numpy()) < TOL
    loss64, _, grad64 = O.full_ce(z.numpy(), lab.numpy(), IGNORE, scale=0.5)
    assert abs(a.item() - loss64) < TOL * abs(loss64) and _rel(za.grad.cpu().numpy(), grad64) < TOL


def test_vocab_parallel_ce_contract(cuda):
    """VocabCEF32's contract: upstream gradient 3, a second backward, and the loss-only path."""
    V, bounds = 1000, (0, 333, 667, 1000)
    z, lab = _rows(V, bounds, 1, seed=11)
    labc = lab.to(cuda)
    _, _, grad64 = O.full_ce(z.numpy(), lab.numpy(), IGNORE, scale=0.5)
    zc = z.to(cuda).requires_grad_(True)
    a = A.cross_entropy_vocab_parallel(zc, labc, 0, V, None, None, IGNORE, scale=0.5)
    (a * 3).backward(retain_graph=True)
    assert _rel(zc.grad.cpu().numpy(), 3 * grad64) < TOL
    zc.grad = None
    a.backward()  # the first backward rescaled the stored gradient in place: this one recomputes it
    assert _rel(zc.grad.cpu().numpy(), grad64) < TOL
    with torch.no_grad():  # no gradient wanted: ddl_cevp_grad with dz = null
        e = A.cross_entropy_vocab_parallel(z.to(cuda), labc, 0, V, None, None, IGNORE, scale=0.5)
    assert torch.equal(e, a.detach())
    # a column slice as the op's input (row stride V, no copy), labels in the middle shard
    inv = torch.tensor([0.5 / 4], device=cuda)
    sl = z.to(cuda)[:, 333:667]
    st = torch.stack([L32.cevp_stats(z.to(cuda)[:, bounds[t]:bounds[t + 1]], labc, bounds[t], IGNORE)
                      for t in range(3)])
    loss_only = L32.cevp_grad(sl, labc, st, 333, V, inv, IGNORE, want_dz=False)
    with_dz = L32.cevp_grad(sl, labc, st, 333, V, inv, IGNORE, want_dz=True)
    assert loss_only[2] is None and torch.equal(loss_only[0], with_dz[0]) and torch.equal(loss_only[1], with_dz[1])


# ------------------------------------------------------------------ two ranks sharing the GPU
MODEL = dict(vocab_size=512, dmodel=96, num_heads=2, n_layers=2, ctx_size=64)
BATCH, SEED = 3, 0


def _first_batch():
    from ddl25spring_amd.data.text import SPTokenizer, TinyStories
    return next(iter(TinyStories(SPTokenizer(MODEL["vocab_size"]), BATCH, MODEL["ctx_size"], skip=0,
                                 seed=1234 + SEED)))


def _tp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from ddl25spring_amd.apps.llm import LLMConfig, train_llm
    from ddl25spring_amd.models.llama import LLama, causalLLMLoss
    from ddl25spring_amd.parallel.tp import TPHandle, shard_llama
    from ddl25spring_amd.runtime import dist as rdist
    ctx = rdist.init(backend="gloo", device="cuda", timeout_s=120)  # a mismatch fails, it does not wait
    # one forward + backward of this rank's shard of the seeded model on the run's first batch
    torch.manual_seed(SEED)
    tph = TPHandle(ctx, None, world, rank)
    mod = shard_llama(LLama(**MODEL), world, rank, tph).to(ctx.device)
    x = _first_batch().to(ctx.device)
    loss = causalLLMLoss(mod(x), x, MODEL["vocab_size"], tp=tph)
    loss.backward()
    grads = {n: p.grad.cpu() for n, p in mod.named_parameters()}
    del mod
    cfg = LLMConfig(**MODEL, batch_size=BATCH, tp=world, graph=False, iters=3, log_every=1, seed=SEED,
                    ckpt_dir=os.path.join(out, "ck"))
    res = train_llm(cfg, ctx, log=None)
    torch.save({"loss0": loss.detach().cpu(), "grads": grads, "losses": res["losses"]},
               os.path.join(out, f"r{rank}.pt"))
    rdist.shutdown()


def test_tp2_llama_two_ranks_share_gpu(cuda):
    import copy
    from ddl25spring_amd.apps.llm import LLMConfig, train_llm
    from ddl25spring_amd.models.llama import LLama, causalLLMLoss
    from ddl25spring_amd.parallel.tp import _kind, gather_llama
    from ddl25spring_amd.runtime.dist import DistContext
    # float64 copy of the FULL model on the same first batch: the reference of loss and gradients
    torch.manual_seed(SEED)
    m64 = copy.deepcopy(LLama(**MODEL)).double()
    x = _first_batch()
    l64 = causalLLMLoss(m64(x), x)
    l64.backward()
    # the unsharded program on the device
    one = train_llm(LLMConfig(**MODEL, batch_size=BATCH, tp=1, graph=False, iters=3, log_every=1, seed=SEED),
                    DistContext(device=cuda), log=None)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_tp_worker, args=(2, 29763, d), nprocs=2, join=True)
        res = [torch.load(os.path.join(d, f"r{r}.pt"), weights_only=True) for r in range(2)]
        shards = [torch.load(os.path.join(d, "ck", "step00000003", f"rank{r:05d}.pt"), weights_only=True)
                  ["state"]["model"] for r in range(2)]
    # the loss: same bits on both ranks, every step; first step within 1e-5 of the tp = 1 run
    assert torch.equal(res[0]["loss0"], res[1]["loss0"])
    assert res[0]["losses"] == res[1]["losses"] and len(res[0]["losses"]) == 3
    first_tp, first_one = res[0]["losses"][0][1], one["losses"][0][1]
    print(f"first-step loss tp=2 {first_tp!r} tp=1 {first_one!r} float64 {l64.item()!r}")
    assert abs(first_tp - first_one) < 1e-5 * abs(first_one)
    assert abs(res[0]["loss0"].item() - l64.item()) < 1e-5 * abs(l64.item())
    # every gathered gradient within the bound of test_llama_step_matches_float64
    full = gather_llama([r["grads"] for r in res], {n: p.shape for n, p in m64.named_parameters()})
    worst = 0.0
    for n, p in m64.named_parameters():
        e = ((full[n].double() - p.grad).norm() / (p.grad.norm() + 1e-30)).item()
        worst = max(worst, e)
        assert e < 1e-4, (n, e)
    print(f"worst relative gradient error {worst:.2e}")
    # replicated parameters (norm gains, embedding): bit-equal on the two ranks after the 3 steps
    rep = [n for n in shards[0] if _kind(n) == "replicated"]
    assert len(rep) == 2 * MODEL["n_layers"] + 2
    for n in rep:
        assert torch.equal(shards[0][n], shards[1][n]), n
    assert not torch.equal(shards[0]["last.head"], shards[1]["last.head"])
