"""Every softmax-shaped kernel at extreme logits, against the float64 oracle and the ONE acceptance
rule of tests/softmax_oracle.py (err[r] <= MARGIN * budget[r] + FLOOR per row, budget = the error
of torch fp32 on the CPU on the same inputs), at the smallest shapes that reach each dispatch tier.

Kernels: ddl_cevf (register tiers 8 / 16 / 32, 16-byte and scalar streaming), ddl_cevp_stats /
ddl_cevp_grad (W = 1 and W = 2), ddl_ce_vocab / _fused / _lse + _grad (bf16), ddl_ce_fwd_bwd[_f32]
(per class), ddl_ce_f32 (tabular), ddl_head_train / ddl_headf_train, ddl_attnf_fwd / _bwd.

Structural checks, exact: the loss is finite on every regime, the gradient is 0 at every -inf
column, gradient row and row loss are 0 for an ignored / out-of-range label, `tie` counts the first
maximum. The per-class, tabular and head kernels have no ignore_index (their labels index the row,
their torch reference raises on a label out of range): they get every regime but those two.
Probability targets skip the masked regimes (torch itself returns 0 * -inf = NaN there).

Each test prints its worst err / (MARGIN * budget + FLOOR) per regime. Worst ratio over all widths as
measured on an MI355X when these tests were added (1.0 = the rule's limit):

  kernel        drawn peak12 peak30 other30 off+50 off-50 spread uniform tie  mask_head mask_span loss
  cevf / cevp   0.07  0.19   0.09   0.08    0.11   0.10   0.58   0.16    0.25 0.14      0.09      0.25
  bf16 LM       0.50  0.50   0.21   0.50    0.50   0.50   0.50   0.50    0.50 0.50      0.50      0.09
  per class     0.50  0.50   0.00   0.50    0.50   0.50   0.50   0.50    0.50 0.50      -         0.36
  tabular       0.23  0.11   0.00   0.11    0.13   0.21   0.13   0.08    0.20 0.11      -         0.34
  head bf16     0.10  0.27   0.00   0.21    0.11   0.17   0.12   0.11    0.23 0.05      -         -
  head fp32     0.08  0.36   0.00   0.02    0.22   0.50   1.86   0.54    0.03 0.14      -         -
  (head fp32 spread 1.86: HEAD_OPEN below, an open finding)
  (0.50 = one bf16 rounding of the gradient against MARGIN_BF16 = 2)
  attention     drawn sharp  one_key constant big_v
    o           0.33  3.13   0.29    0.32     0.32
    dq          0.90  12.85  9.6e6   0.42     1.49
    dk          0.66  3.30   6.26    0.81     0.70
    dv          0.58  8.01   0.62    0.55     0.58     (above 1: ATTN_OPEN below, open findings)"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import softmax_oracle as SO
from ddl25spring_amd.ops import _lib
from ddl25spring_amd.ops import autograd_ops as A
from ddl25spring_amd.ops import functional as Fn
from ddl25spring_amd.ops import llama_f32 as L32
from ddl25spring_amd.ops import tabular_ops as TO
from ddl25spring_amd.ops._lib import check, ptr, stream

pytestmark = pytest.mark.gpu
IGNORE = SO.IGNORE
SCALE = 0.5


@functools.lru_cache(maxsize=None)
def _case(V, bf=False, kind="lm", seed=0, k=None):
    """Regimes, oracle and budgets of one width, made once on the CPU and shared (read only).
    kind: "lm" every regime, k = unit(SCALE); "hard" without ignored / out_of_range; "soft"
    probability targets, also without the masked regimes."""
    drop = {"lm": (), "hard": SO.NO_LABEL, "soft": SO.MASKED + SO.NO_LABEL}[kind]
    z, lab, names = SO.select(*SO.ce_rows(V, seed=1000 + V + seed), drop)
    if bf:
        z = SO.bf16(z)
    k = SO.unit(SCALE, lab.numpy()) if k is None else k
    c = SimpleNamespace(V=V, z=z, lab=lab, names=names, k=k, t=None, R=z.shape[0])
    if kind == "soft":
        c.t = SO.soft_targets(z, lab, names, seed=seed + 5)
        c.rowloss64, c.grad64, amax, ytrue = SO.soft_ce(z.numpy(), c.t.numpy())
        c.bl, c.bg, c.bt = SO.budget_soft(z, c.t, k, bf16_out=bf)
    else:
        c.rowloss64, c.grad64 = SO.hard_ce(z.numpy(), lab.numpy())
        c.bl, c.bg, c.bt = SO.budget_hard(z, lab, k, bf16_out=bf)
        amax, ytrue = z.double().numpy().argmax(axis=1), lab.numpy()
    c.correct = int((amax == ytrue).sum())
    if "tie" in names:  # the label (or target) is the second / first tie column: argmax is the first
        assert (amax[names.index("tie")] == ytrue[names.index("tie")]) == (kind == "soft")
    return c


def _structure(what, c, d, rowloss=None):
    d = d.detach().float().cpu()
    assert torch.isfinite(d).all(), what
    assert (d[torch.isinf(c.z)] == 0).all(), f"{what}: gradient at a -inf column"
    for n in SO.NO_LABEL:
        if n in c.names:
            i = c.names.index(n)
            assert (d[i] == 0).all(), f"{what}: gradient row of {n}"
            assert rowloss is None or rowloss[i].item() == 0, f"{what}: row loss of {n}"
    if rowloss is not None:
        assert torch.isfinite(rowloss).all(), what


def _hold(what, c, loss, rowloss, d, margin):
    """Structure, then the rule: gradient rows, row losses (fp32 outputs: MARGIN_F32) and the loss."""
    assert torch.isfinite(loss).all(), f"{what}: loss {loss}"
    _structure(what, c, d, rowloss)
    SO.check(f"{what} grad", c.names, SO.grad_err(d.detach().float().double() / c.k, c.grad64), c.bg, margin)
    if rowloss is not None:
        SO.check(f"{what} rowloss", c.names, SO.loss_err(rowloss, c.rowloss64), c.bl, SO.MARGIN_F32)
    SO.check_total(f"{what} loss", loss.item(), c.k, c.rowloss64, c.bt, SO.MARGIN_F32)


# ------------------------------------------------------------------------ fp32 LM loss: ddl_cevf
# register tiers of 8192 / 16384 / 32768 columns; 32772 streams on the 16-byte path, 1001 on the
# scalar path, and so does every width whose row stride is odd
CEVF_V = (36, 1001, 8192, 8196, 16388, 32772)


def _cevf(z, lab, k):
    """ddl_cevf on rows z [R, V] with unit column stride (the row stride may be wider)
    -> (loss [1], rowloss [R], d [R, V])."""
    R, V = z.shape
    assert z.stride(1) == 1 and z.stride(0) >= V and lab.dtype == torch.int32 and lab.numel() == R
    inv = torch.tensor([k], dtype=torch.float32, device=z.device)
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    rowloss = torch.empty(R, dtype=torch.float32, device=z.device)
    d = torch.empty(R, V, dtype=torch.float32, device=z.device)
    check(L32.K().ddl_cevf(ptr(z), ptr(lab), R, V, z.stride(0), ptr(inv), IGNORE, ptr(rowloss), ptr(loss), ptr(d),
                           V, stream()), "cevf")
    return loss, rowloss, d


@pytest.mark.parametrize("V", CEVF_V)
def test_cross_entropy_vocab_f32(cuda, V):
    c = _case(V)
    zc, labc = c.z.to(cuda), c.lab.to(cuda, torch.int32)
    x = zc.clone().requires_grad_(True)
    loss = A.cross_entropy_vocab(x, labc, IGNORE, scale=SCALE)
    loss.backward()
    l1, rowloss, d = _cevf(zc, labc, c.k)
    assert torch.equal(l1[0], loss.detach()) and torch.equal(d, x.grad)  # the op is this kernel
    _hold(f"cevf V={V}", c, loss.detach(), rowloss, d, SO.MARGIN_F32)
    # rows of a wider tensor (odd row stride: no 16-byte alignment), read in place by the kernel
    wide = torch.full((c.R, V + 3), 7.0, device=cuda)
    wide[:, :V] = zc
    l2, rl2, d2 = _cevf(wide[:, :V], labc, c.k)
    _hold(f"cevf V={V} strided", c, l2[0], rl2, d2, SO.MARGIN_F32)
    # the same view through the op (which copies it): the contiguous call's bits, nothing outside
    wide.requires_grad_(True)
    loss3 = A.cross_entropy_vocab(wide[:, :V], labc, IGNORE, scale=SCALE)
    loss3.backward()
    assert torch.equal(loss3.detach(), loss.detach()) and torch.equal(wide.grad[:, :V], x.grad)
    assert wide.grad[:, V:].abs().max().item() == 0


# ------------------------------------------------- sharded fp32 LM loss: ddl_cevp_stats / _grad
CEVP_CASES = [(V, (0, V)) for V in CEVF_V] + [(1001, (0, 333, 1001)), (16388, (0, 8192, 16388))]


def _sharded_ce(zc, labc, bounds, V, scale):
    """tests/test_tp_gpu.py::_sharded_ce: the W ranks' work in one process, on column slices of zc."""
    W = len(bounds) - 1
    inv = (labc != IGNORE).sum(dtype=torch.float32).clamp_min_(1.0).reciprocal_().reshape(1) * scale
    views = [zc[:, bounds[t]:bounds[t + 1]] for t in range(W)]
    stats = torch.stack([L32.cevp_stats(v, labc, bounds[t], IGNORE) for t, v in enumerate(views)])
    return [L32.cevp_grad(v, labc, stats, bounds[t], V, inv, IGNORE) for t, v in enumerate(views)], stats


@pytest.mark.parametrize("V,bounds", CEVP_CASES, ids=[f"V{v}-" + "_".join(map(str, b)) for v, b in CEVP_CASES])
def test_cross_entropy_vocab_parallel_f32(cuda, V, bounds):
    c = _case(V)
    zc, labc = c.z.to(cuda), c.lab.to(cuda, torch.int32)
    outs, stats = _sharded_ce(zc, labc, bounds, V, SCALE)
    for loss, rowloss, _ in outs:  # same bits on every rank
        assert torch.equal(loss, outs[0][0]) and torch.equal(rowloss, outs[0][1])
    d = torch.cat([o[2] for o in outs], dim=1)
    _hold(f"cevp V={V} W={len(bounds) - 1}", c, outs[0][0][0], outs[0][1], d, SO.MARGIN_F32)
    if bounds[1] <= min(V // 2, 2048):  # masked_head covers rank 0's shard: an empty record, not a NaN
        i = c.names.index("masked_head")
        assert stats[0, i, 0].item() == float("-inf") and stats[0, i, 1].item() == 0.0


# ----------------------------------------- bf16 LM loss: ddl_ce_vocab, _fused, _lse + _grad
# 40: one chunk per thread; 8192 / 32768: the fused kernel's register rows (its last width);
# 32776: above CE_FUSED_MAX_V, the lse + gradient pair
CE_BF16_V = (40, 8192, 32768, 32776)


@pytest.mark.parametrize("V", CE_BF16_V)
def test_cross_entropy_vocab_bf16(cuda, V):
    c = _case(V, bf=True)
    zb, labc = c.z.to(cuda, torch.bfloat16), c.lab.to(cuda, torch.int32)
    x = zb.clone().requires_grad_(True)
    loss = A.cross_entropy_vocab(x, labc, IGNORE, scale=SCALE)
    loss.backward()
    assert x.grad.dtype == torch.bfloat16
    _hold(f"ce_vocab bf16 V={V}", c, loss.detach(), None, x.grad, SO.MARGIN_BF16)
    with torch.no_grad():  # no gradient wanted: ddl_ce_vocab_lse at every width
        l0 = A.cross_entropy_vocab(zb, labc, IGNORE, scale=SCALE)
    SO.check_total(f"ce_vocab_lse V={V} loss", l0.item(), c.k, c.rowloss64, c.bt, SO.MARGIN_F32)
    # the kernels add the rows' losses into one scalar: one row per call gives the row's loss
    rows = []
    for r in range(c.R):
        xr = zb[r:r + 1].clone().requires_grad_(True)
        rows.append(A.cross_entropy_vocab(xr, labc[r:r + 1], IGNORE, scale=1.0).detach())
    rowloss = torch.stack(rows)
    assert torch.isfinite(rowloss).all()
    for n in SO.NO_LABEL:
        assert rowloss[c.names.index(n)].item() == 0, n
    SO.check(f"ce_vocab bf16 V={V} rowloss", c.names, SO.loss_err(rowloss, c.rowloss64), c.bl, SO.MARGIN_F32)
    # ddl_ce_vocab (host-side scale), which has no Python wrapper
    loss3 = torch.zeros(1, dtype=torch.float32, device=cuda)
    d3 = torch.empty_like(zb)
    check(_lib.kernels().ddl_ce_vocab(ptr(zb), ptr(labc), c.R, V, V, float(c.k), IGNORE, ptr(loss3), ptr(d3),
                                      stream()), "ce_vocab")
    _hold(f"ddl_ce_vocab V={V}", c, loss3[0], None, d3, SO.MARGIN_BF16)


# --------------------------------------------------------- per-class CE: ddl_ce_fwd_bwd[_f32]
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ncls", [2, 10, 64, 65, 100])
def test_per_class_cross_entropy(cuda, ncls, dtype, soft):
    bf = dtype == torch.bfloat16
    margin = SO.MARGIN_BF16 if bf else SO.MARGIN_F32
    k, ld = 0.25, ncls + 6
    cs = [_case(ncls, bf, "soft" if soft else "hard", seed, k) for seed in (0, 1)]  # G = 2 groups
    N = cs[0].R
    logits = torch.full((2, N, ld), 99.0)  # pad columns the kernel must not read
    for g, c in enumerate(cs):
        logits[g, :, :ncls] = c.z
    logits = logits.to(cuda, dtype)
    labels = None if soft else torch.stack([c.lab for c in cs]).to(cuda, torch.int32)
    targets = torch.stack([c.t for c in cs]).to(cuda) if soft else None
    loss, d, correct = Fn.cross_entropy(logits, labels, targets, ncls=ncls, scale=k, with_correct=True)
    loss = loss.clone()
    assert d.dtype == dtype and d[..., ncls:].abs().max().item() == 0  # pad columns: exactly 0
    for g, c in enumerate(cs):
        what = f"ce ncls={ncls} {'bf16' if bf else 'f32'} {'soft' if soft else 'hard'} g{g}"
        _hold(what, c, loss[g], None, d[g, :, :ncls], margin)
        assert correct[g].item() == c.correct, what
    # rows as groups: a loss per row
    rl = Fn.cross_entropy(logits.reshape(2 * N, 1, ld), None if soft else labels.reshape(2 * N, 1),
                          targets.reshape(2 * N, 1, ncls) if soft else None, ncls=ncls, scale=1.0,
                          want_grad=False)[0].clone().reshape(2, N)
    for g, c in enumerate(cs):
        SO.check(f"ce ncls={ncls} g{g} rowloss", c.names, SO.loss_err(rl[g], c.rowloss64), c.bl, SO.MARGIN_F32)


# ------------------------------------------------------------------------ tabular CE: ddl_ce_f32
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("C", [2, 65, 1000])
def test_tabular_cross_entropy(cuda, C, soft):
    c0 = _case(C, False, "soft" if soft else "hard", 2, 1.0)
    c = _case(C, False, "soft" if soft else "hard", 2, 1.0 / c0.R)  # mean over the M = R rows
    x = c.z.to(cuda).requires_grad_(True)
    tgt = c.t.to(cuda) if soft else c.lab.to(cuda)
    loss = TO.cross_entropy(x, tgt)
    loss.backward()
    what = f"tabular C={C} {'soft' if soft else 'hard'}"
    _hold(what, c, loss.detach(), None, x.grad, SO.MARGIN_F32)
    rowloss = torch.stack([TO.cross_entropy(c.z[r:r + 1].to(cuda), tgt[r:r + 1]).detach() for r in range(c.R)])
    assert torch.isfinite(rowloss).all()
    SO.check(f"{what} rowloss", c.names, SO.loss_err(rowloss, c.rowloss64), c.bl, SO.MARGIN_F32)


# ------------------------------------- fused classifier heads: ddl_head_train / ddl_headf_train
# (N, H, W, C, Kp, ncls) of tests/test_kernels_gpu.py::HEAD_CASES (bf16, 64 classes: one lane each)
# and of tests/test_fp32_gpu.py::test_head_f32_matches_torch (fp32); one group per regime, the
# regime driven through the group's bias so that the logits INSIDE the kernel are extreme
HEADS = {"bf16": (torch.bfloat16, 4, 1, 1, 256, 64, 64), "f32": (torch.float32, 7, 4, 4, 512, 32, 10)}


# OPEN FINDING: regimes ddl_headf_train (fp32) does not hold the rule on, left out of the assertion
# (still run, checked for finite values and structure, ratio printed). It forms lse = mx + log(sum)
# and exp(z - lse), rounded at the magnitude of the logits; the fix that ddl_head_train (bf16) took
# changes the last bits of the benchmark's trained weights, so it waits for a change that may.
# Measured: db spread_20 1.86 (every other regime, and the loss on all of them, at most 0.54).
HEAD_OPEN = {"f32": ("spread_20",)}


@functools.lru_cache(maxsize=None)
def _head_case(name):
    dtype, N, H, W, C, Kp, ncls = HEADS[name]
    z, lab, names = SO.select(*SO.ce_rows(ncls, seed=77), SO.NO_LABEL)
    G = z.shape[0]
    g = torch.Generator().manual_seed(78)
    x = torch.randn(G, N, H, W, C, generator=g).relu().to(dtype)
    w = (torch.randn(G, Kp, 1, 1, C, generator=g) * 0.05).to(dtype)
    a, b2 = SO.tie_columns(ncls)
    w[names.index("tie"), b2] = w[names.index("tie"), a]  # equal rows + equal bias: an exact tie
    b = torch.zeros(G, Kp)
    b[:, :ncls] = z
    labels = lab.reshape(G, 1).expand(G, N).contiguous()
    scale = 0.25 if N == 4 else 0.125
    def logits(prec):  # pooled mean -> Linear -> + bias in plain torch
        zz = torch.einsum("gnc,gkc->gnk", x.to(prec).mean((2, 3)), w.to(prec).reshape(G, Kp, C)[:, :ncls])
        zz = zz + b.to(prec)[:, None, :ncls]
        zz[names.index("tie"), :, b2] = zz[names.index("tie"), :, a]  # exact, whatever a GEMM's summing order
        return zz

    # the oracle: float64 logits through the float64 CE; the budget's reference: fp32 logits through
    # torch's fp32 CE; loss and db are sums over the group's N samples
    zz64 = logits(torch.float64)
    loss64, db64, loss32, db32 = [], [], [], []
    for i in range(G):
        rl, gr = SO.hard_ce(zz64[i].numpy(), labels[i].numpy())
        loss64.append(rl.sum()); db64.append(gr.sum(axis=0))
        rl, _, gr = SO._ref_hard(logits(torch.float32)[i], labels[i], scale)
        loss32.append(float(rl.sum())); db32.append((gr.sum(0).double() / scale).numpy())
    loss64, db64, loss32, db32 = (np.asarray(v, dtype=np.float64) for v in (loss64, db64, loss32, db32))
    correct = (zz64.argmax(-1) == labels).sum(1)
    assert correct[names.index("tie")] == 0 and correct[names.index("peak_label_30")] == N
    return SimpleNamespace(x=x, w=w, b=b, labels=labels, names=names, scale=scale, loss64=loss64, db64=db64,
                           correct=correct, bl=SO.loss_err(loss32, loss64), bg=SO.grad_err(db32, db64))


@pytest.mark.parametrize("name", list(HEADS))
def test_head_train(cuda, name):
    dtype, N, H, W, C, Kp, ncls = HEADS[name]
    c = _head_case(name)
    G = len(c.names)
    assert Fn.head_train_ok(C, ncls, dtype)
    dw = torch.zeros(G, Kp, 1, 1, C, device=cuda)
    db = torch.zeros(G, Kp, device=cuda)
    loss, correct, dx, _ = Fn.head_train(c.x.to(cuda), c.w.to(cuda), c.b.to(cuda), c.labels.to(cuda, torch.int32),
                                         ncls, c.scale, dw, db, bn=None, with_correct=True)
    loss, db = loss.clone().cpu(), db.cpu()
    assert torch.isfinite(loss).all() and torch.isfinite(db).all() and torch.isfinite(dw).all()
    assert torch.isfinite(dx.float()).all()
    assert (db[:, :ncls][torch.isinf(c.b[:, :ncls])] == 0).all() and (db[:, ncls:] == 0).all()
    held = [n not in HEAD_OPEN.get(name, ()) for n in c.names]
    bad = []
    for what, err, bud in (("db", SO.grad_err(db[:, :ncls].double() / c.scale, c.db64), c.bg),
                           ("loss", SO.loss_err(loss.double() / c.scale, c.loss64), c.bl)):
        r = SO.ratios(err, bud, SO.MARGIN_F32)
        print(f"head {name} {what}: " + "  ".join(f"{n}={x:.2f}" for n, x in zip(c.names, r)))
        bad += [(what, n, float(e), float(bb), float(x)) for n, e, bb, x, h in zip(c.names, err, bud, r, held)
                if h and not x <= 1.0]
    assert not bad, f"head {name}: (output, regime, err, budget, ratio) {bad}"
    assert torch.equal(correct.cpu().long(), c.correct), (correct, c.correct)


# -------------------------------------------------------------- fp32 attention: ddl_attnf_*
# S = 1 and 17 sit under one 64-row tile; 65 and 130 cross tiles with a one- / two-row tail
ATTN_SHAPES = [(1, 1, 1, 16), (2, 17, 2, 16), (1, 65, 2, 128), (2, 130, 2, 48)]


# OPEN FINDINGS: (regime, output) pairs the kernels do not hold the rule on, left out of the assertion
# (they are still run, checked for finite values, and their ratio printed). Worst measured ratios:
#   sharp    o 3.1  dq 12.9  dk 3.3  dv 8.0   scores of +-70 in the log2 domain: exp2(s * sl2 - lse)
#            rounds s * sl2 and lse there (4e-6 on every P), in the forward's rescale as well
#   one_key  dq 9.6e6  dk 6.3    P = 1 on key 0, dS = P (dP - delta) is pure cancellation: delta =
#            rowsum(dO * O) and dP = dO . v are summed in different orders and differ by 1e-7 |dP|,
#            where torch's sum(P * dP) - dP is exactly 0 (budget 0: the floor is the only slack)
#   big_v    dq 1.5 (S = 17 only)    the same cancellation, |dP| and delta 1e3 times larger
ATTN_OPEN = {"sharp": ("o", "dq", "dk", "dv"), "one_key": ("dq", "dk"), "big_v": ("dq",)}


@functools.lru_cache(maxsize=None)
def _attn_case(B, S, H, hd, regime):
    g = torch.Generator().manual_seed(10 * S + hd)
    dout = torch.randn(B, S, H * hd, generator=g)
    qkv = SO.attention_qkv(B, S, H, hd, regime, seed=S)
    o64, d64 = SO.attention64(qkv, H, hd, dout)
    return qkv, dout, o64, d64, SO.budget_attention(qkv, H, hd, dout, regime == "constant")


@pytest.mark.parametrize("regime", SO.ATTN_REGIMES)
@pytest.mark.parametrize("B,S,H,hd", ATTN_SHAPES)
def test_causal_attention_f32(cuda, B, S, H, hd, regime):
    qkv, dout, o64, d64, bud = _attn_case(B, S, H, hd, regime)
    x = qkv.to(cuda).requires_grad_(True)
    o = A.causal_attention(x, H, hd)
    o.backward(dout.to(cuda))
    assert o.dtype == torch.float32 and torch.isfinite(o).all() and torch.isfinite(x.grad).all()
    err = SO.attention_errors(o.detach(), x.grad, o64, d64, H, hd, regime == "constant")
    worst = {n: SO.ratios(err[n], bud[n], SO.MARGIN_F32) for n in err}
    print(f"attention B{B} S{S} H{H} hd{hd} {regime}: " + "  ".join(f"{n}={r.max():.2f}" for n, r in worst.items()))
    for n, r in worst.items():
        if n in ATTN_OPEN.get(regime, ()):
            continue
        i = np.unravel_index(np.argmax(r), r.shape)
        assert r.max() <= 1.0, (regime, n, "(batch, query, head)", i, float(err[n][i]), float(bud[n][i]))
