"""The FedLoRA engine (fl/lora.py) on the CPU reference ops: a base pretrained on one grammar,
4 clients over 2 other grammars, rank 4, alpha 8, 8 local Adam steps at lr 1e-2.

A stock-torch probe of this configuration gave the held-out losses 6.65 -> 4.12 -> 3.59 -> 3.21
(first dialect) and 6.21 -> 4.15 -> 3.79 -> 3.45 (second) over rounds 0..3, a relative gap between
the mean of the clients' B A and the aggregate's B A of 0.127, 0.071, 0.056 with A trained and of
7e-8 with A frozen. The assertions leave more than a factor of 10 to those: the gap above 1e-3 with
A trained, below 1e-5 with ``lora_freeze_a``."""
import json
import types

import pytest
import torch

from ddl25spring_amd.fl.lora import FedLoRA, FedLoRAConfig, build_base
from ddl25spring_amd.runtime.dist import DistContext

MODEL = dict(vocab_size=96, dmodel=32, num_heads=2, n_layers=4, ctx_size=16)
BASE = dict(clients=4, client_fraction=1.0, slots=4, local_steps=8, batch_size=4, lr=1e-2, rounds=3, lora_rank=4,
            lora_alpha=8.0, dialects=2, sub_vocab=64, branching=4, eval_batches=4, pretrain_iters=150, **MODEL)
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    """The base model, pretrained once on the default grammar and shared through ``base_ckpt``."""
    path = str(tmp_path_factory.mktemp("fedlora") / "base.pt")
    build_base(FedLoRAConfig(base_ckpt=path, **BASE), CPU)
    return path


def _engine(base_ckpt, **kw):
    return FedLoRA(FedLoRAConfig(base_ckpt=base_ckpt, **{**BASE, **kw}), DistContext(device=CPU))


@pytest.fixture(scope="module")
def trained(base_ckpt):
    eng = _engine(base_ckpt, report_gap=True)
    return eng, eng.run()


def test_loss_falls_on_every_dialect_each_round(trained):
    _, res = trained
    print(res.heldout_loss, res.gap)
    assert res.round == [0, 1, 2, 3] and all(len(l) == 2 for l in res.heldout_loss)
    for d in range(2):
        curve = [l[d] for l in res.heldout_loss]
        assert all(b < a for a, b in zip(curve, curve[1:])), curve


def test_round_zero_is_the_base_model(trained, base_ckpt):
    from ddl25spring_amd.models.llama import LLama, causalLLMLoss
    eng, res = trained
    m = LLama(**MODEL)
    m.load_state_dict(torch.load(base_ckpt, weights_only=True))
    for d in range(2):
        with torch.no_grad():
            want = sum(float(causalLLMLoss(m(x), x)) for x in (eng.heldout_batch(d, i) for i in range(4))) / 4
        assert res.heldout_loss[0][d] == want


def test_separate_averaging_leaves_a_gap_and_freeze_a_closes_it(trained, base_ckpt):
    _, res = trained
    assert len(res.gap) == 3 and all(g > 1e-3 for g in res.gap), res.gap
    assert all(len(l) == 2 for l in res.mean_merged_loss)
    ffa = _engine(base_ckpt, report_gap=True, lora_freeze_a=True, rounds=2).run()
    print(ffa.gap, ffa.heldout_loss)
    assert all(g < 1e-5 for g in ffa.gap), ffa.gap
    assert ffa.heldout_loss[-1][0] < ffa.heldout_loss[0][0]
    # the aggregate IS the mean of the merged clients: the same loss up to rounding
    for a, b in zip(ffa.heldout_loss[1:], ffa.mean_merged_loss):
        assert a == pytest.approx(b, rel=1e-4)


@pytest.mark.parametrize("agg", ["median", "clipped"])
def test_robust_rules_run_through_the_same_loop(base_ckpt, agg):
    eng = _engine(base_ckpt, aggregator=agg, rounds=1, clip_norm=5.0)
    g0 = eng.global_row.clone()
    res = eng.run()
    assert not torch.equal(eng.global_row, g0) and bool(torch.isfinite(eng.global_row).all())
    assert res.heldout_loss[1][0] < res.heldout_loss[0][0]


def test_waves_and_partial_participation(base_ckpt):
    """2 slots: 4 clients in 2 waves give the 4-slot run's global row (a client's training does not
    depend on who shares the wave; the base GEMMs may round differently at another batch size);
    C = 0.5 samples 2 clients."""
    a, b = _engine(base_ckpt, rounds=1), _engine(base_ckpt, rounds=1, slots=2)
    a.run(), b.run()
    assert b.waves_last_round == 2
    assert ((a.global_row - b.global_row).norm() / a.global_row.norm()).item() < 1e-4
    c = _engine(base_ckpt, rounds=1, client_fraction=0.5)
    c.run()
    assert c.K == 2 and len(c.records[1]["clients"]) == 2


def test_fltrust_and_multi_process_are_refused(base_ckpt):
    with pytest.raises(ValueError, match="root"):
        _engine(base_ckpt, aggregator="fltrust")
    ctx = types.SimpleNamespace(world=2, rank=0, device=CPU, is_distributed=True)
    with pytest.raises(NotImplementedError, match="one process"):
        FedLoRA(FedLoRAConfig(base_ckpt=base_ckpt, **BASE), ctx)


def test_resume_is_bit_identical(base_ckpt, tmp_path):
    whole = _engine(base_ckpt, rounds=3, client_fraction=0.5)
    whole.run()
    path = str(tmp_path / "fedlora.pt")
    _engine(base_ckpt, rounds=2, client_fraction=0.5, checkpoint=path).run()
    resumed = _engine(base_ckpt, rounds=3, client_fraction=0.5, checkpoint=path)
    resumed.run()
    assert resumed.round_idx == 3 and torch.equal(resumed.global_row, whole.global_row)
    strip = lambda recs: [{k: v for k, v in r.items() if k != "round_time"} for r in recs]  # noqa: E731
    assert strip(resumed.records) == strip(whole.records)


def test_cli_writes_jsonl_and_samples(base_ckpt, tmp_path):
    from ddl25spring_amd.cli import main
    out = tmp_path / "run.jsonl"
    args = ["--device", "cpu", "fedlora", "--base-ckpt", base_ckpt, "--jsonl", str(out), "--rounds", "1",
            "--report-gap", "true", "--sample-tokens", "5", "--sample-prompt-len", "4"]
    for k, v in BASE.items():
        if k not in ("rounds",):
            args += ["--" + k.replace("_", "-"), str(v)]
    assert main(args) == 0
    recs = [json.loads(l) for l in out.read_text().splitlines()]
    assert [r["round"] for r in recs] == [0, 1, 1]
    assert len(recs[0]["heldout_loss"]) == 2
    for k in ("heldout_loss", "round_time", "tokens", "tokens_per_s", "message_count", "gap", "mean_merged_loss",
              "clients"):
        assert k in recs[1], k
    samples = recs[2]["samples"]
    assert len(samples) == 2 * 4 and all(len(s) == 5 and all(0 <= t < 96 for t in s) for s in samples)
