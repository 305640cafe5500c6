"""``fedlora``: federated LoRA fine-tuning of the LLaMA (fl/lora.py).

    python -m ddl25spring_amd fedlora --clients 8 --slots 8 --dialects 2 --rounds 5 \\
        --pretrain-iters 200 --lora-rank 8 --report-gap true --jsonl runs/fedlora.jsonl

Every round writes one JSONL record: ``round``, ``heldout_loss`` (per dialect; round 0 is the base
model), ``round_time``, ``tokens``, ``tokens_per_s``, ``message_count`` and, with ``--report-gap``,
``gap`` and ``mean_merged_loss``. ``--sample-tokens N`` continues held-out prompts with the merged
global adapter at the end (``samples`` in the final record). ``--sample-adapters clients`` instead
continues, for each client of the last round, one held-out prompt of its grammar under the base
model, the global adapter and the client's own upload, batched through per-sequence adapters with
nothing merged; each sample is then ``{client, dialect, adapter, tokens}``."""
from __future__ import annotations

from ..fl.lora import FedLoRA, FedLoRAConfig, FedLoRAResult  # noqa: F401  (the CLI reads the config here)


def run_fedlora(cfg: FedLoRAConfig, ctx, log=print) -> FedLoRAResult:
    from ..utils.metrics import JsonlLogger
    eng = FedLoRA(cfg, ctx, log=log if ctx.rank == 0 else None)
    res = eng.run()
    if cfg.sample_tokens > 0:
        res.samples = eng.sample(cfg.sample_tokens, cfg.sample_prompt_len)
        if log:
            for s in res.samples:
                log(f"[fedlora] sample: {s}")
    with JsonlLogger(cfg.jsonl, ctx.rank) as jl:
        for rec in eng.records:
            rec = dict(rec)
            if rec.get("round_time"):
                rec["tokens_per_s"] = rec["tokens"] / max(rec["round_time"], 1e-9)
            jl.log(**rec)
        if cfg.sample_tokens > 0:
            jl.log(round=eng.round_idx, samples=res.samples)
    return res
