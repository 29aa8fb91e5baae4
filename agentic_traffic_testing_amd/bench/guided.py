"""What the guided-decoding tail costs a decode step, and what a guide costs to compile.

Four variants of the same decode step on one engine (graphs + async look-ahead, bench.py's
configuration, Llama-3.1-8B shape by default), in one process, repeats interleaved:

  topkp            top-k / top-p: logits materialised, the radix-select sampler (variant 1)
  penalty          penalties + logit_bias: penalty_apply -> sample -> penalty_update (variant 8)
  guided           a guide: guide_apply -> sample -> guide_advance (variant 16)
  guided+penalty   both: penalty_apply -> guide_apply in place -> sample -> penalty_update ->
                   guide_advance (variant 24)

per batch size, as wall time per decode step over the steps after the prefill.  All four
materialise the logits, so the differences are the tails.  The guide is ``([a-z]+ )+`` with
ignore_eos: it never ends, so every run has the same length.  Then the apply kernel alone
(replayed from a graph so the host's launch cost stays out), as time per call and achieved
bytes/s over its R x V x (2 logits + 2 table + 4 out) traffic, and the host compile time of a
regex and of a five-field schema at this model's vocabulary.  Needs a GPU.

    python -m agentic_traffic_testing_amd.bench.guided [--model M] [--repeats 3]
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from ..engine.sequence import SamplingParams
from .penalties import run

VARIANTS = ("topkp", "penalty", "guided", "guided+penalty")
PATTERN = r"([a-z]+ )+"
SCHEMA = {"type": "object", "properties": {
    "name": {"type": "string", "maxLength": 32},
    "age": {"type": "integer"},
    "score": {"type": "number"},
    "tags": {"type": "array", "items": {"enum": ["a", "b", "c"]}, "maxItems": 4},
    "ok": {"type": "boolean"}}}


def sampling(variant: str, new_tokens: int, i: int, prompt) -> SamplingParams:
    kw = dict(temperature=0.2, max_tokens=new_tokens, ignore_eos=True, seed=7 + i)
    if variant == "topkp":
        kw.update(top_p=0.9, top_k=40)
    if "penalty" in variant:
        kw.update(presence_penalty=0.5, frequency_penalty=0.5, repetition_penalty=1.1,
                  logit_bias={int(prompt[0]): 4.0, 3500: -4.0, 7: -100.0})
    if "guided" in variant:
        kw.update(guided_regex=PATTERN)
    return SamplingParams(**kw)


def measure(eng, B: int, ctx: int, new_tokens: int, repeats: int, seed: int = 0) -> dict:
    rng = np.random.default_rng(seed + 1000 * B + ctx)
    vocab = min(eng.model_cfg.vocab_size, 32000)
    prompts = [rng.integers(1000, vocab, size=ctx + int(rng.integers(0, 16))).tolist()
               for _ in range(B)]
    ms = {v: [] for v in VARIANTS}
    for rep in range(-1, repeats):  # rep -1: every variant once, untimed (captures its graphs)
        for v in VARIANTS:
            eng.runner.reset_state()
            sps = [sampling(v, new_tokens, i, p) for i, p in enumerate(prompts)]
            dt, steps = run(eng, prompts, sps, f"{v}-{rep}")
            if rep >= 0:
                ms[v].append(dt / steps * 1e3)
    med = {v: float(np.median(x)) for v, x in ms.items()}
    return {"B": B, "ctx": ctx, "new_tokens": new_tokens,
            "step_ms": {v: [round(x, 4) for x in xs] for v, xs in ms.items()},
            "step_ms_median": {v: round(x, 4) for v, x in med.items()},
            "guided_minus_topkp_us": round((med["guided"] - med["topkp"]) * 1e3, 1),
            "guided_minus_penalty_us": round((med["guided"] - med["penalty"]) * 1e3, 1),
            "both_minus_penalty_us": round((med["guided+penalty"] - med["penalty"]) * 1e3, 1)}


def apply_alone(eng, R: int, calls: int = 20, replays: int = 10) -> dict:
    """ops.guide_apply on R bf16 rows of this model's vocabulary, every row with a slot, the
    slots in the rows of the bench pattern's guide."""
    import torch

    from .. import ops

    r = eng.runner
    r.ensure_guide_state()
    gd, V, dev = r.guide, eng.model_cfg.vocab_size, r.device
    logits = torch.randn(R, V, device=dev).to(torch.bfloat16)
    slots = gd["state"].shape[0]
    slot = torch.arange(R, dtype=torch.int32, device=dev) % slots
    ent = next(iter(r._guide_pool.values()))     # measure() left the bench guide uploaded
    base, n = ent["base"], ent["guide"].num_states
    state = gd["state"].clone()
    state.copy_(base + torch.arange(slots, dtype=torch.int32, device=dev) % n)
    out = gd["logits"][:R]

    def call():
        ops.guide_apply(out, logits, gd["next"], state, slot)

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            call()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls * 1e-3)
    t = float(np.median(times))
    return {"apply_rows": R, "vocab": V, "apply_us": round(t * 1e6, 2),
            "apply_GBps": round(R * V * 8 / t / 1e9, 1)}


def compile_times(eng) -> dict:
    """Host seconds to compile a guide from scratch (pattern -> DFA -> token table), cache
    bypassed, and the first call's one-off cost of listing the tokenizer's bytes."""
    from ..engine.guided import compile_regex, schema_regex, token_table

    t0 = time.perf_counter()
    pieces = eng.tokenizer.token_bytes()
    out = {"vocab": eng.model_cfg.vocab_size,
           "token_bytes_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    for name, pattern in (("regex", PATTERN), ("digits", r"[0-9]{3}-[0-9]{4}"),
                          ("schema5", schema_regex(SCHEMA))):
        t0 = time.perf_counter()
        dfa = compile_regex(pattern)
        t1 = time.perf_counter()
        token_table(dfa, pieces, eng.model_cfg.vocab_size, eng.eos_ids)
        t2 = time.perf_counter()
        out[name] = {"states": dfa.num_states, "dfa_ms": round((t1 - t0) * 1e3, 1),
                     "table_ms": round((t2 - t1) * 1e3, 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="meta-llama/Llama-3.1-8B-Instruct")
    ap.add_argument("--batches", default="1,5,32")
    ap.add_argument("--ctx", type=int, default=600)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--num-kv-blocks", type=int, default=4096)
    ap.add_argument("--pool-states", type=int, default=4096)
    a = ap.parse_args(argv)
    import torch

    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    if not torch.cuda.is_available():
        raise SystemExit("bench/guided.py needs a GPU")
    batches = [int(x) for x in a.batches.split(",")]
    # bench.py's engine configuration, with room for the largest batch
    eng = LLMEngine(EngineConfig(model=a.model, dtype="bfloat16", max_model_len=4096,
                                 max_num_seqs=max(12, max(batches)), max_num_batched_tokens=8192,
                                 use_graphs=True, seed=1234, device="cuda:0",
                                 load_format="dummy", num_kv_blocks=a.num_kv_blocks,
                                 guided_pool_states=a.pool_states))
    print(json.dumps({"compile": compile_times(eng)}), flush=True)
    for b in batches:
        print(json.dumps(measure(eng, b, a.ctx, a.new_tokens, a.repeats)), flush=True)
    for b in batches:
        print(json.dumps(apply_alone(eng, b)), flush=True)


if __name__ == "__main__":
    main()
