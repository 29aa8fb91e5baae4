"""What scoring a prompt (SamplingParams.prompt_logprobs) costs a prefill step.

One engine (Llama-3.1-8B shape by default, random-init weights, bf16, prefix caching off), one
process.  Per scored-row count n, a prompt of n + 1 tokens is served with max_tokens=1 three ways,
repeats interleaved:

  off           no prompt logprobs: the prefill step samples its one row (the baseline)
  fused         prompt_logprobs=0: ops.lm_head_score per chunk of <= 128 rows, no logits in HBM
  materialised  prompt_logprobs=0 with the fused route switched off: per chunk the LM-head GEMM
                into a [<= 128, vocab] buffer, then ops.token_logprobs

as wall time of the whole request (one prefill step; the host's sync copies of the results are
part of what a request pays).  Then the two routes alone on one 128-row chunk of normalised
hidden states, replayed from a graph so the host's launch cost stays out: time per call, and for
the fused route the achieved bytes/s over the LM-head weights it streams.  Needs a GPU.

    python -m agentic_traffic_testing_amd.bench.scoring [--model M] [--rows 128,475,3070]
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from ..engine.sequence import SamplingParams

VARIANTS = ("off", "fused", "materialised")


def run(eng, prompt, variant: str) -> float:
    import torch

    eng.runner.reset_state()
    eng.runner.score_fused = variant != "materialised"
    sp = SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True,
                        prompt_logprobs=None if variant == "off" else 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate([prompt], sp)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.runner.score_fused = True
    if variant != "off":
        assert len(out.prompt_logprobs) == len(prompt)
    return dt


def measure(eng, rows: int, repeats: int, seed: int = 0) -> dict:
    rng = np.random.default_rng(seed + rows)
    vocab = min(eng.model_cfg.vocab_size, 32000)
    prompt = rng.integers(1000, vocab, size=rows + 1).tolist()
    ms = {v: [] for v in VARIANTS}
    for rep in range(-1, repeats):  # rep -1: every variant once, untimed
        for v in VARIANTS:
            dt = run(eng, prompt, v)
            if rep >= 0:
                ms[v].append(dt * 1e3)
    med = {v: float(np.median(x)) for v, x in ms.items()}
    return {"scored_rows": rows, "launches": -(-rows // eng.runner.model.score_chunk_rows()),
            "request_ms": {v: [round(x, 3) for x in xs] for v, xs in ms.items()},
            "request_ms_median": {v: round(x, 3) for v, x in med.items()},
            "fused_minus_off_ms": round(med["fused"] - med["off"], 3),
            "materialised_minus_off_ms": round(med["materialised"] - med["off"], 3)}


def routes_alone(eng, R: int, calls: int = 10, replays: int = 10) -> dict:
    """LlamaModel.score_rows on R normalised rows, each route, from a graph."""
    import torch

    r = eng.runner
    r.ensure_score_state()
    m = r.model
    dev = r.device
    hidden = torch.randn(R, eng.model_cfg.hidden_size, device=dev).to(r.dtype)
    tgt = torch.randint(0, eng.model_cfg.vocab_size, (R,), dtype=torch.int32, device=dev)
    out = {"rows": R, "vocab": eng.model_cfg.vocab_size}
    for name, fused in (("fused", True), ("materialised", False)):
        def call():
            return m.score_rows(hidden, tgt, 0, r.score_ws or None, fused=fused)

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
        out[name + "_us"] = round(t * 1e6, 1)
        if fused:
            wbytes = eng.model_cfg.vocab_size * eng.model_cfg.hidden_size * 2
            out["fused_weight_GBps"] = round(-(-R // m.score_chunk_rows()) * wbytes / t / 1e9, 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="meta-llama/Llama-3.1-8B-Instruct")
    ap.add_argument("--rows", default="128,475,3070")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--num-kv-blocks", type=int, default=2048)
    a = ap.parse_args(argv)
    import torch

    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    if not torch.cuda.is_available():
        raise SystemExit("bench/scoring.py needs a GPU")
    rows = [int(x) for x in a.rows.split(",")]
    eng = LLMEngine(EngineConfig(model=a.model, dtype="bfloat16", max_model_len=4096,
                                 max_num_seqs=12, max_num_batched_tokens=8192,
                                 use_graphs=True, seed=1234, device="cuda:0",
                                 load_format="dummy", num_kv_blocks=a.num_kv_blocks,
                                 enable_prefix_caching=False))
    for n in rows:
        print(json.dumps(measure(eng, n, a.repeats)), flush=True)
    for n in (128, 32):
        print(json.dumps(routes_alone(eng, n)), flush=True)


if __name__ == "__main__":
    main()
