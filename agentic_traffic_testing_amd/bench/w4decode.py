"""What MXFP4 weights buy at decode: the 4-bit GEMV against the pre-shuffled bf16 and fp8 GEMVs
per projection, and decode tokens/s of the three formats in the engine.

Kernel level: for the Llama 8B and 70B projection shapes at M = 1, 4, 8, 16, 32, microseconds
per ``ops.linear`` call with the production wave counts and cold caches - the calls rotate over
weight copies totalling >= 768 MB per format (three times the 256 MiB Infinity Cache), the
method of scripts/gpu/microbench_gemm.py.  The formats are interleaved: every round times each
format once, and a line reports the median and the [min, max] spread over the rounds, so a
difference can be held against the run's own noise.

Engine level: decode tokens/s over the steps after the prefill at B = 1, 5, 12, the formats
alternating per repeat (8B: bf16, fp8, mxfp4 engines side by side; 70B: fp8 then mxfp4, one at a
time - they do not fit together).

One JSON object per line.  Needs a GPU.

    python -m agentic_traffic_testing_amd.bench.w4decode [--kernels 8b,70b] [--engines 8b,70b]
"""
from __future__ import annotations

import argparse
import gc
import json
import math
import statistics
import time

import numpy as np
import torch

from .. import ops
from ..engine.sequence import SamplingParams

SHAPES = {
    "8b": [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096),
           ("down", 4096, 14336)],
    "70b": [("qkv", 10240, 8192), ("o", 8192, 8192), ("gate_up", 57344, 8192),
            ("down", 8192, 28672)],
}
ROWS = (1, 4, 8, 16, 32)
FORMATS = ("bf16", "fp8", "mxfp4")
BITS = {"bf16": 16.0, "fp8": 8.0, "mxfp4": 4.25}
MODELS = {"8b": "meta-llama/Llama-3.1-8B-Instruct", "70b": "llama-3-70b"}
COLD_BYTES = 768e6


def _weights(fmt: str, n: int, k: int, copies: int):
    """``copies`` random weights of one format as (w, kwargs of ops.linear); the values do not
    matter for the timing, the layouts and sizes do."""
    out = []
    for _ in range(copies):
        if fmt == "mxfp4":
            wq = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device="cuda")
            sq = torch.randint(120, 128, (n, k // 32), dtype=torch.uint8, device="cuda")
            out.append((wq, {"w_block_scale": sq}))
            continue
        w = torch.randn(n, k, dtype=torch.bfloat16, device="cuda") * 0.02
        if fmt == "fp8":
            q, sc = ops.quantize_fp8(w)
            out.append((ops.preshuffle_fp8(q), {"w_scale": sc}))
        else:
            out.append((ops.preshuffle(w), {"preshuffled": True}))
        del w
    return out


def _time_us(fn, iters: int) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000.0


def kernel_level(size: str, rounds: int, iters: int):
    ops.ensure_splitk_workspace("cuda")
    for proj, n, k in SHAPES[size]:
        ws = {f: _weights(f, n, k, max(4, math.ceil(COLD_BYTES / (n * k * BITS[f] / 8))))
              for f in FORMATS}
        for m in ROWS:
            x = torch.randn(m, k, dtype=torch.bfloat16, device="cuda")
            out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
            calls = {}
            for f in FORMATS:
                waves = ops.decode_waves(proj, True, f == "fp8", m=m, mxfp4=f == "mxfp4")
                i = [0]

                def call(f=f, waves=waves, i=i):
                    i[0] = (i[0] + 1) % len(ws[f])
                    w, kw = ws[f][i[0]]
                    ops.linear(x, w, out=out, waves=waves, ksplit=None, proj=proj, **kw)

                calls[f] = call
                for _ in range(len(ws[f]) + 2):  # warm: code objects, every copy touched
                    call()
            torch.cuda.synchronize()
            us = {f: [] for f in FORMATS}
            for _ in range(rounds):
                for f in FORMATS:  # interleaved: one timing of each format per round
                    us[f].append(_time_us(calls[f], iters))
            rec = {"level": "kernel", "model": size, "proj": proj, "N": n, "K": k, "M": m,
                   "rounds": rounds, "iters": iters}
            for f in FORMATS:
                med = statistics.median(us[f])
                rec[f] = {"us": round(med, 2), "min": round(min(us[f]), 2),
                          "max": round(max(us[f]), 2),
                          "GBps": round(n * k * BITS[f] / 8 / med / 1e3, 1),
                          "kernel": ops.fused_kernel(m, True, f == "fp8", mxfp4=f == "mxfp4")}
            lo8, hi8 = rec["fp8"]["min"], rec["fp8"]["max"]
            rec["mxfp4_vs_fp8"] = round(rec["fp8"]["us"] / rec["mxfp4"]["us"], 3)
            # slower than fp8 beyond this run's own spread of the fp8 number?
            rec["mxfp4_slower_than_fp8"] = bool(rec["mxfp4"]["us"] > hi8)
            rec["fp8_spread_us"] = round(hi8 - lo8, 2)
            print(json.dumps(rec), flush=True)
        del ws
        gc.collect()
        torch.cuda.empty_cache()


def _decode_tok_s(eng, prompts, sps, tag: str):
    """Decode tokens/s over the steps after every request has its first token."""
    for i, (p, sp) in enumerate(zip(prompts, sps)):
        eng.add_request(f"{tag}/r{i}", p, sp)
    first, t0, n0 = set(), None, 0
    while eng.has_unfinished():
        for o in eng.step():
            first.add(o.request_id)
        if t0 is None and len(first) == len(prompts):
            torch.cuda.synchronize()
            t0, n0 = time.perf_counter(), eng.total_generated
    torch.cuda.synchronize()
    return (eng.total_generated - n0) / (time.perf_counter() - t0)


def _make_engine(size: str, fmt: str, kv_blocks: int):
    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    return LLMEngine(EngineConfig(
        model=MODELS[size], dtype="bfloat16", max_model_len=4096, max_num_seqs=12,
        max_num_batched_tokens=8192, use_graphs=True, seed=1234, device="cuda:0",
        load_format="dummy", num_kv_blocks=kv_blocks, quantization="" if fmt == "bf16" else fmt))


def _workload(eng, B: int, ctx: int, new_tokens: int):
    rng = np.random.default_rng(1000 * B + ctx)
    vocab = min(eng.model_cfg.vocab_size, 32000)
    prompts = [rng.integers(1000, vocab, size=ctx + int(rng.integers(0, 16))).tolist()
               for _ in range(B)]
    sps = [SamplingParams(temperature=0.0, max_tokens=new_tokens, ignore_eos=True)
           for _ in range(B)]
    return prompts, sps


def _engine_record(size, B, ctx, new_tokens, toks, engines):
    rec = {"level": "engine", "model": size, "B": B, "ctx": ctx, "new_tokens": new_tokens}
    for f, xs in toks.items():
        m = engines[f]
        rec[f] = {"tok_s": round(statistics.median(xs), 1), "min": round(min(xs), 1),
                  "max": round(max(xs), 1), "preshuffled_16bit": m[0], "graph_steps": m[1]}
    if "fp8" in toks and "mxfp4" in toks:
        rec["mxfp4_vs_fp8"] = round(rec["mxfp4"]["tok_s"] / rec["fp8"]["tok_s"], 3)
    print(json.dumps(rec), flush=True)


def engine_level(size: str, batches, ctx: int, new_tokens: int, repeats: int):
    fmts = FORMATS if size == "8b" else ("fp8", "mxfp4")
    together = size == "8b"
    toks = {B: {f: [] for f in fmts} for B in batches}
    info = {}

    def facts(eng):
        return (eng.runner.model.layers[0].qkv_ps is not None, eng.runner.graph_steps)

    if together:  # engines side by side, formats alternating per repeat
        engs = {f: _make_engine(size, f, 2048) for f in fmts}
        for B in batches:
            prompts, sps = _workload(engs[fmts[0]], B, ctx, new_tokens)
            for rep in range(-1, repeats):  # rep -1: warm-up, untimed
                for f in fmts:
                    engs[f].runner.reset_state()
                    t = _decode_tok_s(engs[f], prompts, sps, f"{f}-{B}-{rep}")
                    if rep >= 0:
                        toks[B][f].append(t)
        info = {f: facts(e) for f, e in engs.items()}
    else:  # one engine at a time
        for f in fmts:
            eng = _make_engine(size, f, 1024)
            for B in batches:
                prompts, sps = _workload(eng, B, ctx, new_tokens)
                for rep in range(-1, repeats):
                    eng.runner.reset_state()
                    t = _decode_tok_s(eng, prompts, sps, f"{f}-{B}-{rep}")
                    if rep >= 0:
                        toks[B][f].append(t)
            info[f] = facts(eng)
            del eng
            gc.collect()
            torch.cuda.empty_cache()
    for B in batches:
        _engine_record(size, B, ctx, new_tokens, toks[B], info)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="8b,70b", help="shape sets of the kernel level ('' off)")
    ap.add_argument("--engines", default="8b,70b", help="presets of the engine level ('' off)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--batches", default="1,5,12")
    ap.add_argument("--context", type=int, default=600)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/w4decode.py needs a GPU")
    for size in filter(None, a.kernels.split(",")):
        kernel_level(size, a.rounds, a.iters)
    for size in filter(None, a.engines.split(",")):
        engine_level(size, [int(b) for b in a.batches.split(",")], a.context, a.new_tokens,
                     a.repeats)


if __name__ == "__main__":
    main()
