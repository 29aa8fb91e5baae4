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

Weights-only mode (``--wide`` / ``--ttft``, both off by default): per projection at M = 48, 96,
128 the wide kernel's 4-bit builds against the 16-bit wide kernel on the pre-shuffled
dequantised copy and against ``ops.expand_mxfp4`` + the library GEMM on the scratch, and the
expand kernel alone in GB/s (0.53 B read + 2 B written per weight) - plain projections, the
same interleaved rounds and cold weight rotation; and at engine level the time to the first
token of an 85-row cached burst, a 475-row burst and a 3000-row prefill, a weights-only engine
against a default-mode mxfp4 engine, alternating per repeat.

One JSON object per line.  Needs a GPU.

    python -m agentic_traffic_testing_amd.bench.w4decode [--kernels 8b,70b] [--engines 8b,70b]
        [--wide 8b,70b] [--ttft 8b]
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


WIDE_ROWS = (48, 96, 128)


def wide_level(size: str, rounds: int, iters: int):
    """The 33-128-row routes of the weights-only mode, per projection (plain GEMM, bf16)."""
    ops.ensure_splitk_workspace("cuda")
    dt = torch.bfloat16
    for proj, n, k in SHAPES[size]:
        w4 = _weights("mxfp4", n, k, max(4, math.ceil(COLD_BYTES / (n * k * 4.25 / 8))))
        w16 = _weights("bf16", n, k, max(4, math.ceil(COLD_BYTES / (n * k * 2))))
        scratch = torch.empty(n, k, dtype=dt, device="cuda")
        for m in WIDE_ROWS:
            x = torch.randn(m, k, dtype=dt, device="cuda")
            out = torch.empty(m, n, dtype=dt, device="cuda")
            i4, i16 = [0], [0]

            def next4():
                i4[0] = (i4[0] + 1) % len(w4)
                return w4[i4[0]][0], w4[i4[0]][1]["w_block_scale"]

            def wide_w4():
                wq, sq = next4()
                ops.linear(x, wq, out=out, w_block_scale=sq, wide_w4=True)

            def wide_16():
                i16[0] = (i16[0] + 1) % len(w16)
                ops.linear(x, w16[i16[0]][0], out=out, preshuffled=True)

            def expand():
                wq, sq = next4()
                ops.expand_mxfp4(wq, sq, "plain", scratch)

            def expand_lib():
                expand()
                torch.mm(x, scratch.t(), out=out)

            calls = {"wide_w4": wide_w4, "wide_16": wide_16, "expand_lib": expand_lib,
                     "expand": expand}
            for name, fn in calls.items():  # warm: code objects, every copy touched
                for _ in range((len(w16) if name == "wide_16" else len(w4)) + 2):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in calls}
            for _ in range(rounds):
                for name, fn in calls.items():  # interleaved: one timing of each per round
                    us[name].append(_time_us(fn, iters))
            rec = {"level": "wide", "model": size, "proj": proj, "N": n, "K": k, "M": m,
                   "rounds": rounds, "iters": iters}
            for name in calls:
                med = statistics.median(us[name])
                rec[name] = {"us": round(med, 2), "min": round(min(us[name]), 2),
                             "max": round(max(us[name]), 2)}
            rec["expand"]["GBps"] = round(n * k * (4.25 / 8 + 2) / rec["expand"]["us"] / 1e3, 1)
            rec["w4_vs_wide16"] = round(rec["wide_16"]["us"] / rec["wide_w4"]["us"], 3)
            rec["w4_vs_expand_lib"] = round(rec["expand_lib"]["us"] / rec["wide_w4"]["us"], 3)
            # slower than the fallback beyond this run's own spread of the fallback's number?
            rec["w4_slower_than_expand_lib"] = bool(rec["wide_w4"]["us"] > rec["expand_lib"]["max"])
            print(json.dumps(rec), flush=True)
        del w4, w16, scratch
        gc.collect()
        torch.cuda.empty_cache()


def _ttft_ms(eng, prompts):
    sp = SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.generate(prompts, sp)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ttft_level(size: str, repeats: int):
    """Time to the first token (one ``generate`` of one-token requests) of the three step
    shapes the weights-only mode routes differently: an 85-row cached burst (5 requests of 17
    new rows behind a cached 592-token prefix: the wide 4-bit kernels), a 475-row burst
    (5 x 95 uncached rows) and a 3000-row prefill (both expand + library).  The default-mode
    mxfp4 engine is the baseline; the two alternate per repeat on fresh random tokens."""
    engs = {"default": _make_engine(size, "mxfp4", 2048),
            "weights_only": _make_engine(size, "mxfp4", 2048, mxfp4_weights_only=True)}
    vocab = min(engs["default"].model_cfg.vocab_size, 32000)
    rng = np.random.default_rng(99)

    def toks(n):
        return rng.integers(1000, vocab, size=n).tolist()

    def cases():
        prefix = toks(592)
        return {"cached_burst_85": (prefix, [prefix + toks(17) for _ in range(5)]),
                "burst_475": (None, [toks(95) for _ in range(5)]),
                "prefill_3000": (None, [toks(3000)])}

    ms = {c: {e: [] for e in engs} for c in cases()}
    for rep in range(-1, repeats):  # rep -1: warm-up, untimed
        for case, (prefix, prompts) in cases().items():
            for name, eng in engs.items():
                eng.runner.reset_state()
                if prefix is not None:
                    _ttft_ms(eng, [prefix])  # leaves the prefix in the cache
                t = _ttft_ms(eng, prompts)
                if rep >= 0:
                    ms[case][name].append(t)
    for case, by in ms.items():
        rec = {"level": "ttft", "model": size, "case": case, "repeats": repeats}
        for name, xs in by.items():
            rec[name] = {"ms": round(statistics.median(xs), 3), "min": round(min(xs), 3),
                         "max": round(max(xs), 3)}
        rec["weights_only_vs_default"] = round(rec["weights_only"]["ms"] / rec["default"]["ms"], 3)
        print(json.dumps(rec), flush=True)
    for name, eng in engs.items():
        print(json.dumps({"level": "ttft", "model": size, "engine": name,
                          "resident_weights": eng.runner.resident_weights,
                          "memory_allocated": torch.cuda.memory_allocated()}), flush=True)


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


def _make_engine(size: str, fmt: str, kv_blocks: int, **extra):
    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    return LLMEngine(EngineConfig(
        model=MODELS[size], dtype="bfloat16", max_model_len=4096, max_num_seqs=12,
        max_num_batched_tokens=8192, use_graphs=True, seed=1234, device="cuda:0",
        load_format="dummy", num_kv_blocks=kv_blocks, quantization="" if fmt == "bf16" else fmt,
        **extra))


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
    ap.add_argument("--wide", default="", help="shape sets of the 33-128-row level ('' off)")
    ap.add_argument("--ttft", default="", help="presets of the weights-only TTFT level ('' off)")
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
    for size in filter(None, a.wide.split(",")):
        wide_level(size, a.rounds, a.iters)
    for size in filter(None, a.ttft.split(",")):
        ttft_level(size, a.repeats)
    for size in filter(None, a.engines.split(",")):
        engine_level(size, [int(b) for b in a.batches.split(",")], a.context, a.new_tokens,
                     a.repeats)


if __name__ == "__main__":
    main()
