"""What MXFP4 W4A8 prefill (``--mxfp4-fp8-activations``) costs and buys: ``ops.gemm_w4a8`` per
projection against the path it replaces, and whole prefill steps with the flag on and off.

Kernel level: for the Llama 8B projection shapes at 160, 475, 1024 and 3070 rows, microseconds
of
  * ``w4a8``        the GEMM alone,
  * ``w4a8_chain``  the GEMM with the row quantiser that feeds it in the chain (norm + quant for
                    qkv / gate_up, plain quant for o / down; gate_up with the SiLU epilogue),
  * ``expand_lib``  what a weights-only step runs today: ``ops.expand_mxfp4`` into the scratch,
                    the library GEMM on it (o / down with the residual add) and the separate
                    RMSNorm / SiLU-mul kernels,
  * ``lib16``       the same without the expand pass: the default mode's step.
Cold weights: the calls rotate over copies totalling >= 768 MB per format (three times the
256 MiB Infinity Cache).  The paths are interleaved - every round times each once - and a line
reports the median and the [min, max] over the rounds.

Step level (``--steps``): time to the first token of one-token requests of 160, 475 (5 x 95),
1024 and 3070 rows on four 8B engines - weights-only and default mode, each with the flag off and
on - alternating per repeat on fresh random tokens.

One JSON object per line.  Needs a GPU.

    python -m agentic_traffic_testing_amd.bench.w4a8prefill [--kernels 8b] [--steps 8b]
"""
from __future__ import annotations

import argparse
import gc
import json
import math
import statistics

import numpy as np
import torch

from .. import ops
from .w4decode import COLD_BYTES, SHAPES, _make_engine, _time_us, _ttft_ms

ROWS = (160, 475, 1024, 3070)
ROWMAPS = {"qkv": "qkv", "o": "plain", "gate_up": "silu", "down": "plain"}
EPS = 1e-5


def kernel_level(size: str, rounds: int, iters: int, rows=ROWS):
    dt = torch.bfloat16
    for proj, n, k in SHAPES[size]:
        copies = max(4, math.ceil(COLD_BYTES / (n * k * 4.25 / 8)))
        w4 = [(torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, device="cuda"),
               torch.randint(120, 128, (n, k // 32), dtype=torch.uint8, device="cuda"))
              for _ in range(copies)]
        w16 = [torch.randn(n, k, dtype=dt, device="cuda") * 0.02
               for _ in range(max(4, math.ceil(COLD_BYTES / (n * k * 2))))]
        scratch = torch.empty(n, k, dtype=dt, device="cuda")
        norm_w = torch.ones(k, dtype=dt, device="cuda")
        silu = proj == "gate_up"
        mode = ops.GEMM_SILU if silu else ops.GEMM_PLAIN
        normed = proj in ("qkv", "gate_up")
        resadd = proj in ("o", "down")
        width = n // 2 if silu else n
        for m in rows:
            x = torch.randn(m, k, dtype=dt, device="cuda")
            xq, xs = ops.quant_rows_fp8(x)
            res = torch.zeros(m, n, dtype=dt, device="cuda") if resadd else None
            out = torch.empty(m, width, dtype=dt, device="cuda")
            i4, i16 = [0], [0]

            def next4():
                i4[0] = (i4[0] + 1) % len(w4)
                return w4[i4[0]]

            def w4a8():
                wq, sq = next4()
                ops.gemm_w4a8(xq, xs, wq, sq, ROWMAPS[proj], mode, out=out)

            def w4a8_chain():
                wq, sq = next4()
                q, s = (ops.quant_rows_fp8(x, ops.QUANT_NORM, norm_w, EPS) if normed
                        else ops.quant_rows_fp8(x))
                ops.gemm_w4a8(q, s, wq, sq, ROWMAPS[proj], mode, out=out)

            def lib(w):
                h = ops.rms_norm(x, norm_w, EPS) if normed else x
                if resadd:
                    ops.linear(h, w, residual=res)
                elif silu:
                    ops.silu_and_mul(ops.linear(h, w))
                else:
                    ops.linear(h, w)

            def expand_lib():
                wq, sq = next4()
                lib(ops.expand_mxfp4(wq, sq, ROWMAPS[proj], scratch))

            def lib16():
                i16[0] = (i16[0] + 1) % len(w16)
                lib(w16[i16[0]])

            calls = {"w4a8": w4a8, "w4a8_chain": w4a8_chain, "expand_lib": expand_lib,
                     "lib16": lib16}
            for name, fn in calls.items():  # warm: code objects, every copy touched
                for _ in range((len(w16) if name == "lib16" else len(w4)) + 2):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in calls}
            for _ in range(rounds):
                for name, fn in calls.items():  # interleaved: one timing of each per round
                    us[name].append(_time_us(fn, iters))
            rec = {"level": "kernel", "model": size, "proj": proj, "N": n, "K": k, "M": m,
                   "rounds": rounds, "iters": iters}
            for name in calls:
                med = statistics.median(us[name])
                rec[name] = {"us": round(med, 2), "min": round(min(us[name]), 2),
                             "max": round(max(us[name]), 2)}
            rec["w4a8"]["TFLOPs"] = round(2.0 * m * n * k / rec["w4a8"]["us"] / 1e6, 1)
            rec["chain_vs_expand_lib"] = round(rec["expand_lib"]["us"] / rec["w4a8_chain"]["us"], 3)
            rec["chain_vs_lib16"] = round(rec["lib16"]["us"] / rec["w4a8_chain"]["us"], 3)
            # slower than the replaced path beyond this run's own spread of that path's number?
            rec["chain_slower_than_expand_lib"] = bool(
                rec["w4a8_chain"]["us"] > rec["expand_lib"]["max"])
            print(json.dumps(rec), flush=True)
        del w4, w16, scratch
        gc.collect()
        torch.cuda.empty_cache()


STEP_CASES = {"prefill_160": (160,), "burst_475": (95,) * 5, "prefill_1024": (1024,),
              "prefill_3070": (3070,)}


def step_level(size: str, repeats: int):
    """Time to the first token (one ``generate`` of one-token requests, every request's rows in
    one step) per case and engine.  ``weights_only`` is the path of the parent commit (expand +
    library), ``default`` the 16-bit copies; ``*_w4a8`` the same with the flag."""
    engs = {"weights_only": _make_engine(size, "mxfp4", 2048, mxfp4_weights_only=True),
            "weights_only_w4a8": _make_engine(size, "mxfp4", 2048, mxfp4_weights_only=True,
                                              mxfp4_fp8_activations=True),
            "default": _make_engine(size, "mxfp4", 2048),
            "default_w4a8": _make_engine(size, "mxfp4", 2048, mxfp4_fp8_activations=True)}
    vocab = min(engs["default"].model_cfg.vocab_size, 32000)
    rng = np.random.default_rng(99)
    ms = {c: {e: [] for e in engs} for c in STEP_CASES}
    for rep in range(-1, repeats):  # rep -1: warm-up, untimed
        for case, lens in STEP_CASES.items():
            prompts = [rng.integers(1000, vocab, size=n).tolist() for n in lens]
            for name, eng in engs.items():
                eng.runner.reset_state()
                t = _ttft_ms(eng, prompts)
                if rep >= 0:
                    ms[case][name].append(t)
    for case, by in ms.items():
        rec = {"level": "step", "model": size, "case": case, "rows": sum(STEP_CASES[case]),
               "repeats": repeats}
        for name, xs in by.items():
            rec[name] = {"ms": round(statistics.median(xs), 3), "min": round(min(xs), 3),
                         "max": round(max(xs), 3)}
        rec["w4a8_vs_weights_only"] = round(
            rec["weights_only"]["ms"] / rec["weights_only_w4a8"]["ms"], 3)
        rec["w4a8_minus_default_ms"] = round(
            rec["weights_only_w4a8"]["ms"] - rec["default"]["ms"], 3)
        print(json.dumps(rec), flush=True)
    for name, eng in engs.items():
        print(json.dumps({"level": "step", "model": size, "engine": name,
                          "plan_475": str(eng.runner.model.step_plan(475)),
                          "resident_weights": eng.runner.resident_weights}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="8b", help="shape sets of the kernel level ('' off)")
    ap.add_argument("--steps", default="8b", help="presets of the step level ('' off)")
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/w4a8prefill.py needs a GPU")
    for size in filter(None, a.kernels.split(",")):
        kernel_level(size, a.rounds, a.iters, tuple(int(r) for r in a.rows.split(",")))
    for size in filter(None, a.steps.split(",")):
        step_level(size, a.repeats)


if __name__ == "__main__":
    main()
