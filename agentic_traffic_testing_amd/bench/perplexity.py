"""Perplexity of a fixed text under each numerics mode of the engine, and how far each mode
moves the per-token logprobs.

    python -m agentic_traffic_testing_amd.bench.perplexity --model M --input FILE
        [--modes bf16,fp8,mxfp4,mxfp4-wo,w4a8] [--window 2048]

FILE is a local text file (tokenised with the model's tokenizer), a ``.npy`` of token ids, or
``synthetic:N[:SEED]`` for N uniformly random ids of the model's vocabulary from numpy's
``default_rng(SEED)`` (the same ids in every mode and on every machine).
The ids are cut into non-overlapping windows of ``--window`` tokens; every window is one request
scored teacher-forced through ``LLMEngine.generate(..., prompt_logprobs=0, max_tokens=1)``: a
window of n tokens yields n - 1 logprobs (its first token has nothing before it).  One engine
per mode, each in a fresh child process.  Output: one JSON line per mode - tokens scored, mean
negative log-likelihood, perplexity = exp(mean NLL) - and for every mode but the first the mean
and max |delta logprob| per token against the first.

Modes: ``bf16`` (no quantisation), ``fp8``, ``mxfp4``, ``mxfp4-wo`` (4-bit weights only) and
``w4a8`` (4-bit weights, fp8 activations on prefill steps).  A preset name or ``--dummy`` gives
random-init weights: the perplexity is then that of noise (about the vocabulary size), but the
deltas are still a real measurement of what each mode does to the numerics of that shape.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

from ..engine.sequence import SamplingParams

MODES = {
    "bf16": {},
    "fp8": {"quantization": "fp8"},
    "mxfp4": {"quantization": "mxfp4"},
    "mxfp4-wo": {"quantization": "mxfp4", "mxfp4_weights_only": True},
    "w4a8": {"quantization": "mxfp4", "mxfp4_fp8_activations": True},
}


def load_ids(path: str, tokenizer=None, vocab: int = 0) -> np.ndarray:
    """Token ids of ``path``: ``synthetic:N[:SEED]`` as seeded random ids below ``vocab``, a
    ``.npy`` of ids as it is, any other file as text."""
    if path.startswith("synthetic:"):
        n, _, seed = path[len("synthetic:"):].partition(":")
        return np.random.default_rng(int(seed or 0)).integers(0, vocab, size=int(n),
                                                              dtype=np.int64)
    if path.endswith(".npy"):
        return np.load(path).astype(np.int64).reshape(-1)
    if tokenizer is None:
        raise ValueError("a text input needs the tokenizer")
    with open(path, encoding="utf-8") as f:
        return np.asarray(tokenizer.encode(f.read()), dtype=np.int64)


def windows(ids, window: int) -> list:
    """Non-overlapping windows of ``window`` ids; a tail of one token scores nothing and is
    dropped."""
    ids = [int(t) for t in ids]
    out = [ids[i:i + window] for i in range(0, len(ids), window)]
    return [w for w in out if len(w) >= 2]


def score_ids(eng, ids, window: int) -> np.ndarray:
    """log p(token | window so far) of every token of ``ids`` but each window's first, in order
    (fp64), through the engine's prompt logprobs."""
    ws = windows(ids, window)
    sp = SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True, prompt_logprobs=0)
    outs = eng.generate(ws, sp)
    lp = []
    for w, o in zip(ws, outs):
        if o.prompt_logprobs is None or len(o.prompt_logprobs) != len(w):
            raise RuntimeError(f"window of {len(w)} tokens came back with "
                               f"{0 if o.prompt_logprobs is None else len(o.prompt_logprobs)} "
                               "entries")
        lp.extend(o.prompt_logprobs[1:])
    return np.asarray(lp, dtype=np.float64)


def summarise(lp: np.ndarray, base: np.ndarray | None = None) -> dict:
    nll = float(-lp.mean())
    out = {"tokens": int(lp.size), "mean_nll": nll, "perplexity": math.exp(nll)}
    if base is not None:
        d = np.abs(lp - base)
        out.update(mean_abs_dlogprob=float(d.mean()), max_abs_dlogprob=float(d.max()))
    return out


def make_engine(mode: str, a):
    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    kw = dict(model=a.model, dtype=a.dtype, device=a.device, max_model_len=a.window + 8,
              max_num_seqs=8, max_num_batched_tokens=max(4096, a.window + 8),
              use_graphs=False, startup_warmup=False, seed=1234,
              enable_prefix_caching=False, **MODES[mode])
    if a.dummy:
        kw["load_format"] = "dummy"
    if a.num_kv_blocks:
        kw["num_kv_blocks"] = a.num_kv_blocks
    return LLMEngine(EngineConfig(**kw))


def child(mode: str, a) -> None:
    """One mode in this process: the scored logprobs go to ``a.child_out`` (.npy)."""
    eng = make_engine(mode, a)
    vocab = eng.model_cfg.vocab_size
    ids = load_ids(a.input, eng.tokenizer, vocab)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise SystemExit(f"{a.input}: ids outside the model's vocabulary of {vocab}")
    np.save(a.child_out, score_ids(eng, ids, a.window))


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="meta-llama/Llama-3.1-8B-Instruct")
    ap.add_argument("--input", required=True)
    ap.add_argument("--modes", default="bf16,fp8,mxfp4,mxfp4-wo,w4a8")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--dummy", action="store_true", help="random-init weights")
    ap.add_argument("--num-kv-blocks", type=int, default=0)
    ap.add_argument("--child-out", default="", help=argparse.SUPPRESS)
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    modes = [m.strip() for m in a.modes.split(",") if m.strip()]
    for m in modes:
        if m not in MODES:
            raise SystemExit(f"unknown mode {m!r}: one of {', '.join(MODES)}")
    if a.window < 2:
        raise SystemExit("--window must be at least 2")
    if a.child_out:
        return child(modes[0], a)
    base = None
    with tempfile.TemporaryDirectory() as tmp:
        for m in modes:
            out = os.path.join(tmp, f"{m}.npy")
            cmd = [sys.executable, "-m", "agentic_traffic_testing_amd.bench.perplexity",
                   "--model", a.model, "--input", a.input, "--modes", m,
                   "--window", str(a.window), "--device", a.device, "--dtype", a.dtype,
                   "--num-kv-blocks", str(a.num_kv_blocks), "--child-out", out]
            if a.dummy:
                cmd.append("--dummy")
            # (the child imports this package from wherever this process found it)
            root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            env = dict(os.environ)
            env["PYTHONPATH"] = os.pathsep.join(filter(None, [root, env.get("PYTHONPATH")]))
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, env=env)
            if r.returncode != 0 or not os.path.exists(out):
                print(json.dumps({"mode": m, "error": f"child exited with {r.returncode}"}),
                      flush=True)
                continue
            lp = np.load(out)
            if base is not None and lp.shape != base.shape:
                print(json.dumps({"mode": m, "error": "token count differs from the first "
                                  "mode's"}), flush=True)
                continue
            print(json.dumps({"mode": m, "model": a.model, "window": a.window,
                              **summarise(lp, base)}), flush=True)
            if base is None:
                base = lp


if __name__ == "__main__":
    main()
