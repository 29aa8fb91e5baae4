"""Cost side of speculative decoding: verify-step time against rows, and the acceptance rate
at which n-gram speculation breaks even with plain decode.

What speculation gains depends on how often a real checkpoint repeats its context, which a
random-init model cannot show (its outputs never repeat: the n-gram proposer drafts nothing).
What it costs can be measured: a *replay* proposer drafts from a finished run of the same
requests and makes each draft token right with probability p, so the acceptance rate is set
from outside.  Per shape (batch B, context length) and variant, decode throughput over the
steps after the prefill:

  off       speculation off (an engine of its own: graphs + async look-ahead, today's path)
  nodraft   speculation on, a proposer that never drafts: what losing look-ahead costs - and
            what a workload without repetition pays with the n-gram proposer
  p=0..1    speculation on, k drafts per sequence and step, each right with probability p
            (p = 0: every verify step is wasted rows; p = 1: every draft accepted)

and the verify step's wall time by row count.  The break-even p is where the p-curve crosses
``off`` (linear interpolation between the measured points).  Needs a GPU.

Caveat: the replay only drafts while the live output equals the recorded run.  On random-init
weights (near-flat logits) a verify step's arithmetic flips a near tie within a few steps and
the replay falls silent - ``sequences_off_replay`` counts it, and the p columns then mostly
hold steps without drafts.  ``verify_ms_by_rows`` and off / nodraft stay valid.

    python -m agentic_traffic_testing_amd.bench.specdecode [--model M] [--repeats 3]
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from ..engine.sequence import SamplingParams
from ..engine.spec_decode import Proposer

PS = (0.0, 0.25, 0.5, 0.75, 1.0)


class NoDraft(Proposer):
    def propose(self, seq, k):
        return []


class Replay(Proposer):
    """Drafts k tokens of a finished run of the same request while the live output equals its
    prefix; each token is the run's with probability p, else a wrong one (and everything after
    a wrong token is rejected by the verify step anyway)."""

    def __init__(self, runs: dict, p: float, vocab: int, seed: int = 0):
        self.runs, self.p, self.vocab = runs, p, vocab
        self.rng = np.random.default_rng(seed)
        self.left = set()   # sequences whose live output left the recorded run

    def propose(self, seq, k):
        run = self.runs[seq.request_id.split("/")[-1]]
        n = len(seq.output_ids)
        if seq.output_ids != run[:n]:
            self.left.add(seq.request_id)
            return []
        d = list(run[n:n + k])
        right = self.rng.random(len(d)) < self.p
        return [t if ok else (t + 1) % self.vocab for t, ok in zip(d, right)]


def run(eng, prompts, sps, tag: str):
    """Generate; returns ({short id: tokens}, decode seconds, decode tokens): the clock starts
    once every request has its first token (the prefill steps are not speculation's)."""
    rids = [f"{tag}/r{i}" for i in range(len(prompts))]
    for rid, p, sp in zip(rids, prompts, sps):
        eng.add_request(rid, p, sp)
    done, first, t0, n0 = {}, set(), None, 0
    while eng.has_unfinished():
        outs = eng.step()
        for o in outs:
            first.add(o.request_id)
            if o.finished:
                done[o.request_id.split("/")[-1]] = list(o.token_ids)
        if t0 is None and len(first) == len(rids):
            import torch

            torch.cuda.synchronize()
            t0, n0 = time.perf_counter(), eng.total_generated
    dt = time.perf_counter() - t0
    return done, dt, eng.total_generated - n0


def measure(eng_off, eng_on, B: int, ctx: int, new_tokens: int, repeats: int, seed: int = 0):
    rng = np.random.default_rng(seed + 1000 * B + ctx)
    vocab = min(eng_on.model_cfg.vocab_size, 32000)
    prompts = [rng.integers(1000, vocab, size=ctx + int(rng.integers(0, 16))).tolist()
               for _ in range(B)]
    sps = [SamplingParams(temperature=0.2, max_tokens=new_tokens, ignore_eos=True, seed=7 + i)
           for i in range(B)]
    r = eng_on.runner
    # the run the replay drafts from: this engine, proposer off; also warms every shape
    eng_on.proposer = None
    runs, _, _ = run(eng_on, prompts, sps, "ref")
    run(eng_off, prompts, sps, "warm")
    verify = r.verify
    vtimes: dict[int, list] = {}

    def timed(batch, drafts):
        t = time.perf_counter()
        out = verify(batch, drafts)  # ends in the tokens' D2H copy: the step is complete
        vtimes.setdefault(batch.num_tokens, []).append(time.perf_counter() - t)
        return out

    variants = ["off", "nodraft"] + [f"p={p:g}" for p in PS]
    toks = {v: [] for v in variants}
    stats = {v: [0, 0, 0] for v in variants}
    left = 0
    r.verify = timed
    try:
        for rep in range(-1, repeats):  # rep -1: every variant once, untimed
            for v in variants:
                eng = eng_off if v == "off" else eng_on
                eng.runner.reset_state()
                if v == "nodraft":
                    eng.proposer = NoDraft()
                elif v != "off":
                    eng.proposer = Replay(runs, float(v[2:]), vocab, seed=rep + 1)
                s0 = dict(eng.spec_stats)
                if rep < 0:
                    vtimes.clear()
                _, dt, n = run(eng, prompts, sps, f"{v}-{rep}")
                if rep < 0:
                    vtimes.clear()
                    continue
                toks[v].append(n / dt)
                for j, key in enumerate(("verify_steps", "draft_tokens", "accepted_tokens")):
                    stats[v][j] += eng.spec_stats[key] - s0[key]
                if isinstance(eng.proposer, Replay):
                    left += len(eng.proposer.left)
    finally:
        del r.verify  # the instance attribute: back to the class's method, no cycle left
        eng_on.proposer = None
    med = {v: float(np.median(x)) for v, x in toks.items()}
    curve = [(p, med[f"p={p:g}"]) for p in PS]
    be = None
    for (p0, t0), (p1, t1) in zip(curve, curve[1:]):
        if (t0 - med["off"]) * (t1 - med["off"]) <= 0 and t0 != t1:
            be = p0 + (med["off"] - t0) * (p1 - p0) / (t1 - t0)
            break
    return {
        "B": B, "ctx": ctx, "new_tokens": new_tokens, "k": r.spec_tokens,
        "tok_s": {v: [round(x, 1) for x in xs] for v, xs in toks.items()},
        "tok_s_median": {v: round(x, 1) for v, x in med.items()},
        "spec_stats": {v: dict(zip(("verify_steps", "draft_tokens", "accepted_tokens"), s))
                       for v, s in stats.items() if v != "off"},
        "verify_ms_by_rows": {rows: round(float(np.median(t)) * 1e3, 3)
                              for rows, t in sorted(vtimes.items())},
        "verify_steps_timed": {rows: len(t) for rows, t in sorted(vtimes.items())},
        "lookahead_cost": round(1.0 - med["nodraft"] / med["off"], 4),
        "p0_over_off": round(med["p=0"] / med["off"], 4),
        "break_even_p": None if be is None else round(be, 3),
        "sequences_off_replay": left,
    }


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="meta-llama/Llama-3.1-8B-Instruct")
    ap.add_argument("--batches", default="1,5,7")
    ap.add_argument("--contexts", default="600,3000")
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spec-tokens", type=int, default=3)
    ap.add_argument("--num-kv-blocks", type=int, default=4096)
    a = ap.parse_args(argv)
    import torch

    from ..config import EngineConfig
    from ..engine.llm_engine import LLMEngine

    if not torch.cuda.is_available():
        raise SystemExit("bench/specdecode.py needs a GPU")
    # bench.py's engine configuration; the KV pool is sized by hand so that two engines share
    # the device
    kw = dict(model=a.model, dtype="bfloat16", max_model_len=4096, max_num_seqs=12,
              max_num_batched_tokens=8192, use_graphs=True, seed=1234, device="cuda:0",
              load_format="dummy", num_kv_blocks=a.num_kv_blocks)
    eng_off = LLMEngine(EngineConfig(**kw))
    eng_on = LLMEngine(EngineConfig(speculative="ngram", spec_tokens=a.spec_tokens, **kw))
    for b in (int(x) for x in a.batches.split(",")):
        for ctx in (int(x) for x in a.contexts.split(",")):
            print(json.dumps(measure(eng_off, eng_on, b, ctx, a.new_tokens, a.repeats)),
                  flush=True)


if __name__ == "__main__":
    main()
