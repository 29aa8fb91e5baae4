"""Speculative decoding: n-gram drafts verified in one decode step (engine/spec_decode.py,
LLMEngine._drafts / _verify_step, ModelRunner.verify).

Sampling is a pure function of (logits, seed, step, token id), so speculation may change how
many steps a generation takes and nothing else.  The CPU tier holds the engine to that: with
speculation on, every run equals the run without it token for token and finish reason for
finish reason, under proposers that are always right (a replay of the spec-off run), always
wrong, and in between.  The GPU tier checks the verify step's tokens against the fp32 dense
oracle, teacher-forced at every position, like tests/test_engine.py.
"""
import gc

import numpy as np
import pytest
import torch

from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.engine.spec_decode import NgramProposer, Proposer
from agentic_traffic_testing_amd.ops import reference as ref

from helpers import dense_logits, dense_logits_fp8

VOCAB = 4096  # tiny


# ---- proposers the tests inject -------------------------------------------------------------
class ReplayProposer(Proposer):
    """Drafts from a finished run of the same requests (by request id), for as long as the
    live output still equals that run's prefix.  ``keep`` < 1 cuts each draft at a seeded
    random length; ``corrupt_every`` = m makes every m-th draft token wrong; ``wrong`` makes
    all of them wrong; ``skip_every`` = m answers every m-th call with no draft (so the
    sequences of one verify step differ in qlen whatever k is)."""

    def __init__(self, runs: dict, keep: float = 1.0, corrupt_every: int = 0, wrong: bool = False,
                 vocab: int = VOCAB, seed: int = 0, skip_every: int = 0):
        self.runs, self.keep, self.corrupt_every, self.wrong = runs, keep, corrupt_every, wrong
        self.vocab, self.skip_every = vocab, skip_every
        self.rng = np.random.default_rng(seed)
        self.count = self.calls = 0

    def propose(self, seq, k):
        run = self.runs[seq.request_id]
        n = len(seq.output_ids)
        if k <= 0 or seq.output_ids != run[:n]:
            return []
        self.calls += 1
        if self.skip_every and self.calls % self.skip_every == 0:
            return []
        d = list(run[n:n + k])
        if self.keep < 1.0:
            m = 0
            while m < len(d) and self.rng.random() < self.keep:
                m += 1
            d = d[:m]
        for i in range(len(d)):
            self.count += 1
            if self.wrong or (self.corrupt_every and self.count % self.corrupt_every == 0):
                d[i] = (d[i] + 1) % self.vocab
        return d


class _Seq:
    def __init__(self, ids):
        self._a = np.asarray(ids, dtype=np.int64)

    def token_array(self):
        return self._a


def run_engine(eng, prompts, sps, admit_at=None):
    """Drive ``eng`` step by step; request i ("r<i>") is added before step ``admit_at[i]``
    (default: all up front).  Returns {request id: dict(tokens, reason, streamed, cached)} and
    the number of steps; checks per-token accounting and that every KV block came back."""
    if not isinstance(sps, list):
        sps = [sps] * len(prompts)
    admit_at = admit_at or [0] * len(prompts)
    g0 = eng.total_generated
    res, streamed, step = {}, {}, 0
    pending = sorted(range(len(prompts)), key=lambda i: admit_at[i])
    while pending or eng.has_unfinished():
        while pending and admit_at[pending[0]] <= step:
            i = pending.pop(0)
            eng.add_request(f"r{i}", prompts[i], sps[i])
        for o in eng.step():
            streamed.setdefault(o.request_id, []).extend(o.new_token_ids)
            assert o.token_ids == streamed[o.request_id], "new_token_ids must stream every token"
            assert o.first_token_time is not None
            if o.finished:
                res[o.request_id] = dict(tokens=list(o.token_ids), reason=o.finish_reason,
                                         cached=o.cached_prompt_tokens)
        step += 1
        assert step < 10000
    assert len(res) == len(prompts)
    assert eng.total_generated - g0 == sum(len(r["tokens"]) for r in res.values())
    info = eng.kv_cache_info()
    assert info["free_blocks"] == info["num_gpu_blocks"], "KV blocks leaked"
    return res, step


def cpu_engine(spec="ngram", **kw):
    base = dict(model="tiny", device="cpu", max_model_len=256, num_kv_blocks=64,
                max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False, speculative=spec)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def runs_of(res):
    return {rid: r["tokens"] for rid, r in res.items()}


def same(a, b):
    assert {k: (v["tokens"], v["reason"]) for k, v in a.items()} == \
           {k: (v["tokens"], v["reason"]) for k, v in b.items()}


def simulate(propose, prompt, out, k_max, max_tokens, max_model_len):
    """(verify steps, drafts, accepted, engine steps) of one sequence generating ``out`` alone:
    the first token comes from the prefill step, every later step drafts with ``propose``."""
    n, steps, vsteps, drafts, acc = 1, 1, 0, 0, 0
    P = len(prompt)
    while n < len(out):
        k = min(k_max, max_tokens - n - 1, max_model_len - (P + n) - 1)
        d = propose(list(prompt) + list(out[:n]), k) if k > 0 else []
        a = 0
        while a < len(d) and d[a] == out[n + a]:
            a += 1
        vsteps += bool(d)
        drafts += len(d)
        acc += a
        n += a + 1
        steps += 1
    return vsteps, drafts, acc, steps


def _loop_prompts():
    rng = np.random.default_rng(0)
    blk = rng.integers(300, 3000, size=12).tolist()
    return [blk * 4, blk * 4 + [5, 6, 7], rng.integers(300, 3000, size=40).tolist()]


# =========================================================================================
# CPU tier
# =========================================================================================
def test_ngram_proposer():
    p = NgramProposer(4, 2)
    look = lambda ids, k: p.propose(_Seq(ids), k)  # noqa: E731
    assert look([1, 2, 3, 4, 5, 6, 7, 8], 3) == []                      # no match
    assert look([9, 9], 3) == [] and look([7], 3) == [] and look([], 2) == []
    # longest n wins: the 4-gram [1 2 3 4] (-> 50) beats the more recent 2-gram [3 4] (-> 60)
    assert look([1, 2, 3, 4, 50, 51, 8, 3, 4, 60, 61, 1, 2, 3, 4], 2) == [50, 51]
    # most recent occurrence wins
    assert look([3, 4, 10, 11, 3, 4, 20, 21, 5, 3, 4], 2) == [20, 21]
    # continuation clipped at the end of the sequence
    assert look([5, 6, 7, 5, 6], 4) == [7, 5, 6]
    assert look([5, 6, 5, 6], 4) == [5, 6]
    assert look([1, 2, 3, 1, 2, 3], 0) == []                             # k = 0
    assert look([1, 2, 3, 1, 2, 3], 1) == [1]
    # n_min: a 1-gram match alone drafts nothing at n_min = 2, something at n_min = 1
    assert look([4, 8, 9, 4], 2) == []
    assert NgramProposer(4, 1).propose(_Seq([4, 8, 9, 4]), 2) == [8, 9]
    with pytest.raises(ValueError):
        NgramProposer(2, 3)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_greedy_loops_equal_plain_decode(which):
    """Greedy prompts that loop (a 12-token block four times, the same with a tail, a random
    prompt): the n-gram proposer drafts, the accepted count is the one a simulation of the
    proposer over the spec-off output gives, and the tokens are those of plain decode."""
    prompt = _loop_prompts()[which]
    sp = SamplingParams(temperature=0.0, max_tokens=96, ignore_eos=True)
    off, steps_off = run_engine(cpu_engine(""), [prompt], sp)
    eng = cpu_engine()
    on, steps_on = run_engine(eng, [prompt], sp)
    same(off, on)
    k = eng.runner.spec_tokens
    assert k == 3
    prop = NgramProposer(4, 2)
    v, d, a, s = simulate(lambda ids, kk: prop.lookup(np.asarray(ids), kk), prompt,
                          off["r0"]["tokens"], k, 96, 256)
    print(f"loop prompt {which}: {a} of {d} drafts accepted in 96 tokens, {s} steps")
    assert eng.spec_stats == {"verify_steps": v, "draft_tokens": d, "accepted_tokens": a}
    assert a > 0 and steps_on == s == steps_off - a


@pytest.mark.parametrize("temp", [0.7, 0.2])
def test_seeded_rows_replay_all_accepted(temp):
    """Seeded sampling rows under the replay proposer: every draft is accepted and the step
    count is the arithmetic one."""
    rng = np.random.default_rng(1)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (33, 9)]
    sps = [SamplingParams(temperature=temp, max_tokens=n, ignore_eos=True, seed=11 + i)
           for i, n in enumerate((41, 30))]
    off, _ = run_engine(cpu_engine(""), prompts, sps)
    eng = cpu_engine()
    eng.proposer = ReplayProposer(runs_of(off))
    on, steps = run_engine(eng, prompts, sps)
    same(off, on)
    st = eng.spec_stats
    # per sequence: the prefill step gives one token, every later step 1 + min(3, what is
    # left - 1); both prefill in step 0, so the run takes the longer sequence's steps
    sims = [simulate(lambda ids, k, r=off[f"r{i}"]["tokens"], p=prompts[i]:
                     r[len(ids) - len(p):len(ids) - len(p) + k],
                     prompts[i], off[f"r{i}"]["tokens"], 3, sps[i].max_tokens, 256)
            for i in range(2)]
    assert st["draft_tokens"] == st["accepted_tokens"] == sum(x[2] for x in sims)
    assert st["accepted_tokens"] == (41 - 1 - sims[0][3] + 1) + (30 - 1 - sims[1][3] + 1)
    assert steps == max(x[3] for x in sims) == 1 + -(-(41 - 1) // 4)


def test_always_wrong_proposer():
    rng = np.random.default_rng(2)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (20, 31, 5)]
    sp = SamplingParams(temperature=0.7, max_tokens=24, ignore_eos=True, seed=3)
    off, steps_off = run_engine(cpu_engine(""), prompts, sp)
    eng = cpu_engine()
    eng.proposer = ReplayProposer(runs_of(off), wrong=True)
    on, steps_on = run_engine(eng, prompts, sp)
    same(off, on)
    assert eng.spec_stats["accepted_tokens"] == 0 and eng.spec_stats["draft_tokens"] > 0
    assert steps_on == steps_off  # one token per sequence and step


@pytest.mark.parametrize("seed", [0, 1])
def test_random_truncation_and_corruption(seed):
    rng = np.random.default_rng(4 + seed)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (18, 40, 7, 64)]
    sps = [SamplingParams(temperature=t, max_tokens=40, ignore_eos=True, seed=20 + i)
           for i, t in enumerate((0.0, 0.7, 0.2, 0.0))]
    off, steps_off = run_engine(cpu_engine(""), prompts, sps)
    eng = cpu_engine()
    eng.proposer = ReplayProposer(runs_of(off), keep=0.6, corrupt_every=5, seed=seed)
    on, steps_on = run_engine(eng, prompts, sps)
    same(off, on)
    st = eng.spec_stats
    assert 0 < st["accepted_tokens"] < st["draft_tokens"] and steps_on < steps_off


def test_stop_token_inside_accepted_run():
    rng = np.random.default_rng(6)
    prompt = rng.integers(300, 3000, size=25).tolist()
    free = SamplingParams(temperature=0.7, max_tokens=40, ignore_eos=True, seed=5)
    base, _ = run_engine(cpu_engine(""), [prompt], free)
    toks = base["r0"]["tokens"]
    # a token whose first occurrence falls in the middle of a 4-token run (runs start at
    # output 1, 5, 9, ...) under full acceptance
    idx = next(i for i in range(6, 40) if (i - 1) % 4 in (1, 2) and toks.index(toks[i]) == i)
    sp = SamplingParams(temperature=0.7, max_tokens=40, seed=5, stop_token_ids=(toks[idx],))
    off, _ = run_engine(cpu_engine(""), [prompt], sp)
    assert off["r0"]["reason"] == "stop" and len(off["r0"]["tokens"]) <= idx + 1
    eng = cpu_engine()
    eng.proposer = ReplayProposer({"r0": toks})  # drafts run past the stop token
    on, _ = run_engine(eng, [prompt], sp)
    same(off, on)
    assert eng.spec_stats["accepted_tokens"] > 0


def test_max_tokens_and_max_model_len():
    rng = np.random.default_rng(7)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (30, 120)]
    # max_tokens 7 = 1 + 4 + 2: the third step may draft one token only; the 120-token prompt
    # reaches max_model_len = 128 after 8 tokens
    sps = [SamplingParams(temperature=0.0, max_tokens=7, ignore_eos=True),
           SamplingParams(temperature=0.7, max_tokens=50, ignore_eos=True, seed=1)]
    kw = dict(max_model_len=128, max_num_batched_tokens=128)
    long = SamplingParams(temperature=0.0, max_tokens=50, ignore_eos=True)
    ref_runs, _ = run_engine(cpu_engine("", max_model_len=256), prompts,
                             [long, SamplingParams(temperature=0.7, max_tokens=50,
                                                   ignore_eos=True, seed=1)])
    off, _ = run_engine(cpu_engine("", **kw), prompts, sps)
    assert [len(off[r]["tokens"]) for r in ("r0", "r1")] == [7, 8]
    assert off["r0"]["reason"] == off["r1"]["reason"] == "length"
    eng = cpu_engine(**kw)
    eng.proposer = ReplayProposer(runs_of(ref_runs))  # drafts past both limits are on offer
    on, _ = run_engine(eng, prompts, sps)
    same(off, on)
    assert eng.spec_stats["accepted_tokens"] == eng.spec_stats["draft_tokens"] > 0


def test_preemption_with_speculation():
    """A 16-block KV pool forces preemption / recompute; drafts never preempt (a sequence
    whose drafts do not fit gets none) and outputs stay exact."""
    kw = dict(max_model_len=128, num_kv_blocks=16, max_num_batched_tokens=128,
              enable_prefix_caching=False)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(300, 3000, size=60).tolist() for _ in range(3)]
    sp = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True)
    e0 = cpu_engine("", **kw)
    off, _ = run_engine(e0, prompts, sp)
    eng = cpu_engine(**kw)
    eng.proposer = ReplayProposer(runs_of(off))
    on, _ = run_engine(eng, prompts, sp)
    same(off, on)
    assert eng.scheduler.num_preemptions > 0 and e0.scheduler.num_preemptions > 0
    assert eng.spec_stats["accepted_tokens"] > 0


def test_mid_run_admission_and_prefix_cache():
    """Requests admitted while others are in verify steps, and a follow-up request that shares
    a finished request's prompt + output: same tokens and the same cached_prompt_tokens as
    without speculation (the prefix cache holds accepted tokens only)."""
    rng = np.random.default_rng(8)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (40, 22, 35)]
    sps = [SamplingParams(temperature=t, max_tokens=36, ignore_eos=True, seed=30 + i)
           for i, t in enumerate((0.0, 0.7, 0.0))]
    e0 = cpu_engine("")
    off, _ = run_engine(e0, prompts, sps)
    eng = cpu_engine()
    eng.proposer = ReplayProposer(runs_of(off), corrupt_every=7)
    on, _ = run_engine(eng, prompts, sps, admit_at=[0, 3, 5])
    same(off, on)
    assert eng.spec_stats["accepted_tokens"] > 0
    follow = prompts[0] + off["r0"]["tokens"] + [5, 6, 7]
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    f0, _ = run_engine(e0, [follow], sp)
    eng.proposer = ReplayProposer(runs_of(f0))
    f1, _ = run_engine(eng, [follow], sp)
    same(f0, f1)
    assert f1["r0"]["cached"] == f0["r0"]["cached"] == (len(follow) - 4) // 16 * 16


def test_row_cap_trims_longest_draft_first():
    """More rows than the verify step takes: drafts are trimmed one token at a time from the
    longest, lowest batch index first."""
    eng = cpu_engine(max_num_seqs=4)
    eng.runner._verify_rows = 9
    rng = np.random.default_rng(9)
    prompts = [rng.integers(300, 3000, size=n).tolist() for n in (10, 11, 12)]
    sp = SamplingParams(temperature=0.0, max_tokens=30, ignore_eos=True)
    off, _ = run_engine(cpu_engine(""), prompts, sp)
    eng.proposer = ReplayProposer(runs_of(off))
    seen = []
    verify = eng.runner.verify

    def spy(batch, drafts):
        seen.append([len(d) for d in drafts])
        return verify(batch, drafts)

    eng.runner.verify = spy
    try:
        on, _ = run_engine(eng, prompts, sp)
    finally:
        del eng.runner.verify  # back to the class's method, no reference cycle left behind
    same(off, on)
    assert seen[0] == [2, 2, 2] and all(sum(s) + len(s) <= 9 for s in seen)


def test_config():
    with pytest.raises(ValueError):
        EngineConfig(model="tiny", device="cpu", speculative="ngram", tensor_parallel_size=2)
    with pytest.raises(ValueError):
        EngineConfig(model="tiny", device="cpu").replace(speculative="ngram",
                                                         tensor_parallel_size=2)
    with pytest.raises(ValueError):
        EngineConfig(model="tiny", device="cpu", speculative="medusa")
    assert EngineConfig().speculative == "" and EngineConfig().spec_tokens == 3
    eng = cpu_engine(spec_tokens=99)
    g = eng.runner.model.g
    assert eng.runner.spec_tokens == 16 // g - 1
    off = cpu_engine("")
    assert off.proposer is None and off.runner.spec_tokens == 0 and off.runner.verify_rows() == 0
    assert off.runner.ws_rows == off.runner.max_seqs


def test_serve_llm_flags_and_counters(monkeypatch):
    from agentic_traffic_testing_amd.serving import serve_llm
    from agentic_traffic_testing_amd.serving.metrics import LLMMetrics

    args = serve_llm.make_parser().parse_args(
        ["--model", "tiny", "--device", "cpu", "--speculative", "ngram",
         "--num-speculative-tokens", "2"])
    cfg = serve_llm.build_config(args)
    assert cfg.speculative == "ngram" and cfg.spec_tokens == 2
    monkeypatch.setenv("LLM_SPECULATIVE", "ngram")
    monkeypatch.setenv("LLM_NUM_SPECULATIVE_TOKENS", "5")
    args = serve_llm.make_parser().parse_args(["--model", "tiny", "--device", "cpu"])
    cfg = serve_llm.build_config(args)
    assert cfg.speculative == "ngram" and cfg.spec_tokens == 5
    args = serve_llm.make_parser().parse_args(["--model", "tiny", "--speculative", "off"])
    assert serve_llm.build_config(args).speculative == ""
    m = LLMMetrics(process_collectors=False)
    m.sync_spec({"verify_steps": 3, "draft_tokens": 9, "accepted_tokens": 4})
    m.sync_spec({"verify_steps": 5, "draft_tokens": 12, "accepted_tokens": 4})
    text = m.exposition().decode()
    assert "llm_spec_verify_steps_total 5.0" in text
    assert "llm_spec_draft_tokens_total 12.0" in text
    assert "llm_spec_accepted_tokens_total 4.0" in text


# =========================================================================================
# GPU tier
# =========================================================================================
TOL_LOGIT = 0.25  # the near-tie bound of the GPU engine tests


def _oracle_check(eng, prompts, sps, res, fp8=False):
    """Teacher-forced at every generated position: the engine's token is the fp32 oracle's
    (argmax for greedy rows, ops.reference.sample's for seeded rows) or a near tie - logit gap
    (greedy) / score gap times T (seeded) below TOL_LOGIT - and at most one position in five
    diverges."""
    m = eng.runner.model
    bad = checked = 0
    for i, (p, sp) in enumerate(zip(prompts, sps)):
        toks = res[f"r{i}"]["tokens"]
        assert len(toks) == sp.max_tokens
        seed = eng_seed = sp.seed
        ids = list(p)
        for step, got in enumerate(toks):
            lg = dense_logits_fp8(m, ids, len(p)) if fp8 else dense_logits(m, ids)
            lg = lg.float().cpu()
            checked += 1
            if sp.temperature > 1e-5:
                sc = ref._sample_scores(lg[None], 0, [sp.temperature], [seed], [step], 0)
                want, gap = int(torch.argmax(sc)), float(sc.max() - sc[got]) * sp.temperature
            else:
                want, gap = int(torch.argmax(lg)), float(lg.max() - lg[got])
            if want != got:
                assert gap < TOL_LOGIT, (i, step, got, want, gap)
                bad += 1
            ids.append(got)
        del eng_seed
    assert bad <= max(1, checked // 5), (bad, checked)
    return bad, checked


GPU_CASES = [("small", "", 4, 3, 30000), ("llama-70b-slice", "", 8, 1, 16000),
             ("llama-3b-slice", "", 3, 4, 16000), ("small", "fp8", 4, 3, 30000)]


@pytest.mark.gpu
@pytest.mark.parametrize("model,quant,g,k,vocab", GPU_CASES,
                         ids=[f"{c[0]}{'-' + c[1] if c[1] else ''}" for c in GPU_CASES])
def test_gpu_verify_steps_match_oracle(model, quant, g, k, vocab):
    """Replay drafts (from a run of the same engine with the proposer off) through verify
    steps: a clean run and one with every third draft corrupted.  Greedy and seeded rows, a
    context past two attention partitions, staggered admission (16-bit weights), mixed qlen."""
    fp8 = quant == "fp8"
    gc.collect()  # engines of earlier tests go now, not while this one captures a hipGraph
    cfg = EngineConfig(model=model, device="cuda", max_model_len=512, num_kv_blocks=512,
                       max_num_batched_tokens=2048 if fp8 else 128, max_num_seqs=8,
                       graph_batch_sizes=(1, 2, 4, 8), quantization=quant, speculative="ngram",
                       spec_tokens=4)
    eng = LLMEngine(cfg)
    r = eng.runner
    assert r.model.g == g and r.spec_tokens == k
    assert 1 < r.verify_rows() <= (32 if fp8 else 128)
    rng = np.random.default_rng(0)
    # 300 tokens: three 128-token partitions at this batch size
    prompts = [rng.integers(300, vocab, size=n).tolist() for n in (40, 300, 17, 1, 70)]
    sps = [SamplingParams(temperature=t, max_tokens=n, ignore_eos=True, seed=40 + i)
           for i, (t, n) in enumerate(((0.0, 12), (0.0, 10), (0.7, 12), (0.2, 9), (0.0, 11)))]
    # every prompt of the fp8 case prefills in the first step (the oracle does not model a
    # decode row inside a quantised prefill forward)
    admit = None if fp8 else [0, 0, 2, 4, 4]
    live, eng.proposer = eng.proposer, None
    base, steps_off = run_engine(eng, prompts, sps, admit_at=admit)
    assert eng.spec_stats["verify_steps"] == 0 and isinstance(live, NgramProposer)
    seen = []
    verify = r.verify

    def spy(batch, drafts):
        out = verify(batch, drafts)
        acc = []
        for d, s in zip(drafts, out):
            a = 0
            while a < len(d) and d[a] == int(s[a]):
                a += 1
            acc.append(a)
        seen.append((list(batch.q_len), acc))
        return out

    # the wrapper holds a bound method of the runner: installed on the instance it closes a
    # reference cycle, and an engine left to the cycle collector may have its hipGraphs
    # destroyed while a later engine is capturing one (a HIP error inside a destructor: the
    # process aborts).  The wrapper comes off again below, so the engine dies with this frame.
    r.verify = spy
    try:
        for name, corrupt in (("replay", 0), ("corrupt-every-3rd", 3)):
            r.reset_state()
            eng.proposer = ReplayProposer(runs_of(base), corrupt_every=corrupt, vocab=vocab,
                                          skip_every=4)
            st0 = dict(eng.spec_stats)
            del seen[:]
            res, steps_on = run_engine(eng, prompts, sps, admit_at=admit)
            bad, checked = _oracle_check(eng, prompts, sps, res, fp8)
            d = eng.spec_stats["draft_tokens"] - st0["draft_tokens"]
            a = eng.spec_stats["accepted_tokens"] - st0["accepted_tokens"]
            equal = sum(res[k_]["tokens"] == base[k_]["tokens"] for k_ in res)
            print(f"SPEC {model}{quant and '-' + quant} {name}: {a} of {d} drafts accepted, "
                  f"{steps_on} steps vs {steps_off} plain, {len(seen)} verify steps, {bad} of "
                  f"{checked} positions off the oracle's token, {equal} of {len(res)} sequences "
                  "equal to the plain run")
            assert seen and d > 0
            assert any(len(set(ql)) > 1 for ql, _ in seen), "no verify step with mixed qlen"
            full = any(q - 1 == k and acc == k for ql, accs in seen for q, acc in zip(ql, accs))
            rej = any(acc < q - 1 for ql, accs in seen for q, acc in zip(ql, accs))
            if corrupt:
                assert rej, "no verify step rejected a draft"
            else:
                assert full, "no verify step accepted all k drafts"
            assert max(q for ql, _ in seen for q in ql) == k + 1
    finally:
        del r.verify
