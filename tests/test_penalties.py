"""Sampling penalties and logit bias on the CPU backend: SamplingParams validation, the
reference formula against hand-worked values, the engine against a host oracle at every position
(plain, chunked prefill, prefix cache, preemption, mixed batch, speculation on, TP refusal) and
the /chat and OpenAI-proxy plumbing.

The oracle applies the documented formula in fp64 to ``helpers.dense_logits`` on the engine's
own prefix, from the prompt and the outputs so far:  a token seen in prompt or outputs has its
logit divided (l > 0) or multiplied by rep;  l -= freq * count + pres * (count > 0) with the
count over the outputs only;  l += bias.  The engine's token must be within 0.05 of the
penalised maximum (test_engine.py's CPU near-tie tolerance; the engine and the dense forward
differ by ~1e-5 on a logit)."""
import asyncio

import httpx
import numpy as np
import pytest
import torch

from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref
from helpers import dense_logits

REP, FREQ, PRES = 1.25, 1.0, 0.5
SHAPES = ((0, 12), (1, 40), (2, 23))   # (seed, prompt length)
N_TOKENS = 24


def engine(**kw):
    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def prompts(hi=3000):
    return [np.random.default_rng(seed).integers(10, hi, n).tolist() for seed, n in SHAPES]


def params(prompt, bias=8.0, **kw):
    return SamplingParams(temperature=0.0, max_tokens=N_TOKENS, ignore_eos=True,
                          repetition_penalty=REP, frequency_penalty=FREQ, presence_penalty=PRES,
                          logit_bias={prompt[0]: bias, 3500: bias, 7: -100.0}, **kw)


def penalised_logits(raw, prompt, outs, sp):
    """The documented formula in fp64 on one row of raw logits."""
    l = raw.double().clone()
    V = l.shape[0]
    cnt = torch.bincount(torch.tensor(outs, dtype=torch.long), minlength=V).double()
    seen = cnt > 0
    seen[torch.tensor(prompt, dtype=torch.long)] = True
    rep = sp.repetition_penalty
    l = torch.where(seen, torch.where(l > 0, l / rep, l * rep), l)
    l = l - sp.frequency_penalty * cnt - sp.presence_penalty * (cnt > 0).double()
    for k, b in (sp.logit_bias or {}).items():
        l[k] += b
    return l


def check_against_oracle(model, prompt, token_ids, sp, tol=0.05, max_bad=0):
    """Every position teacher-forced; returns (positions whose penalised argmax differs from
    the raw argmax, the highest count of one token, the smallest penalised top-2 gap)."""
    changed = bad = 0
    min_gap = float("inf")
    outs = []
    for t in token_ids:
        raw = dense_logits(model, list(prompt) + outs).float().cpu()
        pl = penalised_logits(raw, prompt, outs, sp)
        top2 = torch.topk(pl, 2).values
        min_gap = min(min_gap, float(top2[0] - top2[1]))
        changed += int(torch.argmax(pl)) != int(torch.argmax(raw))
        if int(torch.argmax(pl)) != t:
            gap = float(pl.max() - pl[t])
            assert gap < tol, (len(outs), t, int(torch.argmax(pl)), gap)
            bad += 1
        outs.append(t)
    assert bad <= max_bad, (bad, len(token_ids))
    most = max(np.bincount(np.asarray(token_ids)))
    return changed, int(most), min_gap


# ---- validation -----------------------------------------------------------------------------
VOCAB = 4096  # the tiny model's


@pytest.mark.parametrize("bad", [
    dict(presence_penalty=2.5), dict(frequency_penalty=2.5), dict(presence_penalty=-2.5),
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
    dict(presence_penalty=float("nan")), dict(frequency_penalty=float("nan")),
    dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
    dict(logit_bias={i: 1.0 for i in range(301)}), dict(logit_bias={VOCAB: 1.0}),
    dict(logit_bias={-1: 1.0}), dict(logit_bias={5: 101.0}), dict(logit_bias={5: float("nan")}),
    dict(logit_bias={5: True}), dict(logit_bias={True: 1.0}), dict(presence_penalty=True),
    dict(repetition_penalty=True), dict(logit_bias={"5": 1.0}), dict(logit_bias=[5, 1.0]),
    dict(frequency_penalty="1"),
])
def test_bad_values_raise_and_leave_the_engine_idle(bad):
    eng = engine()
    assert eng.model_cfg.vocab_size == VOCAB
    with pytest.raises(ValueError):
        eng.add_request("r", [1, 2, 3], SamplingParams(**bad))
    assert not eng.has_unfinished()
    assert eng.runner.pen is None  # nothing allocated for a refused request


def test_boundary_values_pass_and_defaults_are_not_penalised():
    eng = engine()
    for ok in (dict(presence_penalty=2.0, frequency_penalty=-2.0),
               dict(presence_penalty=-2, frequency_penalty=2),
               dict(repetition_penalty=1e-3), dict(repetition_penalty=50),
               dict(logit_bias={i: 100.0 for i in range(300)}),
               dict(logit_bias={0: -100, VOCAB - 1: 100}), dict(logit_bias={})):
        sp = SamplingParams(**ok)
        sp.check(VOCAB)
        eng.check_sampling(sp)
    assert not SamplingParams().penalised and not SamplingParams(logit_bias={}).penalised
    assert SamplingParams(repetition_penalty=1.1).penalised
    assert SamplingParams(logit_bias={1: 0.0}).penalised
    # an engine that never saw a penalised request allocates nothing and runs variant 0
    eng.generate([[5, 6, 7]], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    assert eng.runner.pen is None


def test_variant_code_and_layout_keep_their_old_values():
    from agentic_traffic_testing_amd.engine import model_runner as mr

    assert mr.V_PENALTY == 8
    for topkp in (False, True):
        for lp in (mr.LP_NONE, mr.LP_SAMPLED, mr.LP_TOPN):
            old = mr.variant_code(topkp, lp)
            assert old == int(topkp) | lp << 1 and mr.variant_lp(old) == lp
            new = mr.variant_code(topkp, lp, True)
            assert new == old | 8 and mr.variant_lp(new) == lp
    plain, pen = mr.MetaLayout(7, 3, 4, 2), mr.MetaLayout(7, 3, 4, 2, penalty=True)
    for name, field in plain.fields.items():     # existing offsets do not move
        assert pen.fields[name] == field
    assert list(pen.fields)[len(plain.fields):] == ["pen_slot", "pen_rep", "pen_freq",
                                                     "pen_pres"]
    assert pen.size > plain.size and "pen_slot" not in plain.fields


# ---- reference semantics --------------------------------------------------------------------
def test_reference_apply_hand_worked_table():
    V = 8
    state = torch.zeros(3, V, dtype=torch.int32)
    bias_ids = torch.full((3, 300), -1, dtype=torch.int32)
    bias_vals = torch.zeros(3, 300)
    # slot 2: token 1 prompt-only; token 2 generated twice (duplicates); token 3 in the prompt
    # (twice) and generated once; tokens 4 and 5 generated once; a bias on token 3 (seen),
    # token 6 (unseen) and token 7 (unseen, id V - 1); id 99 is outside the vocabulary
    ref.penalty_seed(state[2], [1, 3, 3, 99], [2, 4, 2, 3, 5], bias_ids[2], bias_vals[2],
                     [3, 6, 7], [0.75, -1.5, 2.0])
    P = ref.PENALTY_PROMPT_BIT
    assert state[2].tolist() == [0, P, 2, P + 1, 1, 1, 0, 0]
    assert state[:2].abs().sum() == 0
    assert bias_ids[2, :4].tolist() == [3, 6, 7, -1] and bias_vals[2, :3].tolist() == [0.75, -1.5, 2]
    logits = torch.tensor([[1.0, 2.0, 3.0, -4.0, 5.0, -1.0, 0.5, -0.25],
                           [1.0, 2.0, 3.0, -4.0, 5.0, -1.0, 0.5, -0.25]])
    out = torch.full((2, V), 77.0)
    slot = torch.tensor([2, -1], dtype=torch.int32)
    rep, freq, pres = torch.tensor([2.0, 2.0]), torch.tensor([0.5, 0.5]), torch.tensor([0.25, 0.25])
    ref.penalty_apply(out, logits, state, slot, rep, freq, pres, bias_ids, bias_vals)
    want0 = [1.0,                           # unseen
             2.0 / 2,                       # prompt only: rep, no count
             3.0 / 2 - 0.5 * 2 - 0.25,      # generated twice, positive
             -4.0 * 2 - 0.5 * 1 - 0.25 + 0.75,   # prompt + generated, negative, biased
             5.0 / 2 - 0.5 - 0.25,          # generated once, positive
             -1.0 * 2 - 0.5 - 0.25,         # generated once, negative
             0.5 - 1.5,                     # unseen, biased
             -0.25 + 2.0]                   # unseen, biased, last id
    assert out[0].tolist() == want0 == [1.0, 1.0, 0.25, -8.0, 1.75, -2.75, -1.0, 1.75]
    assert out[1].tolist() == logits[1].tolist()   # slot -1: unchanged
    # update: counts rise, the prompt flag stays, slot -1 rows touch nothing
    before = state.clone()
    ref.penalty_update(state, slot, torch.tensor([3, 3]))
    ref.penalty_update(state, slot, torch.tensor([0, 1]))
    before[2, 3] += 1
    before[2, 0] += 1
    assert torch.equal(state, before) and int(state[2, 3]) == P + 2


# ---- engine against the oracle --------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_run():
    """The three penalised requests through the default engine, checked against the oracle."""
    eng = engine()
    ps = prompts()
    sps = [params(p) for p in ps]
    outs = eng.generate(ps, sps)
    return eng, ps, sps, [o.token_ids for o in outs]


def test_engine_matches_oracle_at_every_position(plain_run):
    eng, ps, sps, toks = plain_run
    for p, sp, ids in zip(ps, sps, toks):
        assert len(ids) == N_TOKENS
        changed, most, gap = check_against_oracle(eng.runner.model, p, ids, sp)
        print(f"prompt {len(p)}: changed {changed}/{N_TOKENS}, most-generated count {most}, "
              f"smallest top-2 gap {gap:.4f}")
        assert changed >= 12     # the penalties decide most positions ...
        assert most >= 4         # ... the counts matter (a token comes back four times) ...
        assert 7 not in ids      # ... and the -100 bias bans its token
    # every slot went back, the counts of a finished request are nobody's
    r = eng.runner
    assert not r._pen_slot and sorted(r._pen_free) == list(range(eng.cfg.max_num_seqs))
    assert r.pen["state"].shape == (eng.cfg.max_num_seqs, VOCAB)


def test_chunked_prefill_equals_plain(plain_run):
    _, ps, sps, toks = plain_run
    eng = engine(max_num_batched_tokens=16)   # the 40- and 23-token prompts prefill in chunks
    assert [o.token_ids for o in eng.generate(ps, sps)] == toks


def test_prefix_cache_repeat_equals_plain(plain_run):
    _, ps, sps, toks = plain_run
    eng = engine(enable_prefix_caching=True)
    assert [o.token_ids for o in eng.generate(ps, sps)] == toks
    again = eng.generate(ps, sps)
    assert any(o.cached_prompt_tokens > 0 for o in again)
    assert [o.token_ids for o in again] == toks


def test_preemption_continues_the_counts(plain_run):
    _, ps, sps, toks = plain_run
    # 8 blocks of 16 tokens hold 128 of the 147 tokens the three requests end with
    eng = engine(max_model_len=64, num_kv_blocks=8, enable_prefix_caching=False)
    outs = eng.generate(ps, sps)
    assert eng.scheduler.num_preemptions > 0
    assert [o.token_ids for o in outs] == toks
    assert not eng.runner._pen_slot


def test_mixed_batch_equals_alone(plain_run):
    _, ps, sps, toks = plain_run
    other = prompts()[1][:17]
    sp_other = SamplingParams(temperature=0.8, max_tokens=15, ignore_eos=True, seed=11)
    alone = engine().generate([other], sp_other)[0].token_ids
    eng = engine()
    outs = eng.generate([other, ps[0]], [sp_other, sps[0]])
    assert outs[0].token_ids == alone and outs[1].token_ids == toks[0]


def test_speculation_steps_aside_for_penalties():
    rng = np.random.default_rng(0)
    loop = rng.integers(300, 3000, size=12).tolist() * 4   # the n-gram proposer drafts on this
    plain, spec = engine(), engine(speculative="ngram")
    sp = SamplingParams(temperature=0.0, max_tokens=48, ignore_eos=True)
    assert spec.generate([loop], sp)[0].token_ids == plain.generate([loop], sp)[0].token_ids
    assert spec.spec_stats["verify_steps"] > 0              # speculation is live here ...
    before = dict(spec.spec_stats)
    sp_pen = SamplingParams(temperature=0.0, max_tokens=48, ignore_eos=True,
                            repetition_penalty=REP, frequency_penalty=FREQ, presence_penalty=PRES)
    want = plain.generate([loop], sp_pen)[0].token_ids
    assert spec.generate([loop], sp_pen)[0].token_ids == want
    assert spec.spec_stats == before                        # ... and no verify step ran now
    check_against_oracle(plain.runner.model, loop, want, sp_pen)


def test_tp2_gloo_refuses_penalised_requests():
    from agentic_traffic_testing_amd.parallel.tp_engine import TPEngine

    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    p = prompts()[0]
    sp = SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True)
    want = LLMEngine(EngineConfig(**base)).generate([p], sp)[0].token_ids
    eng = TPEngine(EngineConfig(tensor_parallel_size=2, **base))
    try:
        for kw in (dict(presence_penalty=0.5), dict(frequency_penalty=0.5),
                   dict(repetition_penalty=1.1), dict(logit_bias={5: 1.0})):
            with pytest.raises(ValueError, match="tensor-parallel"):
                eng.add_request("r", p, SamplingParams(**kw))
        assert not eng.has_unfinished()
        assert eng.generate([p], sp)[0].token_ids == want
    finally:
        eng.shutdown()


# ---- /chat and the OpenAI proxy --------------------------------------------------------------
def test_chat_takes_the_four_keys():
    from agentic_traffic_testing_amd.testing.stack import LLMBackendThread, cpu_engine

    eng = cpu_engine()
    be = LLMBackendThread(eng)
    k = 1234
    req = {"prompt": "hello there", "max_tokens": 6, "temperature": 0.0, "ignore_eos": True}
    seen = []
    add = eng.add_request

    def spy(rid, ids, sampling, *a, **kw):
        seen.append(sampling)
        return add(rid, ids, sampling, *a, **kw)

    eng.add_request = spy

    async def main():
        async with httpx.AsyncClient(timeout=60) as c:
            url = f"{be.url}/chat"
            plain = await c.post(url, json=req)
            forced = await c.post(url, json=dict(req, logit_bias={str(k): 100}, logprobs=0))
            allk = await c.post(url, json=dict(req, presence_penalty=0.5, frequency_penalty=-0.25,
                                               repetition_penalty=1.5, logit_bias={"7": -100}))
            bad = [await c.post(url, json=dict(req, **kw)) for kw in (
                dict(presence_penalty=2.5), dict(frequency_penalty="x"),
                dict(repetition_penalty=0), dict(logit_bias={"abc": 1}),
                dict(logit_bias={str(k): 101}), dict(logit_bias={"4096": 1}),
                dict(logit_bias=[1, 2]), dict(presence_penalty=True))]
        return plain, forced, allk, bad

    try:
        plain, forced, allk, bad = asyncio.run(main())
    finally:
        be.stop()
    assert plain.status_code == forced.status_code == allk.status_code == 200
    assert set(plain.json()) == {"output", "meta"} == set(allk.json())
    assert set(allk.json()["meta"]) == set(plain.json()["meta"])
    assert forced.json()["logprobs"]["token_ids"] == [k] * 6      # the bias forces token k
    assert [r.status_code for r in bad] == [400] * len(bad)
    assert all("error" in r.json() for r in bad)
    assert len(seen) == 3 and not seen[0].penalised
    assert seen[1].logit_bias == {k: 100}
    s = seen[2]
    assert (s.presence_penalty, s.frequency_penalty, s.repetition_penalty, s.logit_bias) == \
           (0.5, -0.25, 1.5, {7: -100})


def test_proxy_forwards_the_keys_and_nothing_else():
    from aiohttp import web

    from agentic_traffic_testing_amd.tools.mcp_universe import openai_proxy

    seen = []

    async def fake_chat(request):
        seen.append(await request.json())
        return web.json_response({"output": "hi", "meta": {}})

    async def main():
        app = web.Application()
        app.router.add_post("/chat", fake_chat)
        r = web.AppRunner(app)
        await r.setup()
        s = web.TCPSite(r, "127.0.0.1", 0)
        await s.start()
        port = s._server.sockets[0].getsockname()[1]
        px = web.AppRunner(openai_proxy.create_app(f"http://127.0.0.1:{port}/chat"))
        await px.setup()
        ps = web.TCPSite(px, "127.0.0.1", 0)
        await ps.start()
        pport = ps._server.sockets[0].getsockname()[1]
        msgs = [{"role": "user", "content": "x"}]
        async with httpx.AsyncClient() as c:
            url = f"http://127.0.0.1:{pport}/v1/chat/completions"
            await c.post(url, json={"messages": msgs, "max_tokens": 3})
            await c.post(url, json={"messages": msgs, "presence_penalty": 0.5,
                                    "frequency_penalty": 1, "logit_bias": {"50": -100}})
            await c.post(url, json={"messages": msgs, "repetition_penalty": 1.2,
                                    "presence_penalty": None, "temperature": 0.3})
        await px.cleanup()
        await r.cleanup()

    asyncio.run(main())
    assert seen[0] == {"prompt": "[USER]\nx", "max_tokens": 3}
    assert seen[1] == {"prompt": "[USER]\nx", "presence_penalty": 0.5, "frequency_penalty": 1,
                       "logit_bias": {"50": -100}}
    assert seen[2] == {"prompt": "[USER]\nx", "repetition_penalty": 1.2}
