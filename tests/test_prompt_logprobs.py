"""Prompt logprobs on the CPU backend: SamplingParams validation, the reference op, the engine
against a dense all-rows forward (chunked prefill, mixed batches, prefix cache, preemption),
the block manager's ``use_prefix=False``, the TP refusal, the /chat and OpenAI-proxy shapes and
the perplexity instrument.

The engines run in float32 on the same weights as the dense forward here; the two differ only
in operation order (paged against dense attention, fp32 sums of a few hundred terms: ~1e-5 on
a logit), so 1e-3 absolute leaves two orders of margin (tests/test_logprobs.py's argument)."""
import asyncio
import math

import httpx
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from agentic_traffic_testing_amd.config import EngineConfig
from agentic_traffic_testing_amd.engine.llm_engine import LLMEngine
from agentic_traffic_testing_amd.engine.sequence import SamplingParams
from agentic_traffic_testing_amd.ops import reference as ref
from agentic_traffic_testing_amd.runtime import BlockManager

ATOL = 1e-3


def engine(**kw):
    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def prompts(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(10, 3000, size=n).tolist() for n in sizes]


def dense_all_logits(model, ids):
    """``helpers.dense_logits`` for every row: a full-sequence causal forward without paging or
    kernels; returns the fp32 logits [T, vocab], row t predicting token t + 1."""
    c = model.cfg
    dev = model.embed.device
    x = F.embedding(torch.tensor(ids, device=dev), model.embed)
    T = len(ids)
    D = model.head_dim
    nq, nkv = model.n_heads, model.n_kv_heads
    pos = torch.arange(T, device=dev)
    mask = torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), 1)[None]
    for L in model.layers:
        h = ref.rms_norm(x, L.input_norm, c.rms_norm_eps)
        qkv = F.linear(h, L.qkv)
        q = qkv[:, :nq * D].view(T, nq, D)
        k = qkv[:, nq * D:(nq + nkv) * D].view(T, nkv, D)
        v = qkv[:, (nq + nkv) * D:(nq + 2 * nkv) * D].view(T, nkv, D)
        q = ref.rope_rotate(q, pos, model.cos_sin)
        k = ref.rope_rotate(k, pos, model.cos_sin)
        kk = k.float().repeat_interleave(model.g, 1)
        vv = v.float().repeat_interleave(model.g, 1)
        s = torch.einsum("qhd,khd->hqk", q.float(), kk) * model.scale
        s = s.masked_fill(mask, float("-inf"))
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vv).to(x.dtype)
        x = (x.float() + F.linear(a.reshape(T, -1), L.o).float()).to(x.dtype)
        h = ref.rms_norm(x, L.post_norm, c.rms_norm_eps)
        x = (x.float() + F.linear(ref.silu_and_mul(F.linear(h, L.gate_up)), L.down).float()).to(x.dtype)
    x = ref.rms_norm(x, model.norm, c.rms_norm_eps)
    return F.linear(x, model.lm_head).float()


def check_against_dense(eng, prompt, out, n_top):
    """Every prompt position of one request against the dense all-rows forward."""
    assert out.prompt_tokens == len(prompt)
    assert len(out.prompt_logprobs) == len(out.prompt_top_logprobs) == len(prompt)
    assert out.prompt_logprobs[0] is None and out.prompt_top_logprobs[0] is None
    ls = torch.log_softmax(dense_all_logits(eng.runner.model, list(prompt)), -1)
    for i in range(1, len(prompt)):
        row = ls[i - 1]
        assert abs(float(row[prompt[i]]) - out.prompt_logprobs[i]) <= ATOL, i
        alts = out.prompt_top_logprobs[i]
        assert len(alts) == n_top
        vals, order = torch.sort(row, descending=True, stable=True)
        for (t, v), wi, wv in zip(alts, order[:n_top].tolist(), vals[:n_top].tolist()):
            assert abs(v - wv) <= ATOL
            assert t == wi or abs(float(row[t]) - wv) <= 1e-5  # a near tie may swap neighbours


@pytest.mark.parametrize("bad", [-1, 21, 1.5, "3", True])
def test_sampling_params_validation(bad):
    eng = engine()
    with pytest.raises(ValueError):
        eng.add_request("r", [1, 2, 3], SamplingParams(prompt_logprobs=bad))
    assert not eng.has_unfinished()
    for ok in (None, 0, 1, 20):
        SamplingParams(prompt_logprobs=ok).check()


def test_reference_lm_head_score():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 64, generator=g)
    w = torch.randn(96, 64, generator=g) * 0.3
    tgt = torch.tensor([0, 15, 16, 95, 3, 3, 50], dtype=torch.int32)
    for eps in (0.0, 1e-5):
        xn = x.double()
        if eps > 0:
            xn = xn * torch.rsqrt(xn.pow(2).mean(-1, keepdim=True) + eps)
        want = torch.log_softmax(xn @ w.double().t(), -1).gather(1, tgt.long().view(-1, 1))
        got = ref.lm_head_score(x, w, eps, tgt)
        assert got.dtype == torch.float32 and got.shape == (7,)
        assert float((got.double() - want.view(-1)).abs().max()) <= 1e-4


def test_engine_chunked_prefill_and_mixed_batch():
    eng = engine(max_num_batched_tokens=16)
    ps = prompts((40, 23, 7))            # 40 tokens: three chunks, targets across both boundaries
    sps = [SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True, prompt_logprobs=3),
           SamplingParams(temperature=0.8, max_tokens=5, ignore_eos=True, seed=9,
                          prompt_logprobs=0),
           SamplingParams(temperature=0.8, max_tokens=3, ignore_eos=True, seed=4)]
    outs = eng.generate(ps, sps)
    check_against_dense(eng, ps[0], outs[0], 3)
    check_against_dense(eng, ps[1], outs[1], 0)
    assert outs[2].prompt_logprobs is None and outs[2].prompt_top_logprobs is None
    assert outs[0].logprobs is None   # the generated tokens' logprobs stay their own request
    # tokens do not depend on the field
    plain = eng.generate(ps, [SamplingParams(temperature=s.temperature, max_tokens=s.max_tokens,
                                             ignore_eos=True, seed=s.seed) for s in sps])
    assert [o.token_ids for o in plain] == [o.token_ids for o in outs]


def test_streamed_outputs_carry_the_whole_prompt():
    eng = engine(max_num_batched_tokens=16)
    p = prompts((40,), seed=6)[0]
    eng.add_request("r", p, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True,
                                           prompt_logprobs=0))
    seen = []
    while eng.has_unfinished():
        for o in eng.step():
            seen.append((len(o.token_ids), len(o.prompt_logprobs)))
    assert seen == [(1, 40), (2, 40), (3, 40)]


def test_prefix_cache_is_skipped_until_scored():
    eng = engine(enable_prefix_caching=True)
    p = prompts((50,), seed=3)[0]
    plain = SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True)
    first = eng.generate([p], plain)[0]
    assert first.cached_prompt_tokens == 0
    scored = eng.generate([p], SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                              prompt_logprobs=1))[0]
    assert scored.cached_prompt_tokens == 0
    check_against_dense(eng, p, scored, 1)
    assert scored.token_ids == first.token_ids
    again = eng.generate([p], plain)[0]
    assert again.cached_prompt_tokens > 0 and again.token_ids == first.token_ids


def test_engine_preemption_keeps_one_entry_per_prompt_token():
    eng = engine(max_model_len=128, num_kv_blocks=16, enable_prefix_caching=False)
    ps = prompts((30, 28, 33, 25), seed=1)
    sp = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True, prompt_logprobs=1)
    outs = eng.generate(ps, sp)
    assert eng.scheduler.num_preemptions > 0
    for p, o in zip(ps, outs):
        assert len(o.token_ids) == 40
        check_against_dense(eng, p, o, 1)


def test_preempted_mid_prompt_continues_at_the_first_missing_position():
    """A sequence that loses its blocks between two prefill chunks restarts its prefill and
    records each entry once."""
    eng = engine(max_num_batched_tokens=16)
    p = prompts((40,), seed=8)[0]
    eng.add_request("r", p, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                           prompt_logprobs=2))
    eng.step()                                   # the first chunk: entries 1 .. 16
    seq = eng.scheduler.running[0]
    assert len(seq.prompt_logprobs) == 17 and seq.scoring
    eng.scheduler.running.remove(seq)
    eng.scheduler._preempt(seq)
    outs = []
    while eng.has_unfinished():
        outs += eng.step()
    check_against_dense(eng, p, outs[-1], 2)


def test_block_manager_allocate_without_prefix():
    bm = BlockManager(32, 16, True)
    toks = np.arange(100, 170, dtype=np.int64)
    assert bm.allocate(1, toks, 71) == 0
    bm.commit(1, toks, 70)
    bm.free(1)
    q, h = bm.prefix_queries(), bm.prefix_hits()
    assert bm.peek_cached(toks) == 64
    assert bm.allocate(2, toks, 71, use_prefix=False) == 0
    assert (bm.prefix_queries(), bm.prefix_hits()) == (q, h)
    bm.commit(2, toks, 70)                       # hashes already mapped: nothing registered twice
    bm.free(2)
    assert bm.allocate(3, toks, 71) == 64        # the default still hits
    assert bm.prefix_queries() > q and bm.prefix_hits() > h


def test_tp_engine_refuses():
    from agentic_traffic_testing_amd.parallel.tp_engine import TPEngine

    eng = TPEngine(EngineConfig(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4,
                                use_graphs=False, tensor_parallel_size=2))
    try:
        with pytest.raises(ValueError, match="tensor-parallel"):
            eng.add_request("r", [1, 2, 3], SamplingParams(prompt_logprobs=0))
        assert not eng.has_unfinished()
    finally:
        eng.shutdown()


# ---- /chat and the OpenAI proxy over the real aiohttp stack -----------------------------------
def test_chat_and_proxy_shapes():
    from aiohttp import web

    from agentic_traffic_testing_amd.testing.stack import LLMBackendThread, cpu_engine
    from agentic_traffic_testing_amd.tools.mcp_universe import openai_proxy

    be = LLMBackendThread(cpu_engine())
    seen = []

    async def main():
        px = web.AppRunner(openai_proxy.create_app(f"{be.url}/chat"))
        await px.setup()
        site = web.TCPSite(px, "127.0.0.1", 0)
        await site.start()
        pport = site._server.sockets[0].getsockname()[1]

        async def spy(request):                 # what the proxy sends a backend
            seen.append(await request.json())
            return web.json_response({"output": "hi", "meta": {},
                                      "prompt_logprobs": {"tokens": ["x"]}})

        app = web.Application()
        app.router.add_post("/chat", spy)
        sr = web.AppRunner(app)
        await sr.setup()
        ss = web.TCPSite(sr, "127.0.0.1", 0)
        await ss.start()
        sp = web.AppRunner(openai_proxy.create_app(
            f"http://127.0.0.1:{ss._server.sockets[0].getsockname()[1]}/chat"))
        await sp.setup()
        sps = web.TCPSite(sp, "127.0.0.1", 0)
        await sps.start()
        spy_url = f"http://127.0.0.1:{sps._server.sockets[0].getsockname()[1]}/v1/chat/completions"

        req = {"prompt": "hello there", "max_tokens": 3, "temperature": 0.0, "ignore_eos": True}
        msgs = {"messages": [{"role": "user", "content": "hello"}], "max_tokens": 3}
        async with httpx.AsyncClient(timeout=60) as c:
            plain = await c.post(f"{be.url}/chat", json=req)
            top2 = await c.post(f"{be.url}/chat", json=dict(req, prompt_logprobs=2))
            zero = await c.post(f"{be.url}/chat", json=dict(req, prompt_logprobs=0))
            bad = await c.post(f"{be.url}/chat", json=dict(req, prompt_logprobs=99))
            url = f"http://127.0.0.1:{pport}/v1/chat/completions"
            p_plain = await c.post(url, json=msgs)
            p_plp = await c.post(url, json=dict(msgs, prompt_logprobs=1))
            await c.post(spy_url, json=msgs)
            spied = await c.post(spy_url, json=dict(msgs, prompt_logprobs=0))
        for r in (px, sp, sr):
            await r.cleanup()
        return plain, top2, zero, bad, p_plain, p_plp, spied

    try:
        plain, top2, zero, bad, p_plain, p_plp, spied = asyncio.run(main())
    finally:
        be.stop()
    assert bad.status_code == 400
    j0, j = plain.json(), top2.json()
    # without the key: exactly the former keys; with it: one more top-level object
    assert set(j0) == {"output", "meta"}
    assert set(j) == {"output", "meta", "prompt_logprobs"} and set(j["meta"]) == set(j0["meta"])
    assert j["output"] == j0["output"]
    lp = j["prompt_logprobs"]
    assert set(lp) == {"tokens", "token_ids", "token_logprobs", "top_logprobs"}
    n = j["meta"]["prompt_tokens"]              # after chat template (and truncation)
    assert n > 2 and all(len(lp[k]) == n for k in lp)
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert all(v <= 0.0 for v in lp["token_logprobs"][1:])
    assert all(len(a) == 2 and set(a[0]) == {"token", "token_id", "logprob"}
               and a[0]["logprob"] >= a[1]["logprob"] for a in lp["top_logprobs"][1:])
    assert all(a[0]["logprob"] >= v - 1e-6
               for a, v in zip(lp["top_logprobs"][1:], lp["token_logprobs"][1:]))
    z = zero.json()["prompt_logprobs"]
    assert z["token_ids"] == lp["token_ids"] and z["top_logprobs"] == [None] + [[]] * (n - 1)
    assert np.allclose(z["token_logprobs"][1:], lp["token_logprobs"][1:], atol=1e-5)
    # proxy: untouched without the key; with it the backend's block under the same key
    q0, q = p_plain.json(), p_plp.json()
    assert set(q0) == {"id", "object", "created", "model", "choices", "usage"}
    assert set(q) == set(q0) | {"prompt_logprobs"}
    assert set(q["prompt_logprobs"]) == set(lp)
    assert len(q["prompt_logprobs"]["token_ids"]) == q["usage"]["prompt_tokens"]
    assert q["prompt_logprobs"]["token_logprobs"][0] is None
    assert seen[0] == {"prompt": "[USER]\nhello", "max_tokens": 3}
    assert seen[1] == {"prompt": "[USER]\nhello", "max_tokens": 3, "prompt_logprobs": 0}
    assert spied.json()["prompt_logprobs"] == {"tokens": ["x"]}


# ---- the instrument ---------------------------------------------------------------------------
def test_perplexity_instrument_against_dense():
    from agentic_traffic_testing_amd.bench import perplexity

    eng = engine(max_num_batched_tokens=32)
    ids = np.random.default_rng(11).integers(10, 3000, size=100)
    lp = perplexity.score_ids(eng, ids, 40)     # windows of 40, 40 and 20 tokens
    assert lp.shape == (97,)
    want = []
    for w in perplexity.windows(ids, 40):
        ls = torch.log_softmax(dense_all_logits(eng.runner.model, w), -1)
        want += [float(ls[i - 1, w[i]]) for i in range(1, len(w))]
    s = perplexity.summarise(lp)
    ppl = math.exp(-float(np.mean(want)))
    assert s["tokens"] == 97
    assert abs(s["perplexity"] - ppl) <= 1e-3 * ppl
    assert abs(s["perplexity"] - math.exp(s["mean_nll"])) <= 1e-9 * ppl
    d = perplexity.summarise(lp, np.asarray(want))
    assert d["max_abs_dlogprob"] <= ATOL and d["mean_abs_dlogprob"] <= d["max_abs_dlogprob"]
    assert np.array_equal(perplexity.load_ids("synthetic:64:3", vocab=4096),
                          perplexity.load_ids("synthetic:64:3", vocab=4096))
