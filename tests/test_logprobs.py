"""Per-token logprobs on the CPU backend: SamplingParams validation, the engine against the
dense forward's ``log_softmax`` at every position (chunked prefill, prefix cache, preemption,
EOS, mixed batches, speculation on, TP = 2 over gloo) and the /chat and OpenAI-proxy shapes.

The engines here run in float32 on the same weights as ``helpers.dense_logits``; the two
differ only in operation order (paged against dense attention, fp32 sums of a few hundred
terms: ~1e-5 on a logit), so 1e-3 absolute leaves two orders of margin."""
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

ATOL = 1e-3


def engine(**kw):
    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    base.update(kw)
    return LLMEngine(EngineConfig(**base))


def prompts(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(10, 3000, size=n).tolist() for n in sizes]


def check_against_dense(eng, prompt, out, n_top):
    """Every position of one request teacher-forced through the dense forward."""
    assert len(out.logprobs) == len(out.top_logprobs) == len(out.token_ids)
    ids = list(prompt)
    for t, lp, alts in zip(out.token_ids, out.logprobs, out.top_logprobs):
        ls = torch.log_softmax(dense_logits(eng.runner.model, ids), -1)
        assert abs(float(ls[t]) - lp) <= ATOL
        assert len(alts) == n_top
        vals, order = torch.sort(ls, descending=True, stable=True)
        for (i, v), wi, wv in zip(alts, order[:n_top].tolist(), vals[:n_top].tolist()):
            assert abs(v - wv) <= ATOL
            assert i == wi or abs(float(ls[i]) - wv) <= 1e-5  # a near tie may swap neighbours
        ids.append(t)


@pytest.mark.parametrize("bad", [-1, 21, 1.5, "3", True])
def test_sampling_params_validation(bad):
    eng = engine()
    with pytest.raises(ValueError):
        eng.add_request("r", [1, 2, 3], SamplingParams(logprobs=bad))
    assert not eng.has_unfinished()
    for ok in (None, 0, 1, 20):
        SamplingParams(logprobs=ok).check()


def test_reference_token_logprobs_tie_order():
    l = torch.tensor([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    lp, ids, top = ref.token_logprobs(l, torch.tensor([4, 0]), 4)
    assert ids.tolist() == [[1, 2, 5, 0], [0, 1, 2, 3]] and ids.dtype == torch.int32
    want = torch.log_softmax(l.double(), -1)
    assert abs(float(lp[0]) - float(want[0, 4])) < 1e-6
    assert torch.allclose(top[1].double(), want[1, :4], atol=1e-6)


def test_engine_chunked_prefill_prefix_cache_mixed_batch():
    eng = engine(max_num_batched_tokens=16, enable_prefix_caching=True)
    ps = prompts((40, 7, 23))           # 40 tokens: three prefill chunks of <= 16
    sps = [SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=3),
           SamplingParams(temperature=0.8, max_tokens=5, ignore_eos=True, seed=4),
           SamplingParams(temperature=0.8, max_tokens=7, ignore_eos=True, seed=9, logprobs=0)]
    outs = eng.generate(ps, sps)
    assert outs[1].logprobs is None and outs[1].top_logprobs is None
    check_against_dense(eng, ps[0], outs[0], 3)
    check_against_dense(eng, ps[2], outs[2], 0)
    # the same prompt again is served from the prefix cache: same tokens, same logprobs
    again = eng.generate([ps[0]], sps[0])[0]
    assert again.cached_prompt_tokens > 0
    assert again.token_ids == outs[0].token_ids
    assert np.allclose(again.logprobs, outs[0].logprobs, atol=1e-4)
    check_against_dense(eng, ps[0], again, 3)


def test_engine_preemption_keeps_one_entry_per_token():
    eng = engine(max_model_len=128, num_kv_blocks=16, enable_prefix_caching=False)
    ps = prompts((30, 28, 33, 25), seed=1)
    sp = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True, logprobs=1)
    outs = eng.generate(ps, sp)
    assert eng.scheduler.num_preemptions > 0
    for p, o in zip(ps, outs):
        assert len(o.token_ids) == 40
        check_against_dense(eng, p, o, 1)


def test_engine_stop_at_eos():
    eng = engine()
    p = prompts((12,), seed=2)[0]
    free = eng.generate([p], SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))[0]
    stop = free.token_ids[3]
    sp = SamplingParams(temperature=0.0, max_tokens=8, stop_token_ids=(stop,), logprobs=2)
    out = eng.generate([p], sp)[0]
    cut = free.token_ids.index(stop) + 1
    assert out.finish_reason == "stop" and out.token_ids == free.token_ids[:cut]
    check_against_dense(eng, p, out, 2)


@pytest.mark.parametrize("temp", [0.0, 0.8])
def test_tokens_do_not_depend_on_logprobs(temp):
    eng = engine()
    ps = prompts((9, 21, 5), seed=3)
    kw = dict(temperature=temp, max_tokens=10, ignore_eos=True, seed=17)
    off = [o.token_ids for o in eng.generate(ps, SamplingParams(**kw))]
    for n in (0, 5):
        on = eng.generate(ps, SamplingParams(logprobs=n, **kw))
        assert [o.token_ids for o in on] == off
        assert all(len(o.logprobs) == 10 for o in on)


def test_streamed_outputs_grow_with_their_tokens():
    eng = engine()
    eng.add_request("r", prompts((8,))[0], SamplingParams(temperature=0.0, max_tokens=5,
                                                          ignore_eos=True, logprobs=2))
    seen = []
    while eng.has_unfinished():
        for o in eng.step():
            assert len(o.logprobs) == len(o.top_logprobs) == len(o.token_ids)
            seen.append(len(o.token_ids))
    assert seen == [1, 2, 3, 4, 5]


def test_speculation_steps_aside_for_logprobs():
    rng = np.random.default_rng(0)
    loop = rng.integers(300, 3000, size=12).tolist() * 4   # a prompt the n-gram proposer drafts on
    plain = engine()
    spec = engine(speculative="ngram")
    sp = SamplingParams(temperature=0.0, max_tokens=96, ignore_eos=True)
    base = plain.generate([loop], sp)[0]
    assert spec.generate([loop], sp)[0].token_ids == base.token_ids
    assert spec.spec_stats["verify_steps"] > 0              # speculation is live here ...
    before = dict(spec.spec_stats)
    sp_lp = SamplingParams(temperature=0.0, max_tokens=96, ignore_eos=True, logprobs=2)
    want = plain.generate([loop], sp_lp)[0]
    got = spec.generate([loop], sp_lp)[0]
    assert spec.spec_stats == before                        # ... and no verify step ran now
    assert got.token_ids == want.token_ids == base.token_ids
    assert got.logprobs == want.logprobs and got.top_logprobs == want.top_logprobs


def test_tp2_gloo_equals_tp1():
    from agentic_traffic_testing_amd.parallel.tp_engine import TPEngine

    base = dict(model="tiny", device="cpu", dtype="float32", max_model_len=256,
                num_kv_blocks=64, max_num_batched_tokens=64, max_num_seqs=4, use_graphs=False)
    ps = prompts((9, 14), seed=5)
    sps = [SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True, logprobs=0),
           SamplingParams(temperature=0.8, max_tokens=6, ignore_eos=True, seed=2, logprobs=3)]
    want = LLMEngine(EngineConfig(**base)).generate(ps, sps)
    eng = TPEngine(EngineConfig(tensor_parallel_size=2, **base))
    try:
        got = eng.generate(ps, sps)
    finally:
        eng.shutdown()
    for a, b in zip(got, want):
        assert a.token_ids == b.token_ids
        assert np.allclose(a.logprobs, b.logprobs, atol=ATOL)
        assert [[i for i, _ in alts] for alts in a.top_logprobs] == \
               [[i for i, _ in alts] for alts in b.top_logprobs]


# ---- /chat and the OpenAI proxy over the real aiohttp stack -----------------------------------
def test_chat_and_proxy_shapes():
    from aiohttp import web

    from agentic_traffic_testing_amd.testing.stack import LLMBackendThread, cpu_engine
    from agentic_traffic_testing_amd.tools.mcp_universe import openai_proxy

    be = LLMBackendThread(cpu_engine())

    async def main():
        px = web.AppRunner(openai_proxy.create_app(f"{be.url}/chat"))
        await px.setup()
        site = web.TCPSite(px, "127.0.0.1", 0)
        await site.start()
        pport = site._server.sockets[0].getsockname()[1]
        req = {"prompt": "hello there", "max_tokens": 5, "temperature": 0.0, "ignore_eos": True}
        msgs = {"messages": [{"role": "user", "content": "hello"}], "max_tokens": 4}
        async with httpx.AsyncClient(timeout=60) as c:
            plain = await c.post(f"{be.url}/chat", json=req)
            with_lp = await c.post(f"{be.url}/chat", json=dict(req, logprobs=2))
            zero = await c.post(f"{be.url}/chat", json=dict(req, logprobs=0))
            bad = await c.post(f"{be.url}/chat", json=dict(req, logprobs=99))
            p_plain = await c.post(f"http://127.0.0.1:{pport}/v1/chat/completions", json=msgs)
            p_lp = await c.post(f"http://127.0.0.1:{pport}/v1/chat/completions",
                                json=dict(msgs, logprobs=True, top_logprobs=3))
            p_lp0 = await c.post(f"http://127.0.0.1:{pport}/v1/chat/completions",
                                 json=dict(msgs, logprobs=True))
        await px.cleanup()
        return plain, with_lp, zero, bad, p_plain, p_lp, p_lp0

    try:
        plain, with_lp, zero, bad, p_plain, p_lp, p_lp0 = asyncio.run(main())
    finally:
        be.stop()
    assert bad.status_code == 400
    j0, j = plain.json(), with_lp.json()
    # without the field: exactly today's keys; with it: one more top-level object
    assert set(j0) == {"output", "meta"}
    assert set(j) == {"output", "meta", "logprobs"} and set(j["meta"]) == set(j0["meta"])
    assert j["output"] == j0["output"]
    lp = j["logprobs"]
    assert set(lp) == {"tokens", "token_ids", "token_logprobs", "top_logprobs"}
    n = j["meta"]["completion_tokens"]
    assert n == 5 and all(len(lp[k]) == n for k in lp)
    assert all(v <= 0.0 for v in lp["token_logprobs"])
    assert all(len(a) == 2 and set(a[0]) == {"token", "token_id", "logprob"}
               for a in lp["top_logprobs"])
    # greedy: the sampled token is the most likely one
    assert [a[0]["token_id"] for a in lp["top_logprobs"]] == lp["token_ids"]
    z = zero.json()["logprobs"]
    assert z["token_ids"] == lp["token_ids"] and z["top_logprobs"] == [[]] * n
    # proxy: untouched without the fields, OpenAI's content list with them
    q0, q, qz = p_plain.json(), p_lp.json(), p_lp0.json()
    assert set(q0["choices"][0]) == {"index", "message", "finish_reason"}
    content = q["choices"][0]["logprobs"]["content"]
    assert len(content) == q["usage"]["completion_tokens"] > 0
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert e["bytes"] == list(e["token"].encode()) and len(e["top_logprobs"]) == 3
        assert set(e["top_logprobs"][0]) == {"token", "logprob", "bytes"}
    assert all(e["top_logprobs"] == [] for e in qz["choices"][0]["logprobs"]["content"])


def test_proxy_forwards_plain_requests_unchanged():
    """Requests without logprobs reach the backend byte for byte as before."""
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
            await c.post(url, json={"messages": msgs, "logprobs": False, "top_logprobs": 4})
            await c.post(url, json={"messages": msgs, "logprobs": True, "top_logprobs": 4})
            await c.post(url, json={"messages": msgs, "logprobs": True})
        await px.cleanup()
        await r.cleanup()

    asyncio.run(main())
    assert seen[0] == {"prompt": "[USER]\nx", "max_tokens": 3}
    assert seen[1] == {"prompt": "[USER]\nx"}
    assert seen[2] == {"prompt": "[USER]\nx", "logprobs": 4}
    assert seen[3] == {"prompt": "[USER]\nx", "logprobs": 0}
