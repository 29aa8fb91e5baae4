"""Guided decoding over HTTP (CPU backend): /chat with each of the three keys, 400 on bad
values, the OpenAI proxy's forwarding and its ``response_format`` mapping, end to end."""
import asyncio
import json
import re

import httpx
from aiohttp import web

from agentic_traffic_testing_amd.tools.mcp_universe import openai_proxy
from test_guided import BOUNDED, CHOICES, DIGITS, validate_bounded


async def serve(app):
    runner = web.AppRunner(app)
    await runner.setup()
    site = web.TCPSite(runner, "127.0.0.1", 0)
    await site.start()
    return runner, site._server.sockets[0].getsockname()[1]


def test_chat_takes_the_three_keys_and_refuses_bad_values():
    from agentic_traffic_testing_amd.testing.stack import LLMBackendThread, cpu_engine

    eng = cpu_engine()
    be = LLMBackendThread(eng)
    req = {"prompt": "is the build green?", "max_tokens": 120, "temperature": 0.7, "seed": 4}
    seen, compiled = [], []
    add, comp = eng.add_request, eng.compile_guide

    def spy_add(rid, ids, sampling, *a, **kw):
        seen.append((sampling, eng._guides.compiles if eng._guides else 0))
        return add(rid, ids, sampling, *a, **kw)

    def spy_compile(sampling):
        import threading

        n = eng._guides.compiles if eng._guides else 0
        try:
            return comp(sampling)
        finally:     # (thread, did this call compile - a cache miss?)
            compiled.append((threading.current_thread().name,
                             (eng._guides.compiles if eng._guides else 0) > n))

    eng.add_request, eng.compile_guide = spy_add, spy_compile

    async def main():
        async with httpx.AsyncClient(timeout=120) as c:
            url = f"{be.url}/chat"
            plain = await c.post(url, json=dict(req, max_tokens=5))
            good = [await c.post(url, json=dict(req, **kw)) for kw in (
                dict(guided_regex=DIGITS), dict(guided_choice=CHOICES),
                dict(guided_json=BOUNDED), dict(guided_json=json.dumps(BOUNDED)))]
            bad = [await c.post(url, json=dict(req, **kw)) for kw in (
                dict(guided_regex=7), dict(guided_regex="a(?=b)"), dict(guided_regex=""),
                dict(guided_choice="yes"), dict(guided_choice=[]), dict(guided_choice=[1]),
                dict(guided_json=[1]), dict(guided_json="{"),
                dict(guided_json={"type": "object", "additionalProperties": True}),
                dict(guided_regex=DIGITS, guided_choice=CHOICES),
                dict(guided_regex=DIGITS, guided_json=BOUNDED),
                dict(guided_regex=DIGITS, ignore_eos=True))]
        return plain, good, bad

    try:
        plain, good, bad = asyncio.run(main())
    finally:
        be.stop()
    assert plain.status_code == 200 and [r.status_code for r in good] == [200] * 4
    for r in good:       # responses keep today's keys
        assert set(r.json()) == {"output", "meta"} == set(plain.json())
        assert set(r.json()["meta"]) == set(plain.json()["meta"])
        assert r.json()["meta"]["finish_reason"] == "stop"
    assert re.fullmatch(DIGITS, good[0].json()["output"])
    assert good[1].json()["output"] in CHOICES
    validate_bounded(good[2].json()["output"])
    validate_bounded(good[3].json()["output"])
    assert [r.status_code for r in bad] == [400] * len(bad)
    assert all(r.json()["error"] for r in bad)
    assert "look-around" in bad[1].json()["error"] and "only one" in bad[9].json()["error"]
    # only the good requests reached the engine, each with its guide already compiled by the
    # handler, off the engine thread (schema object and schema text: one cache entry)
    assert len(seen) == 5 and not seen[0][0].guided
    assert [n for _, n in seen[1:]] == [1, 2, 3, 3]
    misses = [name for name, miss in compiled if miss]
    assert len(misses) == 3 and all(name != "engine-loop" for name in misses)
    # add_request on the engine thread: nothing for the plain request, cache hits for the rest
    assert sum(name == "engine-loop" for name, _ in compiled) == 5
    assert seen[3][0].guided_json == BOUNDED and seen[4][0].guided_json == json.dumps(BOUNDED)


def test_proxy_forwards_the_keys_and_maps_response_format():
    seen = []

    async def fake_chat(request):
        seen.append(await request.read())
        return web.json_response({"output": "hi", "meta": {}})

    msgs = [{"role": "user", "content": "x"}]
    bodies = [
        {"messages": msgs, "max_tokens": 3},
        {"messages": msgs, "max_tokens": 3, "response_format": {"type": "text"}},
        {"messages": msgs, "max_tokens": 3, "response_format": {"type": "json_object"}},
        {"messages": msgs, "guided_regex": DIGITS},
        {"messages": msgs, "guided_choice": CHOICES, "guided_regex": None},
        {"messages": msgs, "guided_json": BOUNDED, "temperature": 0.3},
        {"messages": msgs, "response_format": {
            "type": "json_schema", "json_schema": {"name": "verdict", "schema": BOUNDED}}},
        {"messages": msgs, "guided_json": {"type": "null"}, "response_format": {
            "type": "json_schema", "json_schema": {"schema": BOUNDED}}},
        {"messages": msgs, "response_format": {"type": "json_schema"}},
    ]

    async def main():
        app = web.Application()
        app.router.add_post("/chat", fake_chat)
        back, port = await serve(app)
        px, pport = await serve(openai_proxy.create_app(f"http://127.0.0.1:{port}/chat"))
        async with httpx.AsyncClient() as c:
            for b in bodies:
                r = await c.post(f"http://127.0.0.1:{pport}/v1/chat/completions", json=b)
                assert r.status_code == 200
        await px.cleanup()
        await back.cleanup()

    asyncio.run(main())
    # without the keys: byte for byte what the proxy sent before (aiohttp's json= encoding of
    # the prompt and max_tokens alone)
    old = json.dumps({"prompt": "[USER]\nx", "max_tokens": 3}).encode()
    assert seen[0] == seen[1] == seen[2] == old
    got = [json.loads(b) for b in seen[3:]]
    p = {"prompt": "[USER]\nx"}
    assert got[0] == dict(p, guided_regex=DIGITS)
    assert got[1] == dict(p, guided_choice=CHOICES)
    assert got[2] == dict(p, guided_json=BOUNDED)
    assert got[3] == dict(p, guided_json=BOUNDED)
    assert list(got[3]["guided_json"]["properties"]) == list(BOUNDED["properties"])   # order kept
    assert got[4] == dict(p, guided_json={"type": "null"})      # an explicit guided_json wins
    assert got[5] == p


def test_proxy_json_schema_end_to_end():
    from agentic_traffic_testing_amd.testing.stack import LLMBackendThread, cpu_engine

    be = LLMBackendThread(cpu_engine())

    async def main():
        px, pport = await serve(openai_proxy.create_app(f"{be.url}/chat"))
        async with httpx.AsyncClient(timeout=120) as c:
            r = await c.post(f"http://127.0.0.1:{pport}/v1/chat/completions", json={
                "messages": [{"role": "user", "content": "verdict?"}], "max_tokens": 120,
                "temperature": 0.7, "response_format": {
                    "type": "json_schema", "json_schema": {"name": "v", "schema": BOUNDED}}})
        await px.cleanup()
        return r

    try:
        r = asyncio.run(main())
    finally:
        be.stop()
    assert r.status_code == 200
    choice = r.json()["choices"][0]
    validate_bounded(choice["message"]["content"])
