"""HTTP interface of prompt scoring on a CPU engine: OpenAI ``echo`` (+ ``logprobs``) on
/v1/completions and vLLM's ``prompt_logprobs`` on both endpoints, streaming, n > 1, bad
values, and the unchanged shape of a request without the new fields."""
import asyncio

import aiohttp
import pytest

from .test_server import sse_events, start_engine_server

PROMPT = [1, 5, 6, 7, 9, 11]


def _serve(fn):
    async def main():
        ae, runner, port = await start_engine_server()
        try:
            async with aiohttp.ClientSession() as s:
                await fn(s, f"http://127.0.0.1:{port}", ae)
        finally:
            ae.stop()
            await runner.cleanup()

    asyncio.run(main())


def _check_vllm(plp, ids, k, tok):
    """null, then {token id as a string: {"logprob", "rank", "decoded_token"}} per prompt
    token: the token itself plus the top k."""
    assert len(plp) == len(ids) and plp[0] is None
    for t, d in zip(ids[1:], plp[1:]):
        own = d[str(t)]
        assert set(own) == {"logprob", "rank", "decoded_token"}
        assert own["logprob"] <= 0 and own["rank"] >= 1 and own["decoded_token"] == tok.decode([t])
        assert k <= len(d) <= k + 1
        by_rank = sorted(d.values(), key=lambda e: e["rank"])
        assert [e["rank"] for e in by_rank[:k]] == list(range(1, k + 1))
        assert all(a["logprob"] >= b["logprob"] for a, b in zip(by_rank, by_rank[1:]))
        assert (len(d) == k) == (own["rank"] <= k)


def _own(choice, ids):
    """The prompt tokens' own log-probs of a choice's prompt_logprobs."""
    return [d[str(t)]["logprob"] for t, d in zip(ids[1:], choice["prompt_logprobs"][1:])]


def test_echo_and_prompt_logprobs_on_completions():
    async def fn(s, base, ae):
        tok = ae.engine.tokenizer
        body = {"model": "tiny", "prompt": PROMPT, "max_tokens": 3, "temperature": 0, "ignore_eos": True}
        plain = await (await s.post(base + "/v1/completions", json=body)).json()
        # the response of a request without the new fields has exactly today's keys
        assert set(plain) == {"id", "object", "created", "model", "choices", "usage"}
        assert set(plain["choices"][0]) == {"index", "text", "logprobs", "finish_reason"}
        with_lp = await (await s.post(base + "/v1/completions", json={**body, "logprobs": 2})).json()
        assert set(with_lp["choices"][0]["logprobs"]) == {"tokens", "token_logprobs"}
        scored0 = ae.engine.runner.stats.get("prompt_logprob_rows", 0)
        assert scored0 == 0
        # echo alone: the prompt text in front (a token-id prompt is detokenised), no device work
        j = await (await s.post(base + "/v1/completions", json={**body, "echo": True})).json()
        ch = j["choices"][0]
        assert ch["text"] == tok.decode(PROMPT) + plain["choices"][0]["text"] and ch["logprobs"] is None
        assert set(ch) == {"index", "text", "logprobs", "finish_reason"}
        j = await (await s.post(base + "/v1/completions", json={**body, "prompt": "hello there", "echo": True})).json()
        assert j["choices"][0]["text"].startswith("hello there")
        assert ae.engine.runner.stats.get("prompt_logprob_rows", 0) == 0
        # echo + logprobs: prompt tokens first, then the generated ones (lm-eval's request)
        j = await (await s.post(base + "/v1/completions", json={**body, "echo": True, "logprobs": 1,
                                                                "max_tokens": 1})).json()
        lp = j["choices"][0]["logprobs"]
        n = len(PROMPT) + 1
        assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
        assert all(len(lp[k]) == n for k in lp)
        assert lp["tokens"][:len(PROMPT)] == [tok.decode([t]) for t in PROMPT]
        assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
        assert all(v <= 0 for v in lp["token_logprobs"][1:])
        assert all(len(d) == 1 for d in lp["top_logprobs"][1:])
        assert lp["token_logprobs"][-1] == with_lp["choices"][0]["logprobs"]["token_logprobs"][0]
        for t, v, d in zip(lp["tokens"][1:], lp["token_logprobs"][1:], lp["top_logprobs"][1:]):
            (best, bv), = d.items()
            assert bv >= v and (bv > v or best == t)  # the top-1 is the token itself or beats it
        assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])
        assert lp["text_offset"][-1] == len("".join(lp["tokens"][:-1]))
        assert "prompt_logprobs" not in j["choices"][0]
        assert ae.engine.runner.stats["prompt_logprob_rows"] == len(PROMPT) - 1
        # prompt_logprobs (vLLM): every choice gains the list; same numbers as the echo form
        j = await (await s.post(base + "/v1/completions", json={**body, "prompt_logprobs": 2})).json()
        ch = j["choices"][0]
        assert set(ch) == {"index", "text", "logprobs", "finish_reason", "prompt_logprobs"}
        assert ch["text"] == plain["choices"][0]["text"]
        _check_vllm(ch["prompt_logprobs"], PROMPT, 2, tok)
        own = [d[str(t)]["logprob"] for t, d in zip(PROMPT[1:], ch["prompt_logprobs"][1:])]
        assert own == pytest.approx(lp["token_logprobs"][1:len(PROMPT)], abs=1e-6)
        # prompt_logprobs: 0 = the token's own entry only
        j = await (await s.post(base + "/v1/completions", json={**body, "prompt_logprobs": 0})).json()
        assert all(list(d) == [str(t)] for t, d in zip(PROMPT[1:], j["choices"][0]["prompt_logprobs"][1:]))

    _serve(fn)


def test_n2_scores_the_prompt_once_and_streaming_carries_it_first():
    async def fn(s, base, ae):
        tok = ae.engine.tokenizer
        body = {"model": "tiny", "prompt": PROMPT, "max_tokens": 3, "temperature": 0.8, "seed": 3, "ignore_eos": True,
                "n": 2, "prompt_logprobs": 1}
        j = await (await s.post(base + "/v1/completions", json=body)).json()
        assert len(j["choices"]) == 2
        assert j["choices"][0]["prompt_logprobs"] == j["choices"][1]["prompt_logprobs"]
        _check_vllm(j["choices"][0]["prompt_logprobs"], PROMPT, 1, tok)
        assert ae.engine.runner.stats["prompt_logprob_rows"] == len(PROMPT) - 1  # once, not per choice
        # streaming, echo + logprobs + prompt_logprobs, n = 2: the first chunk of each choice
        # carries the prompt part, later chunks keep today's shape
        r = await s.post(base + "/v1/completions", json={**body, "stream": True, "echo": True, "logprobs": 1})
        ev = [e for e in await sse_events(r) if e != "[DONE]"]
        firsts = []
        for idx in (0, 1):
            mine = [e["choices"][0] for e in ev if e["choices"] and e["choices"][0]["index"] == idx]
            assert len(mine) == 3
            first = mine[0]
            assert first["text"].startswith(tok.decode(PROMPT))
            firsts.append(first["prompt_logprobs"])
            assert _own(first, PROMPT) == pytest.approx(_own(j["choices"][0], PROMPT), abs=1e-5)
            assert first["logprobs"]["token_logprobs"][1:len(PROMPT)] == _own(first, PROMPT)
            assert len(first["logprobs"]["tokens"]) == len(PROMPT) + 1
            assert first["logprobs"]["token_logprobs"][0] is None and first["logprobs"]["top_logprobs"][0] is None
            for later in mine[1:]:
                assert "prompt_logprobs" not in later and set(later["logprobs"]) == {"tokens", "token_logprobs"}
                assert not later["text"].startswith(tok.decode(PROMPT))
        assert firsts[0] == firsts[1]  # one scoring, copied
        assert ae.engine.runner.stats["prompt_logprob_rows"] == 2 * (len(PROMPT) - 1)
        # two prompts x n = 2: each prompt's choices carry that prompt's list
        other = [1, 8, 8, 3]
        j2 = await (await s.post(base + "/v1/completions", json={**body, "prompt": [PROMPT, other]})).json()
        assert [c["index"] for c in j2["choices"]] == [0, 1, 2, 3]
        assert j2["choices"][1]["prompt_logprobs"] == j2["choices"][0]["prompt_logprobs"]
        assert j2["choices"][2]["prompt_logprobs"] == j2["choices"][3]["prompt_logprobs"]
        assert _own(j2["choices"][1], PROMPT) == pytest.approx(_own(j["choices"][0], PROMPT), abs=1e-5)
        _check_vllm(j2["choices"][3]["prompt_logprobs"], other, 1, tok)

    _serve(fn)


def test_chat_prompt_logprobs():
    async def fn(s, base, ae):
        tok = ae.engine.tokenizer
        msgs = [{"role": "user", "content": "hi"}]
        ids = tok.encode_chat(msgs, add_generation_prompt=True)
        body = {"model": "tiny", "messages": msgs, "max_tokens": 3, "ignore_eos": True, "temperature": 0}
        plain = await (await s.post(base + "/v1/chat/completions", json=body)).json()
        assert set(plain["choices"][0]) == {"index", "message", "logprobs", "finish_reason"}
        j = await (await s.post(base + "/v1/chat/completions", json={**body, "prompt_logprobs": 3, "n": 2})).json()
        assert len(j["choices"]) == 2
        for ch in j["choices"]:
            assert set(ch) == {"index", "message", "logprobs", "finish_reason", "prompt_logprobs"}
            _check_vllm(ch["prompt_logprobs"], ids, 3, tok)
        assert j["choices"][0]["prompt_logprobs"] == j["choices"][1]["prompt_logprobs"]
        assert j["choices"][0]["message"] == plain["choices"][0]["message"]
        # echo is a completions field: ignored here
        r = await s.post(base + "/v1/chat/completions", json={**body, "prompt_logprobs": 3, "stream": True})
        ev = [e for e in await sse_events(r) if e != "[DONE]"]
        assert ev[0]["choices"][0]["delta"]["role"] == "assistant" and "prompt_logprobs" not in ev[0]["choices"][0]
        content = [e["choices"][0] for e in ev[1:] if e["choices"]]
        _check_vllm(content[0]["prompt_logprobs"], ids, 3, tok)
        assert _own(content[0], ids) == pytest.approx(_own(j["choices"][0], ids), abs=1e-5)
        assert all("prompt_logprobs" not in c for c in content[1:])

    _serve(fn)


def test_bad_values_are_400_before_any_stream():
    async def fn(s, base, ae):
        for extra in ({"prompt_logprobs": "2"}, {"prompt_logprobs": -1}, {"prompt_logprobs": 21},
                      {"prompt_logprobs": True}, {"prompt_logprobs": 1.5}, {"echo": "yes"}, {"echo": 1},
                      {"echo": True, "logprobs": 21}):
            for stream in (False, True):
                r = await s.post(base + "/v1/completions", json={"model": "tiny", "prompt": PROMPT, "max_tokens": 2,
                                                                 "stream": stream, **extra})
                assert r.status == 400, (extra, stream, await r.text())
                assert r.headers["Content-Type"].startswith("application/json")
        for extra in ({"prompt_logprobs": "2"}, {"prompt_logprobs": -1}, {"prompt_logprobs": 21}):
            r = await s.post(base + "/v1/chat/completions", json={
                "model": "tiny", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 2, "stream": True,
                **extra})
            assert r.status == 400, (extra, await r.text())
        # an image prompt with the field is refused (placeholder rows have no target)
        r = await s.post(base + "/v1/chat/completions", json={
            "model": "tiny", "max_tokens": 2, "prompt_logprobs": 1, "messages": [{"role": "user", "content": [
                {"type": "text", "text": "what is this?"},
                {"type": "image_url", "image_url": {"url": "data:image/png;base64,AAAA"}}]}]})
        assert r.status == 400 and "prompt_logprobs" in (await r.json())["error"]["message"]
        assert (await s.get(base + "/health")).status == 200

    _serve(fn)
