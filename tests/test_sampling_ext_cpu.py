"""min_p and logit_bias on the request surface (CPU): SamplingParams validation, the
OpenAI endpoints, the CPU engine's slot lifecycle, the reference ops, and the
StepInputs broadcast under TP = 2 (gloo)."""
import asyncio
import math
import os

import aiohttp
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from hipserve.config import EngineConfig
from hipserve.engine.llm_engine import LLMEngine
from hipserve.engine.request import MAX_LOGIT_BIAS, SamplingParams
from hipserve.ops import reference as ref
from hipserve.parallel.comm import TPGroup

from .test_server import start_engine_server
from .test_tp_cpu import PROMPTS, _cfg, _port

A = 3 + ord("A")  # SyntheticTokenizer: byte b is id 3 + b


# ------------------------------------------------------------------ SamplingParams
@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), "x", True, [0.1]])
def test_min_p_range(bad):
    with pytest.raises(ValueError):
        SamplingParams(min_p=bad)


def test_min_p_and_bias_defaults_are_off():
    sp = SamplingParams()
    assert sp.min_p == 0.0 and sp.logit_bias == []
    assert SamplingParams(min_p="0.25").min_p == 0.25
    assert SamplingParams(logit_bias={}).logit_bias == []


@pytest.mark.parametrize("bad", [[1, 2], "5", 7, [[1, 2.0]], {"a": 1.0}, {"1.5": 1.0}, {-1: 1.0},
                                 {5: 100.5}, {5: -101}, {5: "x"}, {5: None}, {5: float("inf")},
                                 {"12": 1.0, 12: 2.0}, {"12": 1.0, " 12": 2.0},
                                 {i: 0.5 for i in range(MAX_LOGIT_BIAS + 1)}])
def test_logit_bias_rejected(bad):
    with pytest.raises(ValueError):
        SamplingParams(logit_bias=bad)


def test_logit_bias_normalised():
    sp = SamplingParams(logit_bias={"12": 1, 7: -100, "300": 100.0})
    assert sp.logit_bias == [(7, -100.0), (12, 1.0), (300, 100.0)]
    assert all(isinstance(t, int) and isinstance(b, float) for t, b in sp.logit_bias)
    assert len(SamplingParams(logit_bias={i: 0.5 for i in range(MAX_LOGIT_BIAS)}).logit_bias) == MAX_LOGIT_BIAS
    # the n > 1 fan-out rebuilds the params from their own fields
    again = SamplingParams(**{**sp.__dict__, "n": 1})
    assert again.logit_bias == sp.logit_bias
    sp.check_vocab(301)
    with pytest.raises(ValueError):
        sp.check_vocab(300)


# ------------------------------------------------------------------ reference ops
def test_reference_min_p_keep_set():
    """ref.sample with min_p never leaves {p_i >= min_p * p_max}; min_p = 1 is the argmax;
    min_p = 0 and None are the plain draw."""
    torch.manual_seed(0)
    B, V = 6, 500
    x = torch.randn(B, V) * 3
    temp = torch.tensor([1.0, 0.7, 1.5, 1.0, 0.0, 1.0])
    tk = torch.zeros(B, dtype=torch.int32)
    tp = torch.ones(B)
    mp_ = torch.tensor([0.1, 0.3, 0.05, 1.0, 0.5, 0.0])
    seeds, steps = torch.arange(B) + 5, torch.zeros(B, dtype=torch.long)
    for step in range(20):
        steps[:] = step
        tok, _ = ref.sample(x, temp, tk, tp, seeds, steps, bf16_row=False, min_p=mp_)
        t0, _ = ref.sample(x, temp, tk, tp, seeds, steps, bf16_row=False)
        tz, _ = ref.sample(x, temp, tk, tp, seeds, steps, bf16_row=False, min_p=torch.zeros(B))
        assert torch.equal(t0, tz) and tok[5] == t0[5]
        for r in range(4):
            p = torch.softmax(x[r] / temp[r], 0)
            assert p[tok[r]] >= mp_[r] * p.max() * (1 - 1e-5)
        assert tok[3] == x[3].argmax() and tok[4] == x[4].argmax()


def test_reference_logit_bias_apply():
    V = 50
    for dtype in (torch.float32, torch.bfloat16):
        logits = torch.randn(3, V).to(dtype)
        before = logits.clone()
        ids = torch.zeros(2, 4, dtype=torch.int32)
        vals = torch.zeros(2, 4)
        ids[1, :3] = torch.tensor([0, V - 1, 7])
        vals[1, :3] = torch.tensor([1.5, -100.0, 100.0])
        n = torch.tensor([0, 3], dtype=torch.int32)
        ref.logit_bias_apply(logits, torch.tensor([-1, 0, 1], dtype=torch.int32), ids, vals, n)
        assert torch.equal(logits[:2], before[:2])  # no slot / empty slot: untouched
        want = before[2].float()
        want[0] += 1.5
        want[V - 1] -= 100.0
        want[7] += 100.0
        assert torch.equal(logits[2], want.to(dtype))


# ------------------------------------------------------------------ CPU engine
def _engine(max_num_seqs=4):
    return LLMEngine(EngineConfig(model="tiny-llama", device="cpu", dtype="float32", max_num_seqs=max_num_seqs,
                                  max_num_batched_tokens=64, num_kv_blocks=128, max_model_len=256), tp=TPGroup())


def test_engine_min_p_one_is_greedy_and_bias_bans():
    eng = _engine()
    greedy = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    want = [r[0] for r in eng.generate(PROMPTS, greedy)]
    got = [r[0] for r in eng.generate(PROMPTS, SamplingParams(temperature=0.9, seed=3, min_p=1.0, max_tokens=10,
                                                               ignore_eos=True))]
    assert got == want
    # ban the token the plain run emits most: it never appears, the output changes
    top = max(set(want[0]), key=want[0].count)
    ban = eng.generate(PROMPTS[:1], SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True,
                                                   logit_bias={str(top): -100}))[0][0]
    assert top not in ban and ban != want[0]
    # +100 forces a token, sampled or greedy
    forced = eng.generate(PROMPTS[:1], SamplingParams(temperature=1.0, seed=1, max_tokens=6, ignore_eos=True,
                                                      logit_bias={9: 100}))[0][0]
    assert forced == [9] * 6
    r = eng.runner
    assert len(r._free_bias) == r.bias_n.shape[0] and sorted(r._free_bias) == list(range(r.bias_n.shape[0]))
    with pytest.raises(ValueError):
        eng.add_request(None, [1, 2], SamplingParams(logit_bias={eng.model_cfg.vocab_size: 1.0}))


def test_engine_n2_fanout_holds_two_bias_slots():
    """The n > 1 fan-out copies the params: each copy takes its own slot, both give
    it back; an abort in flight returns its slot too."""
    eng = _engine()
    r = eng.runner
    nslots = r.bias_n.shape[0]
    base = SamplingParams(temperature=0.8, seed=5, max_tokens=5, ignore_eos=True, n=2, logit_bias={A: 100, 9: -3})
    copies = [SamplingParams(**{**base.__dict__, "n": 1, "seed": base.seed + j}) for j in range(2)]
    seqs = [eng.add_request(None, [1, 5, 6], sp) for sp in copies]
    plain = eng.add_request(None, [1, 5, 6], SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True))
    out = {s.request_id: [] for s in seqs + [plain]}
    for o in eng.step():
        out[o.request_id] += o.new_token_ids
    assert len(r._free_bias) == nslots - 2 and plain.bias_slot is None
    assert sorted(s.bias_slot for s in seqs) == sorted(set(range(nslots)) - set(r._free_bias))
    for s in seqs:
        assert r.bias_n[s.bias_slot] == 2 and r.bias_ids[s.bias_slot, :2].tolist() == [9, A]
    while eng.has_unfinished():
        for o in eng.step():
            out[o.request_id] += o.new_token_ids
    assert all(out[s.request_id] == [A] * 5 for s in seqs) and out[plain.request_id] != [A] * 5
    assert len(r._free_bias) == nslots
    s = eng.add_request(None, [1, 5, 6], copies[0])
    eng.step()
    assert len(r._free_bias) == nslots - 1
    eng.abort(s.request_id)
    assert len(r._free_bias) == nslots and s.bias_slot is None


# ------------------------------------------------------------------ HTTP
def test_http_min_p_and_logit_bias():
    async def main():
        ae, runner, port = await start_engine_server()
        base = f"http://127.0.0.1:{port}"
        V = ae.engine.model_cfg.vocab_size
        msgs = [{"role": "user", "content": "hi"}]
        async with aiohttp.ClientSession() as s:
            # both parameters on both endpoints
            r = await s.post(base + "/v1/completions", json={
                "model": "tiny", "prompt": "hello", "max_tokens": 5, "temperature": 0.8, "seed": 1,
                "min_p": 0.1, "logit_bias": {"70": -5, "71": 2.5}, "ignore_eos": True})
            j = await r.json()
            assert r.status == 200 and j["usage"]["completion_tokens"] == 5, j
            r = await s.post(base + "/v1/chat/completions", json={
                "model": "tiny", "messages": msgs, "max_tokens": 4, "min_p": 0.2, "logit_bias": {"70": 1},
                "ignore_eos": True})
            j = await r.json()
            assert r.status == 200 and j["usage"]["completion_tokens"] == 4, j
            # +100 with greedy decoding yields only that id (byte 'A'), also per choice of n = 2
            r = await s.post(base + "/v1/completions", json={
                "model": "tiny", "prompt": "hello", "max_tokens": 6, "temperature": 0,
                "logit_bias": {str(A): 100}, "ignore_eos": True})
            j = await r.json()
            assert r.status == 200 and j["choices"][0]["text"] == "A" * 6, j
            r = await s.post(base + "/v1/chat/completions", json={
                "model": "tiny", "messages": msgs, "max_tokens": 3, "n": 2, "temperature": 0.7,
                "logit_bias": {str(A): 100}, "ignore_eos": True})
            j = await r.json()
            assert r.status == 200 and [c["message"]["content"] for c in j["choices"]] == ["AAA", "AAA"], j
            # bad values: 400 JSON errors, also for a stream (before any SSE header)
            for extra in ({"logit_bias": {str(V): 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": [[1, 2]]},
                          {"logit_bias": {"5": 101}}, {"logit_bias": {"x": 1}}, {"min_p": 1.5}, {"min_p": -0.1},
                          {"logit_bias": {str(i): 1 for i in range(301)}}):
                for path, body in (("/v1/completions", {"prompt": "x"}), ("/v1/chat/completions", {"messages": msgs})):
                    r = await s.post(base + path, json={"model": "tiny", "stream": True, **body, **extra})
                    j = await r.json()
                    assert r.status == 400 and "error" in j, (extra, j)
            # the engine survived and nothing holds a slot
            r = await s.post(base + "/v1/completions", json={"model": "tiny", "prompt": "x", "max_tokens": 2})
            assert r.status == 200
        run = ae.engine.runner
        assert len(run._free_bias) == run.bias_n.shape[0]
        ae.stop()
        await runner.cleanup()

    asyncio.run(main())


# ------------------------------------------------------------------ TP
def _params():
    return [SamplingParams(temperature=0.8, seed=11, min_p=0.1, logit_bias={5: 4.0, 9: -100, 70: 2.0},
                           max_tokens=8, ignore_eos=True),
            SamplingParams(temperature=0.0, logit_bias={str(A): 100}, max_tokens=8, ignore_eos=True),
            SamplingParams(temperature=1.2, seed=4, min_p=0.3, max_tokens=8, ignore_eos=True)]


def _worker(rank, world, port, ckpt, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from hipserve.config import resolve_model_config
    from hipserve.engine.llm_engine import worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.parallel.comm import init_tp

    tp = init_tp(world, backend="gloo", device_type="cpu")
    cfg = _cfg(ckpt, world)
    try:
        if rank == 0:
            eng = LLMEngine(cfg, tp=tp)
            res = eng.generate(PROMPTS, _params())
            eng.shutdown()
            q.put(([r[0] for r in res], None))
        else:
            runner = ModelRunner(cfg, resolve_model_config(ckpt), tp)
            worker_loop(runner, tp)
            # the worker filled its own copy of the slot tables from the broadcast inputs
            q.put((None, (runner.bias_n.tolist(), runner.bias_ids[:, :3].tolist())))
    finally:
        dist.destroy_process_group()
    q.close()
    q.join_thread()
    os._exit(0)


def test_tp2_matches_tp1_with_min_p_and_bias():
    ref_eng = LLMEngine(_cfg("tiny-llama", 1), tp=TPGroup())
    want = [r[0] for r in ref_eng.generate(PROMPTS, _params())]
    assert want[1] == [A] * 8 and 9 not in want[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, "tiny-llama", q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    toks = next(t for t, _ in got if t is not None)
    bias_n, bias_ids = next(w for _, w in got if w is not None)
    assert toks == want
    assert sorted(bias_n, reverse=True)[:2] == [3, 1]
    assert [5, 9, 70] in bias_ids and math.isclose(sum(bias_n), 4)
