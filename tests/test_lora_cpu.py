"""Multi-LoRA on the CPU engine (fp32 reference ops): adapters against merged checkpoints, the
prefix cache keyed by adapter, the API names and the refusals at start-up."""
import asyncio

import aiohttp
import pytest
import torch
from aiohttp import web

from hipserve.engine.request import SamplingParams
from hipserve.server.api_server import OpenAIServer
from hipserve.server.async_engine import AsyncEngine

from . import lora_cases as LC

GREEDY = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return LC.write_all(str(tmp_path_factory.mktemp("lora")))


def _run(eng, prompts, lora=None):
    import dataclasses

    seqs = [eng.add_request(None, p, dataclasses.replace(GREEDY, lora=lora)) for p in prompts]
    while eng.has_unfinished():
        eng.step()
    return [(s.output_token_ids, s.output_logprobs) for s in seqs]


@pytest.mark.parametrize("name", list(LC.ADAPTERS))
def test_adapter_equals_merged_checkpoint(paths, name):
    """Both runs are fp32: they differ by reassociation only."""
    eng = LC.engine(paths["base"], lora={n: paths[n] for n in LC.ADAPTERS})
    got, base = _run(eng, LC.PROMPTS, name), _run(eng, LC.PROMPTS)
    want = _run(LC.engine(paths[name + "-merged"]), LC.PROMPTS)
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[0] for g in got] != [b[0] for b in base]  # the adapter changes what is generated
    assert torch.allclose(torch.tensor([g[1] for g in got]), torch.tensor([w[1] for w in want]), rtol=0, atol=1e-4)


@pytest.mark.parametrize("name", list(LC.ADAPTERS))
def test_adapter_equals_merged_checkpoint_tp2(paths, name):
    """TP = 2 on gloo: A sliced by K on o / down, B by N on qkv / gate|up, no new collective."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    lora = {n: paths[n] for n in LC.ADAPTERS}
    procs = [ctx.Process(target=LC.tp_worker, args=(r, 2, port, paths["base"], lora, name, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _run(LC.engine(paths[name + "-merged"]), LC.PROMPTS)
    assert [g[0] for g in got] == [w[0] for w in want]
    assert torch.allclose(torch.tensor([g[1] for g in got]), torch.tensor([w[1] for w in want]), rtol=0, atol=1e-4)


def test_prefix_cache_is_keyed_by_adapter(paths):
    eng = LC.engine(paths["base"], lora={"ad1": paths["ad1"]})
    p = [list(range(3, 60))]
    for lora, hit in ((None, 0), ("ad1", 0), ("ad1", 48), (None, 48)):
        before = eng.blocks.prefix_hit_tokens
        _run(eng, p, lora)
        assert eng.blocks.prefix_hit_tokens - before == hit, (lora, hit)


def test_api_lists_and_routes_adapters(paths):
    async def main():
        eng = LC.engine(paths["base"], lora={n: paths[n] for n in LC.ADAPTERS})
        ae = AsyncEngine(eng)
        ae.start(asyncio.get_running_loop())
        runner = web.AppRunner(OpenAIServer(ae, "tiny", eng.max_model_len, lora_names=tuple(eng.lora_names)).app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        base = f"http://127.0.0.1:{site._server.sockets[0].getsockname()[1]}"
        async with aiohttp.ClientSession() as s:
            data = (await (await s.get(base + "/v1/models")).json())["data"]
            assert [(d["id"], d.get("parent")) for d in data] == [("tiny", None), ("ad1", "tiny"), ("ad2", "tiny")]
            out = {}
            for m in ("tiny", "ad2", "nope"):
                r = await s.post(base + "/v1/completions", json={"model": m, "prompt": LC.PROMPTS[0], "max_tokens": 6,
                                                                 "temperature": 0, "ignore_eos": True})
                out[m] = (r.status, (await r.json()).get("choices", [{}])[0].get("text"))
            assert out["nope"][0] == 404 and out["tiny"][0] == out["ad2"][0] == 200
            assert out["tiny"][1] != out["ad2"][1]
        await runner.cleanup()
        ae.stop()

    asyncio.run(main())


@pytest.mark.parametrize("what,cfg,kw", [
    ("DoRA", {"use_dora": True}, {}),
    ("modules_to_save", {"modules_to_save": ["lm_head"]}, {}),
    ("rank 32", {}, {"max_lora_rank": 16}),
])
def test_refused_adapters_are_named(paths, tmp_path, what, cfg, kw):
    K = LC.CFG.hidden_size
    t = {"base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(32, K),
         "base_model.model.model.layers.0.self_attn.q_proj.lora_B.weight": torch.zeros(K, 32)}
    bad = LC.write_adapter(str(tmp_path / "bad"), t, r=32, lora_alpha=32, **cfg)
    with pytest.raises(ValueError, match=f"'badname'.*{what}"):
        LC.engine(paths["base"], lora={"badname": bad}, **({"max_lora_rank": 64} | kw))


def test_forced_single_layout_is_refused(paths, monkeypatch):
    monkeypatch.setenv("HIPSERVE_SINGLE_LAYOUT", "1")
    with pytest.raises(ValueError, match="single layout"):
        LC.engine(paths["base"], lora={"ad1": paths["ad1"]})
