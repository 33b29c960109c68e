"""GGUF tier, architecture ``gemma3``: metadata -> ModelConfig, the sandwich / q / k norm
tensors (stored with Gemma's + 1 already added), tied output, ``add_space_prefix``.

No Gemma GGUF exists offline: the files are written here from a tiny ``transformers``
Gemma-3 following llama.cpp's conventions (key names as in transformers' own
GGUF_CONFIG_MAPPING["gemma3"], no query_pre_attn_scalar, no layer types: every 6th layer
global). CPU: greedy parity with transformers. GPU: head_dim 256 with Q8_0 / Q4_K matrices,
i.e. quant blocks + GeGLU + sandwich norms + the head_dim-256 attention kernels together."""
import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

from hipserve.config import EngineConfig  # noqa: E402
from hipserve.engine.llm_engine import LLMEngine  # noqa: E402
from hipserve.engine.request import SamplingParams  # noqa: E402
from hipserve.parallel.comm import TPGroup  # noqa: E402
from hipserve.weights import gguf as G  # noqa: E402

WINDOW, FACTOR = 8, 2.0


def _hf_model(hidden, head_dim, inter, vocab, window=WINDOW):
    cfg = transformers.Gemma3TextConfig(
        hidden_size=hidden, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2, vocab_size=vocab,
        max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=True, intermediate_size=inter,
        head_dim=head_dim, query_pre_attn_scalar=head_dim, sliding_window=window,
        rope_parameters={"sliding_attention": {"rope_type": "default", "rope_theta": 1e4},
                         "full_attention": {"rope_type": "linear", "factor": FACTOR, "rope_theta": 1e6}},
        layer_types=["sliding_attention"] * 5 + ["full_attention"])
    torch.manual_seed(1234)
    m = transformers.AutoModelForCausalLM.from_config(cfg, torch_dtype=torch.float32).eval()
    with torch.no_grad():
        for _name, p in m.named_parameters():
            if p.dim() == 1:  # non-trivial norm weights (HF initialises them to 0)
                p.add_(torch.randn_like(p) * 0.1)
    return m


def _tokens(V):
    toks = ["<unk>", "<s>", "</s>"] + [f"<0x{b:02X}>" for b in range(256)] + ["▁", "w", "1", "w1", "▁w", "▁w1"]
    return toks + [f"▁x{i}" for i in range(V - len(toks))]


def _write_gemma3_gguf(m, path, qtype=G.F32, arch="gemma3", space_prefix=None, window=WINDOW):
    """The HF model as a llama.cpp ``gemma3`` file: + 1 on every norm weight, matrices in
    ``qtype``, no output.weight (tied), rope.scaling.* for the global layers."""
    c = m.config
    sd = {k: v.detach().float().numpy() for k, v in m.state_dict().items()}
    H, V, L, a = c.hidden_size, c.vocab_size, c.num_hidden_layers, arch
    toks = _tokens(V)
    md = {"general.architecture": a, "general.name": "tiny-gemma3", f"{a}.context_length": 4096,
          f"{a}.embedding_length": H, f"{a}.block_count": L, f"{a}.feed_forward_length": c.intermediate_size,
          f"{a}.attention.head_count": c.num_attention_heads, f"{a}.attention.head_count_kv": c.num_key_value_heads,
          f"{a}.attention.key_length": c.head_dim, f"{a}.attention.value_length": c.head_dim,
          f"{a}.attention.layer_norm_rms_epsilon": float(c.rms_norm_eps), f"{a}.attention.sliding_window": window,
          f"{a}.rope.freq_base": 1e6, f"{a}.rope.scaling.type": "linear", f"{a}.rope.scaling.factor": FACTOR,
          "tokenizer.ggml.model": "llama", "tokenizer.ggml.tokens": toks,
          "tokenizer.ggml.scores": [float(-i) for i in range(len(toks))],
          "tokenizer.ggml.token_type": [3 if i < 3 else (6 if i < 259 else 1) for i in range(len(toks))],
          "tokenizer.ggml.bos_token_id": 1, "tokenizer.ggml.eos_token_id": 2}
    if space_prefix is not None:
        md["tokenizer.ggml.add_space_prefix"] = space_prefix
    t = [("token_embd.weight", sd["model.embed_tokens.weight"], G.F32),
         ("output_norm.weight", 1 + sd["model.norm.weight"], G.F32)]
    for i in range(L):
        p, b = f"model.layers.{i}.", f"blk.{i}."
        t += [(b + n + ".weight", 1 + sd[p + hf + ".weight"], G.F32) for n, hf in (
            ("attn_norm", "input_layernorm"), ("post_attention_norm", "post_attention_layernorm"),
            ("ffn_norm", "pre_feedforward_layernorm"), ("post_ffw_norm", "post_feedforward_layernorm"),
            ("attn_q_norm", "self_attn.q_norm"), ("attn_k_norm", "self_attn.k_norm"))]
        t += [(b + n + ".weight", sd[p + hf + ".weight"], qtype) for n, hf in (
            ("attn_q", "self_attn.q_proj"), ("attn_k", "self_attn.k_proj"), ("attn_v", "self_attn.v_proj"),
            ("attn_output", "self_attn.o_proj"), ("ffn_gate", "mlp.gate_proj"), ("ffn_up", "mlp.up_proj"),
            ("ffn_down", "mlp.down_proj"))]
    G.write_gguf(path, md, [(n, np.ascontiguousarray(x), q) for n, x, q in t])
    return path


@pytest.fixture(scope="module")
def tiny():
    return _hf_model(hidden=64, head_dim=32, inter=128, vocab=320)


def test_gemma3_gguf_matches_transformers(tmp_path, tiny):
    p = _write_gemma3_gguf(tiny, str(tmp_path / "gemma3.gguf"))
    eng = LLMEngine(EngineConfig(model=p, device="cpu", dtype="float32", load_format="gguf", max_num_seqs=4,
                                 max_num_batched_tokens=24, num_kv_blocks=128, max_model_len=256), tp=TPGroup())
    assert eng.runner.model.cfg.family == "gemma3"
    prompts = [[1, 5, 9, 33, 70, 100], list(range(3, 40)), [7] * 11]
    res = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    for pr, (toks, _, reason) in zip(prompts, res):
        assert reason == "length" and len(toks) == 8
        with torch.no_grad():
            lg = tiny(torch.tensor([list(pr) + list(toks)])).logits[0].float()
        for i, t in enumerate(toks):
            row = lg[len(pr) - 1 + i]
            assert row[t] >= row.max() - 1e-4, (i, t, int(row.argmax()), float(row.max() - row[t]))


def test_gemma3_gguf_model_config(tmp_path, tiny):
    c = G.GGUFFile(_write_gemma3_gguf(tiny, str(tmp_path / "gemma3.gguf"))).model_config()
    assert c.family == "gemma3" and c.architecture == "llama" and c.head_dim == 32 and c.num_layers == 6
    assert c.qk_norm and c.sandwich_norm and c.norm_offset and c.hidden_act == "gelu_tanh" and c.rope_mode == 0
    assert c.attn_scale == 32 ** -0.5 and c.embed_scale == 8.0
    assert c.sliding_window == WINDOW and c.layer_windows == (WINDOW,) * 5 + (0,)
    assert c.rope_theta == 1e6 and c.rope_local_theta == 1e4
    assert c.rope_scaling == {"rope_type": "linear", "factor": FACTOR}
    assert c.tie_word_embeddings and c.vocab_size == 320


def test_gemma3_gguf_27b_geometry_scale():
    """62 layers: query_pre_attn_scalar is hidden / heads (168 at the 27B), not key_length."""
    gf = G.GGUFFile.__new__(G.GGUFFile)
    gf.path, gf.tensors = "27b.gguf", {}
    gf.metadata = {"general.architecture": "gemma3", "gemma3.embedding_length": 5376, "gemma3.block_count": 62,
                   "gemma3.attention.head_count": 32, "gemma3.attention.head_count_kv": 16,
                   "gemma3.attention.key_length": 128, "gemma3.feed_forward_length": 21504,
                   "gemma3.attention.sliding_window": 1024, "tokenizer.ggml.tokens": ["a", "b"]}
    c = gf.model_config()
    assert abs(c.attn_scale - 168 ** -0.5) < 1e-12 and c.rope_scaling is None and len(c.layer_windows) == 62


@pytest.mark.parametrize("arch", ["gemma", "gemma2"])
def test_gemma_1_2_gguf_refused(tmp_path, tiny, arch):
    p = _write_gemma3_gguf(tiny, str(tmp_path / f"{arch}.gguf"), arch=arch)
    with pytest.raises(NotImplementedError, match="soft-capping"):
        G.GGUFFile(p).model_config()


def test_gguf_tokenizer_add_space_prefix(tmp_path, tiny):
    toks = _tokens(320)
    enc = {}
    for key, flag in (("default", None), ("on", True), ("off", False)):
        p = _write_gemma3_gguf(tiny, str(tmp_path / f"{key}.gguf"), space_prefix=flag)
        enc[key] = G.GGUFTokenizer(G.GGUFFile(p)).encode("w1", add_special_tokens=False)
    assert enc["default"] == enc["on"] == [toks.index("▁w1")]  # as before: the dummy prefix
    assert enc["off"] == [toks.index("w1")]


def test_gemma3_gguf_serves_through_llama_server_flags(tmp_path, tiny):
    """The chart's ``hipserve-llama-server --model <file.gguf> --alias <name>`` arguments build an
    engine on the file, and the OpenAI endpoints answer a text prompt through its tokenizer."""
    import asyncio

    import aiohttp
    from aiohttp import web

    from hipserve.server.api_server import OpenAIServer
    from hipserve.server.async_engine import AsyncEngine
    from hipserve.server.cli import build_parser, config_from_args

    p = _write_gemma3_gguf(tiny, str(tmp_path / "gemma3.gguf"), space_prefix=False)
    a = build_parser("llama-server").parse_args(["--host", "127.0.0.1", "--port", "8080", "--model", p,
                                                 "--alias", "gemma3-tiny"])
    cfg = config_from_args(a).replace(device="cpu", dtype="float32", num_kv_blocks=128, max_model_len=256,
                                      max_num_batched_tokens=64)
    eng = LLMEngine(cfg, tp=TPGroup())
    assert eng.runner.model.cfg.family == "gemma3" and cfg.model_name == "gemma3-tiny"

    async def main():
        ae = AsyncEngine(eng)
        ae.start(asyncio.get_running_loop())
        runner = web.AppRunner(OpenAIServer(ae, cfg.model_name, eng.max_model_len).app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        base = f"http://127.0.0.1:{site._server.sockets[0].getsockname()[1]}"
        async with aiohttp.ClientSession() as s:
            r = await s.post(base + "/v1/completions", json={"model": "gemma3-tiny", "prompt": "w1 w1",
                                                             "max_tokens": 5, "temperature": 0, "ignore_eos": True})
            j = await r.json()
            assert r.status == 200 and j["usage"]["completion_tokens"] == 5, j
            # bos + "w1" + "▁w1": no dummy prefix piece in front of the first word
            assert j["usage"]["prompt_tokens"] == 3, j
        ae.stop()
        await runner.cleanup()

    asyncio.run(main())


PROMPTS = [[1] + list(range(10, 300)), [1, 7, 8, 9], [1] + [42] * 40, list(range(3, 600))]


@pytest.mark.gpu
@pytest.mark.parametrize("qtype", [G.Q8_0, G.Q4_K], ids=["q8_0", "q4_k"])
def test_gemma3_gguf_d256_gpu(tmp_path, qtype):
    """head_dim 256, hidden 256, quantised matrices kept as blocks: graph == eager on the
    first two tokens, first token == the CPU engine loading the same file."""
    from hipserve.ops.quant import QuantWeight

    m = _hf_model(hidden=256, head_dim=256, inter=512, vocab=1024, window=64)
    p = _write_gemma3_gguf(m, str(tmp_path / "gemma3-d256.gguf"), qtype=qtype, window=64)
    out = {}
    for device, eager in (("cuda", False), ("cuda", True), ("cpu", True)):
        dt = "bfloat16" if device == "cuda" else "float32"
        dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
        eng = LLMEngine(EngineConfig(model=p, device=device, dtype=dt, load_format="gguf", max_num_seqs=16,
                                     max_num_batched_tokens=256, max_model_len=2048, num_kv_blocks=512,
                                     enforce_eager=eager), tp=TPGroup(0, 1, None, dev))
        if device == "cuda":
            assert isinstance(eng.runner.model.layers[0].wqkv, QuantWeight) and eng.runner.model.D == 256
            assert (eng.runner.use_graphs and bool(eng.runner.graphs)) != eager
        out[(device, eager)] = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
        eng.shutdown()
    rg, re_, rc = out[("cuda", False)], out[("cuda", True)], out[("cpu", True)]
    for a, b in zip(rg, re_):
        assert len(a[0]) == 6 and a[0][:2] == b[0][:2], (rg, re_)
    first = sum(a[0][0] == b[0][0] for a, b in zip(rg, rc))
    assert first >= len(PROMPTS) - 1, (rg, rc)
