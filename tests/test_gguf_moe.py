"""Mixture-of-experts GGUF files on the GGUF tier (CPU side): the synthetic writer and
the loader for ``qwen3moe`` and llama-arch (Mixtral) files with stacked ``*_exps``
tensors, greedy parity with transformers on an F32 file, a Q4_K_M-mix file against the
numpy block decoders, the synthetic quantised MoE weights, and the refusals."""
import numpy as np
import pytest
import torch

from hipserve.config import PRESETS, EngineConfig
from hipserve.engine.llm_engine import LLMEngine
from hipserve.engine.request import SamplingParams
from hipserve.parallel.comm import TPGroup
from hipserve.weights import gguf as G

# 4 experts top-2 of width 256 (one K-quant super-block), 2 layers
TINY = PRESETS["tiny-mixtral"].replace(name="tiny-moe", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64,
                                       intermediate_size=512, moe_intermediate_size=256, num_experts=4,
                                       num_experts_per_tok=2)


def _cpu_model(cfg, dtype=torch.float32):
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import get_ops

    dev = torch.device("cpu")
    return LlamaModel(cfg, TPGroup(0, 1, None, dev), dev, dtype, get_ops(dev))


def _engine(path, **kw):
    return LLMEngine(EngineConfig(model=path, device="cpu", dtype="float32", load_format="gguf", max_num_seqs=4,
                                  max_num_batched_tokens=24, num_kv_blocks=128, max_model_len=256, **kw),
                     tp=TPGroup())


@pytest.mark.parametrize("arch", ["qwen3moe", "llama"])
def test_writer_round_trip(tmp_path, arch):
    cfg = TINY.replace(qk_norm=arch == "qwen3moe")
    p = G.write_synthetic_moe_gguf(str(tmp_path / f"{arch}.gguf"), cfg, arch, qtype=G.Q8_0)
    gf = G.GGUFFile(p)
    mc = gf.model_config()
    E, I, H = 4, 256, 256
    assert mc.architecture == "mixtral"
    assert mc.family == ("qwen3_moe" if arch == "qwen3moe" else "mixtral")
    assert (mc.num_experts, mc.num_experts_per_tok, mc.expert_size, mc.norm_topk_prob) == (E, 2, I, True)
    assert mc.moe_intermediate_size == (I if arch == "qwen3moe" else 0)
    assert mc.qk_norm == (arch == "qwen3moe") and mc.rope_mode == (0 if arch == "qwen3moe" else 1)
    for i in range(cfg.num_layers):
        b = f"blk.{i}."
        assert gf.tensors[b + "ffn_gate_inp.weight"].shape == (H, E)
        for n, shape in (("gate", (H, I, E)), ("up", (H, I, E)), ("down", (I, H, E))):  # ggml ne = [K, N, E]
            t = gf.tensors[b + f"ffn_{n}_exps.weight"]
            assert t.shape == shape and t.type == G.Q8_0
            assert t.nbytes == E * I * H // 32 * 34
    m = _cpu_model(mc)
    G.load_gguf_weights(m, p)
    for lw in m.layers:
        assert lw.router.shape == (E, H) and lw.w13.shape == (E, 2 * I, H) and lw.w2.shape == (E, H, I)
        assert lw.wgu is None and lw.wd is None
        assert (lw.q_norm is not None) == (arch == "qwen3moe")


def test_write_gguf_round_trips_3d_quantised(tmp_path):
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((3, 32, 256)) * 0.05).astype(np.float32)
    p = str(tmp_path / "t.gguf")
    for qt in (G.Q4_K, G.Q6_K, G.Q8_0, G.F32):
        G.write_gguf(p, {"general.architecture": "llama"}, [("pad.weight", w[0, 0], G.F32), ("w_exps.weight", w, qt)])
        gf = G.GGUFFile(p)
        t = gf.tensors["w_exps.weight"]
        assert t.shape == (256, 32, 3) and t.rows_cols == (96, 256)
        # expert-major, each expert's rows quantised on their own: expert e == quantising w[e] alone
        raw = np.asarray(gf.raw("w_exps.weight")).reshape(3, -1)
        for e in range(3):
            assert np.array_equal(raw[e], G.quantize(w[e], qt))
        assert np.array_equal(gf.tensor_f32("w_exps.weight").reshape(3, 32, 256)[1],
                              G.dequantize(G.quantize(w[1], qt), qt, 32 * 256).reshape(32, 256))


def _hf_qwen3moe_to_gguf(m, path):
    """The HF Qwen3-MoE model as an F32 ``qwen3moe`` GGUF with stacked ``*_exps`` tensors
    (llama.cpp's converter layout); takes the fused (experts.gate_up_proj [E, 2I, H] /
    experts.down_proj [E, H, I]) and the per-expert HF state-dict layouts."""
    c = m.config
    sd = {k: v.detach().float().numpy() for k, v in m.state_dict().items()}
    H, V, L, D = c.hidden_size, c.vocab_size, c.num_hidden_layers, c.head_dim
    E, I = c.num_experts, c.moe_intermediate_size
    a = "qwen3moe"
    toks = ["<unk>", "<s>", "</s>"] + [f"<0x{b:02X}>" for b in range(256)] + [f"▁w{i}" for i in range(V - 259)]
    theta = c.rope_parameters["rope_theta"] if getattr(c, "rope_parameters", None) else c.rope_theta
    md = {"general.architecture": a, "general.name": "tiny-qwen3moe", f"{a}.context_length": 512,
          f"{a}.embedding_length": H, f"{a}.block_count": L, f"{a}.feed_forward_length": c.intermediate_size,
          f"{a}.expert_feed_forward_length": I, f"{a}.expert_count": E, f"{a}.expert_used_count": c.num_experts_per_tok,
          f"{a}.attention.head_count": c.num_attention_heads, f"{a}.attention.head_count_kv": c.num_key_value_heads,
          f"{a}.attention.key_length": D, f"{a}.rope.freq_base": float(theta), f"{a}.rope.dimension_count": D,
          f"{a}.attention.layer_norm_rms_epsilon": float(c.rms_norm_eps),
          "tokenizer.ggml.model": "llama", "tokenizer.ggml.tokens": toks,
          "tokenizer.ggml.scores": [float(-i) for i in range(len(toks))],
          "tokenizer.ggml.token_type": [3 if i < 3 else (6 if i < 259 else 1) for i in range(len(toks))],
          "tokenizer.ggml.bos_token_id": 1, "tokenizer.ggml.eos_token_id": 2}
    t = [("token_embd.weight", sd["model.embed_tokens.weight"], G.F32),
         ("output_norm.weight", sd["model.norm.weight"], G.F32), ("output.weight", sd["lm_head.weight"], G.F32)]
    for i in range(L):
        p, b = f"model.layers.{i}.", f"blk.{i}."
        t += [(b + "attn_norm.weight", sd[p + "input_layernorm.weight"], G.F32),
              (b + "ffn_norm.weight", sd[p + "post_attention_layernorm.weight"], G.F32),
              (b + "attn_output.weight", sd[p + "self_attn.o_proj.weight"], G.F32),
              (b + "attn_q_norm.weight", sd[p + "self_attn.q_norm.weight"], G.F32),
              (b + "attn_k_norm.weight", sd[p + "self_attn.k_norm.weight"], G.F32),
              (b + "ffn_gate_inp.weight", sd[p + "mlp.gate.weight"], G.F32)]
        t += [(b + f"attn_{x}.weight", sd[p + f"self_attn.{x}_proj.weight"], G.F32) for x in "qkv"]
        if p + "mlp.experts.gate_up_proj" in sd:  # fused
            gu, down = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.down_proj"]
            assert gu.shape == (E, 2 * I, H) and down.shape == (E, H, I), (gu.shape, down.shape)
            gate, up = gu[:, :I], gu[:, I:]
        else:  # per expert
            gate, up, down = (np.stack([sd[p + f"mlp.experts.{e}.{n}_proj.weight"] for e in range(E)])
                              for n in ("gate", "up", "down"))
        t += [(b + "ffn_gate_exps.weight", gate, G.F32), (b + "ffn_up_exps.weight", up, G.F32),
              (b + "ffn_down_exps.weight", down, G.F32)]
    G.write_gguf(path, md, [(n, np.ascontiguousarray(x), q) for n, x, q in t])
    return path


def test_qwen3moe_gguf_matches_transformers(tmp_path):
    """An F32 ``qwen3moe`` GGUF of a tiny HF Qwen3-MoE (8 experts, top-3, width 48)
    greedy-decodes like transformers: every chosen token's HF logit within 1e-3 of the
    row maximum (the bound of test_hf_parity.py::test_gguf_family_matches_transformers)."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Qwen3MoeConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                                      num_key_value_heads=2, vocab_size=320, max_position_embeddings=512,
                                      rms_norm_eps=1e-6, tie_word_embeddings=False, intermediate_size=128,
                                      moe_intermediate_size=48, num_experts=8, num_experts_per_tok=3,
                                      norm_topk_prob=True, head_dim=16, rope_theta=1e6)
    torch.manual_seed(1234)
    m = transformers.AutoModelForCausalLM.from_config(cfg, torch_dtype=torch.float32).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:  # non-trivial norm weights
                p.add_(torch.randn_like(p) * 0.1)
            elif name.endswith("gate.weight") and p.shape[0] <= 8:
                p.mul_(20.0)  # decisive routing: no near-ties between experts
    path = _hf_qwen3moe_to_gguf(m, str(tmp_path / "qwen3moe.gguf"))
    eng = _engine(path)
    mc = eng.runner.model.cfg
    assert mc.family == "qwen3_moe" and mc.rope_mode == 0 and mc.qk_norm and mc.norm_topk_prob
    assert (mc.num_experts, mc.num_experts_per_tok, mc.expert_size) == (8, 3, 48)
    prompts = [[1, 5, 9, 33, 70, 100], list(range(3, 40))]
    res = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    for pr, (toks, _, _) in zip(prompts, res):
        with torch.no_grad():
            lg = m(torch.tensor([list(pr) + list(toks)])).logits[0].float()
        for i, t in enumerate(toks):
            row = lg[len(pr) - 1 + i]
            assert row[t] >= row.max() - 1e-3, (i, t, int(row.argmax()), float(row.max() - row[t]))


def test_quantised_moe_file_on_cpu(tmp_path):
    """Q4_K_M-mix file on CPU: the experts are dense tensors equal to the numpy block
    decoders' output (cast to the model dtype), and the engine generates from it."""
    cfg = TINY.replace(qk_norm=True)
    p = G.write_synthetic_moe_gguf(str(tmp_path / "q4km.gguf"), cfg, "qwen3moe", mixed_k=True)
    gf = G.GGUFFile(p)
    E, I, H = 4, 256, 256
    for dt in (torch.float32, torch.bfloat16):
        m = _cpu_model(gf.model_config(), dt)
        G.load_gguf_weights(m, p)
        for i, lw in enumerate(m.layers):
            b = f"blk.{i}."
            assert gf.tensors[b + "ffn_gate_exps.weight"].type == G.Q4_K
            assert gf.tensors[b + "ffn_down_exps.weight"].type == G.Q6_K

            def deq(n, N, K):
                t = gf.tensors[b + n]
                return torch.from_numpy(G.dequantize(gf.raw(b + n), t.type, t.n_elements).reshape(E, N, K)).to(dt)
            assert isinstance(lw.w13, torch.Tensor) and lw.w13.dtype == dt
            assert torch.equal(lw.w13[:, :I], deq("ffn_gate_exps.weight", I, H))
            assert torch.equal(lw.w13[:, I:], deq("ffn_up_exps.weight", I, H))
            assert torch.equal(lw.w2, deq("ffn_down_exps.weight", H, I))
            assert lw.router.dtype == dt and lw.router.shape == (E, H)
    eng = _engine(p)
    res = eng.generate([[1, 5, 9, 33], list(range(3, 30))], SamplingParams(temperature=0.0, max_tokens=5, ignore_eos=True))
    for toks, _, reason in res:
        assert len(toks) == 5 and reason == "length" and all(0 <= t < cfg.vocab_size for t in toks)


@pytest.mark.parametrize("scheme", ["q4_k_m", "q8_0", "q4_0"])
def test_allocate_random_quant_moe_cpu(scheme):
    from hipserve.models.llama import LlamaModel

    types = LlamaModel.QUANT_SCHEMES[scheme]
    assert (types["gate_exps"], types["up_exps"], types["down_exps"]) == {
        "q4_k_m": (G.Q4_K, G.Q4_K, G.Q6_K), "q8_0": (G.Q8_0,) * 3, "q4_0": (G.Q4_0,) * 3}[scheme]
    cfg = TINY.replace(num_layers=3, qk_norm=True)
    m = _cpu_model(cfg)
    m.allocate_random_quant(scheme)
    E, I, H = 4, 256, 256
    assert len(m.layers) == 3
    for lw in m.layers:
        assert lw.router.shape == (E, H) and lw.w13.shape == (E, 2 * I, H) and lw.w2.shape == (E, H, I)
        assert isinstance(lw.w13, torch.Tensor) and isinstance(lw.w2, torch.Tensor)
        assert lw.wgu is None and lw.wd is None and lw.q_norm is not None
        assert torch.isfinite(lw.w13).all() and 0 < lw.w13.abs().max() < 1.0
    # every layer owns its weights (later layers are copies, not aliases, of a generated stack)
    assert len({lw.w13.data_ptr() for lw in m.layers}) == 3
    # the reference loop serves them
    x = torch.randn(5, H) * 0.5
    y = m.moe(x, m.layers[0])
    assert y.shape == (5, H) and torch.isfinite(y).all() and y.abs().max() > 0


def _rewrite(src, dst, rename=None, extra_md=None):
    """Copy a GGUF file tensor by tensor (raw blocks kept), renaming tensors / adding metadata."""
    gf = G.GGUFFile(src)
    md = {k: (list(v) if isinstance(v, np.ndarray) else v) for k, v in gf.metadata.items() if k != "general.alignment"}
    md.update(extra_md or {})
    tensors = []
    for n, t in gf.tensors.items():
        arr = gf.tensor_f32(n).reshape(tuple(reversed(t.shape)))
        for new in (rename or {}).get(n, [n]):
            tensors.append((new, arr, G.F32 if t.type in (G.F32, G.F16) else G.Q8_0))
    G.write_gguf(dst, md, tensors)
    return dst


def test_refusals_name_the_key(tmp_path):
    cfg = TINY.replace(qk_norm=True)
    src = G.write_synthetic_moe_gguf(str(tmp_path / "ok.gguf"), cfg, "qwen3moe", qtype=G.Q8_0)

    def load(path):
        gf = G.GGUFFile(path)
        m = _cpu_model(gf.model_config())
        G.load_gguf_weights(m, path)

    load(src)
    # shared experts: the metadata count ...
    p = _rewrite(src, str(tmp_path / "shared_md.gguf"), extra_md={"qwen3moe.expert_shared_count": 1})
    with pytest.raises(NotImplementedError, match="expert_shared_count"):
        load(p)
    # ... and the *_shexp tensors
    p = _rewrite(src, str(tmp_path / "shexp.gguf"),
                 rename={"blk.0.ffn_norm.weight": ["blk.0.ffn_norm.weight", "blk.0.ffn_gate_shexp.weight"]})
    with pytest.raises(NotImplementedError, match=r"blk\.0\.ffn_gate_shexp\.weight"):
        load(p)
    # the legacy per-expert names
    p = _rewrite(src, str(tmp_path / "legacy.gguf"),
                 rename={"blk.0.ffn_gate_exps.weight": [f"blk.0.ffn_gate.{e}.weight" for e in range(4)]})
    with pytest.raises(NotImplementedError, match=r"blk\.0\.ffn_gate\.0\.weight"):
        load(p)
    # a missing expert stack is named too, never a bare KeyError
    p = _rewrite(src, str(tmp_path / "missing.gguf"), rename={"blk.1.ffn_down_exps.weight": []})
    with pytest.raises(NotImplementedError, match=r"blk\.1\.ffn_down_exps\.weight"):
        load(p)
    p = _rewrite(src, str(tmp_path / "norouter.gguf"), rename={"blk.1.ffn_gate_inp.weight": []})
    with pytest.raises(NotImplementedError, match=r"blk\.1\.ffn_gate_inp\.weight"):
        load(p)


def test_gguf_archs_and_quant_moe_supported():
    from hipserve.ops import quant as Q

    assert "qwen3moe" in G.GGUF_ARCHS
    for qt in (G.Q4_0, G.Q4_1, G.Q8_0, G.Q4_K, G.Q5_K, G.Q6_K):
        kqt = Q.KERNEL_QT[qt]
        assert Q.QuantMoE.supported(kqt, 512, 256) and kqt in Q.QuantMoE.KERNEL_QTS
        assert not Q.QuantMoE.supported(kqt, 520, 256) and not Q.QuantMoE.supported(kqt, 512, 384)
        rng = np.random.default_rng(qt)
        raw = Q.random_blocks(rng, qt, 32, 256)
        assert Q.QuantMoE.supported(kqt, 32, 256, raw)
        be, bb = G.BLOCK[qt]
        big = raw.copy().reshape(-1, bb)
        off = 208 if qt == G.Q6_K else 0
        big[0, off:off + 2] = np.frombuffer(np.float16(4.0).tobytes(), np.uint8)  # a block scale beyond the range
        if qt in (G.Q4_K, G.Q5_K):
            big[0, 4:16] = 63
        if qt == G.Q6_K:
            big[0, 192:208] = 127
        assert not Q.QuantMoE.supported(kqt, 32, 256, big.reshape(-1))
    assert not Q.QuantMoE.supported(7, 512, 256)  # FP8B has no expert kernel


def test_q5_0_quantiser_round_trip():
    x = (np.random.default_rng(5).standard_normal((8, 256)) * 0.05).astype(np.float32)
    raw = G.quantize(x, G.Q5_0)
    assert raw.size == x.size // 32 * 22
    d = G.dequantize(raw, G.Q5_0, x.size).reshape(8, 8, 32)
    step = np.abs(x.reshape(8, 8, 32)).max(-1, keepdims=True) / 16
    assert (np.abs(d - x.reshape(8, 8, 32)) <= 1.01 * step + 1e-6).all()  # one step at the clipped end, else half
    assert np.array_equal(G.quantize(d.reshape(8, 256), G.Q5_0), raw)     # a fixed point of the block codec


def test_per_layer_expert_formats_load_on_cpu(tmp_path):
    """``expert_types`` writes single layers in other expert formats (Q5_0 down; gate and up
    in different formats); on CPU every layer is dense and equals the block decoders."""
    cfg = TINY.replace(qk_norm=True)
    types = {0: (G.Q4_K, G.Q4_K, G.Q5_0), 1: (G.Q4_K, G.Q5_K, G.Q6_K)}
    p = G.write_synthetic_moe_gguf(str(tmp_path / "mixed.gguf"), cfg, "qwen3moe", mixed_k=True, expert_types=types)
    gf = G.GGUFFile(p)
    m = _cpu_model(gf.model_config())
    G.load_gguf_weights(m, p)
    E, I, H = 4, 256, 256
    for i, lw in enumerate(m.layers):
        b = f"blk.{i}."
        got = [gf.tensors[b + f"ffn_{n}_exps.weight"].type for n in ("gate", "up", "down")]
        assert tuple(got) == types[i]
        t = gf.tensors[b + "ffn_down_exps.weight"]
        want = G.dequantize(gf.raw(b + "ffn_down_exps.weight"), t.type, t.n_elements).reshape(E, H, I)
        assert torch.equal(lw.w2, torch.from_numpy(want)) and lw.w13.shape == (E, 2 * I, H)
    eng = _engine(p)
    res = eng.generate([[1, 5, 9, 33]], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    assert len(res[0][0]) == 3
