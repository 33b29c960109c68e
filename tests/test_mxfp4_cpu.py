"""MXFP4 off the GPU: the codec, the Quark-style loader on a checkpoint written here, the CPU
engine on the dequantised weights, and the CLI value."""
import json

import pytest
import torch

from hipserve.ops import quant as Q

PROMPTS = [[1, 5, 9, 33, 70, 100, 4, 250, 17, 64, 3], list(range(3, 40)), [7] * 11 + [9, 200, 31]]
H, I, V, L = 256, 512, 320, 2
PROJ = {"self_attn.q_proj": (256, H), "self_attn.k_proj": (128, H), "self_attn.v_proj": (128, H),
        "self_attn.o_proj": (H, 256), "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}


def test_codec_round_trip():
    """Every code under several scale bytes decodes to its exact value; quantising the
    decoded values returns the bytes (each 32-block holds a 4 or 6, so its exponent is kept)."""
    scales = torch.tensor([[0, 1, 100, 126, 127, 128, 200, 252]], dtype=torch.uint8)
    codes = torch.arange(16).repeat(2 * scales.shape[1])  # each block: the 16 codes twice
    nib = (codes[0::2] | (codes[1::2] << 4)).to(torch.uint8).reshape(1, -1)
    w = Q.mxfp4_dequantize(nib, scales)
    mag = torch.tensor(Q.E2M1, dtype=torch.float64)
    want = torch.cat([mag, -mag])[codes].reshape(-1, 32) * (2.0 ** (scales.double().reshape(-1, 1) - 127))
    assert torch.equal(w.double().reshape(-1, 32), want)
    q2, s2 = Q.mxfp4_quantize(w)
    assert torch.equal(q2, nib) and torch.equal(s2, scales)
    # nearest, ties to the even mantissa, saturation at 6; the block's 6.0 keeps the scale at 1
    x = torch.zeros(1, 32)
    x[0, :10] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.1, 0.7])
    got = Q.mxfp4_dequantize(*Q.mxfp4_quantize(x))[0, :10]
    assert got.tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -6.0, 0.5]


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """(Quark-style MXFP4 checkpoint, the same model as dequantised bf16, its tensors)."""
    from safetensors.torch import save_file

    g = torch.Generator().manual_seed(3)
    t = {"model.embed_tokens.weight": torch.randn(V, H, generator=g) * 0.5, "model.norm.weight": torch.ones(H),
         "lm_head.weight": torch.randn(V, H, generator=g) * 0.2}
    quant = {}
    for i in range(L):
        p = f"model.layers.{i}."
        t[p + "input_layernorm.weight"] = t[p + "post_attention_layernorm.weight"] = torch.ones(H)
        for name, (n, k) in PROJ.items():
            quant[p + name] = Q.mxfp4_quantize(torch.randn(n, k, generator=g) * 0.08)
    t = {k: v.to(torch.bfloat16) for k, v in t.items()}
    cfg = {"model_type": "llama", "architectures": ["LlamaForCausalLM"], "hidden_size": H, "intermediate_size": I,
           "num_hidden_layers": L, "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 64,
           "vocab_size": V, "max_position_embeddings": 512, "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
           "tie_word_embeddings": False, "torch_dtype": "bfloat16"}
    qcfg = {"quant_method": "quark", "exclude": ["lm_head"], "global_quant_config": {
        "weight": {"dtype": "fp4", "group_size": 32, "scale_format": "e8m0", "qscheme": "per_group"}}}
    root = tmp_path_factory.mktemp("mxfp4")
    out = []
    for name, tensors, c in (
            ("quark", {**t, **{k + ".weight": nib for k, (nib, _) in quant.items()},
                       **{k + ".weight_scale": sc for k, (_, sc) in quant.items()}}, {**cfg, "quantization_config": qcfg}),
            ("bf16", {**t, **{k + ".weight": Q.mxfp4_dequantize(*v).to(torch.bfloat16) for k, v in quant.items()}}, cfg)):
        d = root / name
        d.mkdir()
        save_file({k: v.clone().contiguous() for k, v in tensors.items()}, str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(c))
        out.append(str(d))
    return out[0], out[1], quant


def test_loader_reads_quark_checkpoint(ckpts):
    from hipserve.config import checkpoint_quantization
    from hipserve.weights.safetensors_loader import _Ckpt

    path, _, quant = ckpts
    assert checkpoint_quantization(path) == "mxfp4"
    ck = _Ckpt(path)
    assert not ck.is_mxfp4("lm_head.weight") and ck.full("lm_head.weight").dtype == torch.bfloat16
    for name, (nib, sc) in quant.items():
        assert ck.is_mxfp4(name + ".weight")
        rows, cols = ck.mxfp4_part(name + ".weight", 0, 16, 48), ck.mxfp4_part(name + ".weight", 1, 64, 128)
        assert torch.equal(rows[0], nib[16:48]) and torch.equal(rows[1], sc[16:48])
        assert torch.equal(cols[0], nib[:, 32:64]) and torch.equal(cols[1], sc[:, 2:4])
        assert ck.mxfp4_part(name + ".weight", 1, 16, 128) is None  # would split a 32-block
        part = Q.QuantPart.from_mxfp4(nib, sc, "cpu")
        assert part.qtype == Q.MXFP4 and part.q.shape == (nib.shape[0] // 16, nib.shape[1] // 128, 2176)
        assert part.nbytes * 8 == 4.25 * part.N * part.K
        assert torch.equal(ck.full(name + ".weight").float(), Q.mxfp4_dequantize(nib, sc))
    # lane 16 g + c of tile h: the row's 16 checkpoint bytes of block 4 h + g, its scale at byte h
    nib, sc = quant["model.layers.0.mlp.down_proj"]
    q = Q.QuantPart.from_mxfp4(nib, sc, "cpu").q
    r, sb, h, g, c = 3, 1, 1, 2, 5
    blk = 8 * sb + 4 * h + g
    assert torch.equal(q[r, sb, h * 1024 + (16 * g + c) * 16:][:16], nib[16 * r + c, 16 * blk:16 * blk + 16])
    assert q[r, sb, 2048 + (16 * g + c) * 2 + h] == sc[16 * r + c, blk]
    for bad in (torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(16, 64, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            Q.QuantPart.from_mxfp4(bad, torch.zeros(bad.shape[0], bad.shape[1] // 16, dtype=torch.uint8), "cpu")


def test_cpu_engine_matches_dequantised_weights(ckpts):
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    def run(path):
        eng = LLMEngine(EngineConfig(model=path, device="cpu", dtype="float32", max_num_seqs=4, max_num_batched_tokens=24,
                                     num_kv_blocks=128, max_model_len=256), tp=TPGroup())
        out = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
        return eng, [r[0] for r in out]

    eng, got = run(ckpts[0])
    nib, sc = ckpts[2]["model.layers.1.mlp.down_proj"]
    assert torch.equal(eng.runner.model.layers[1].wd.float(), Q.mxfp4_dequantize(nib, sc))
    assert got == run(ckpts[1])[1] and all(len(t) == 8 for t in got)


def test_cli_budget_and_tp_refusal():
    from hipserve.config import default_batched_tokens
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup
    from hipserve.server.cli import build_parser, config_from_args

    a = build_parser().parse_args(["--model", "llama-3-8b", "--device", "cpu", "--load-format", "dummy",
                                   "--quantization", "mxfp4"])
    cfg = config_from_args(a)
    assert cfg.extra == {"quantization": "mxfp4"}
    assert cfg.max_num_batched_tokens == default_batched_tokens("llama-3-8b", quantization="int8")
    with pytest.raises(ValueError, match="one device"):
        LLMEngine(cfg, tp=TPGroup(0, 2, None, torch.device("cpu")))
