"""Gemma-2 end to end on the GPU: tiny HF checkpoints written by ``transformers`` on the CPU
(head_dim 256: the 2B / 9B head size; head_dim 128: the 27B's, whose global layers take the
fused qkv decode kernel), served by the bf16 GPU engine with soft-capped attention (prefill
v1 / v2, paged decode, sliding layers past their window, chunked prefill) and capped logits,
against the fp32 CPU reference engine loading the same files. Pattern and criteria of
test_gemma3_small_gpu.py. The caps are small and q_proj / the tied embedding scaled up so
that they bite: on the CPU the same weights without the caps choose another first token on
at least 3 of the 4 prompts."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from hipserve.config import PRESETS, EngineConfig, resolve_model_config  # noqa: E402
from hipserve.engine.llm_engine import LLMEngine  # noqa: E402
from hipserve.engine.request import SamplingParams  # noqa: E402
from hipserve.parallel.comm import TPGroup  # noqa: E402

pytestmark = pytest.mark.gpu

PROMPTS = [[1] + list(range(10, 300)), [1, 7, 8, 9], [1] + [42] * 40, list(range(3, 600))]


def _cfg(D):
    return transformers.Gemma2Config(
        hidden_size=256, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, vocab_size=1024,
        max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=True, intermediate_size=512,
        head_dim=D, query_pre_attn_scalar=D, sliding_window=64, attn_logit_softcapping=1.5,
        final_logit_softcapping=4.0, attn_implementation="eager")


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    out = {}
    for D in (256, 128):
        torch.manual_seed(11)
        m = transformers.AutoModelForCausalLM.from_config(_cfg(D), dtype=torch.float32)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(torch.randn_like(p) * 0.1)
                elif name.endswith("q_proj.weight"):
                    p.mul_(150.0)  # scores far past the attention cap
                elif name.endswith("embed_tokens.weight"):
                    p.mul_(2.0)    # logits up to the final cap
        path = tmp_path_factory.mktemp(f"gemma2-d{D}")
        m.save_pretrained(str(path), safe_serialization=True)
        out[D] = str(path)
    return out


def _engine(path, device, eager, kv="auto", model_cfg=None):
    dt = "bfloat16" if device == "cuda" else "float32"
    cfg = EngineConfig(model=path, device=device, dtype=dt, max_num_seqs=16, max_num_batched_tokens=256,
                       max_model_len=2048, num_kv_blocks=512, enforce_eager=eager, kv_cache_dtype=kv)
    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    return LLMEngine(cfg, tp=TPGroup(0, 1, None, dev), model_cfg=model_cfg)


def _generate(path, device, eager, kv="auto", D=None, model_cfg=None, n=6):
    eng = _engine(path, device, eager, kv, model_cfg)
    mc = eng.runner.model.cfg
    if model_cfg is None:
        assert mc.family == "gemma2" and mc.attn_softcap == 1.5 and mc.final_softcap == 4.0
        assert mc.layer_windows == (64, 0, 64, 0)
    if device == "cuda":
        assert eng.runner.model.D == D
        assert (eng.runner.use_graphs and bool(eng.runner.graphs)) != eager
        # head_dim 128: the global layers decode from the qkv partials (the capped fused kernel)
        model = eng.runner.model
        assert model.fused_qkv_attn_ok(1) == (D == 128 and kv == "auto" and model.fused_qkv_attention)
        assert not eng.runner.model.fused_qkv_attn_ok(0)
    res = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True))
    eng.shutdown()
    return res


@pytest.mark.parametrize("D", [256, 128])
def test_gemma2_gpu_matches_cpu(ckpts, D):
    rc = _generate(ckpts[D], "cpu", True, n=1)
    plain = resolve_model_config(ckpts[D]).replace(attn_softcap=0.0, final_softcap=0.0)
    rp = _generate(ckpts[D], "cpu", True, model_cfg=plain, n=1)
    assert sum(a[0][0] != b[0][0] for a, b in zip(rc, rp)) >= len(PROMPTS) - 1, (rc, rp)  # the caps bite
    rg, re_ = _generate(ckpts[D], "cuda", False, D=D), _generate(ckpts[D], "cuda", True, D=D)
    for a, b in zip(rg, re_):
        assert len(a[0]) == 6 and a[0][:2] == b[0][:2], (D, rg, re_)
    first = sum(a[0][0] == b[0][0] for a, b in zip(rg, rc))
    assert first >= len(PROMPTS) - 1, (D, rg, rc)


def test_gemma2_fp8_kv_graph_equals_eager(ckpts):
    rg, re_ = _generate(ckpts[256], "cuda", False, "fp8", D=256), _generate(ckpts[256], "cuda", True, "fp8", D=256)
    for a, b in zip(rg, re_):
        assert len(a[0]) == 6 and a[0][:2] == b[0][:2], (rg, re_)


def test_gemma2_preset_dummy_weights():
    """The gemma-2-2b preset at 2 layers on synthetic weights: builds, decodes, carries the caps."""
    mcfg = PRESETS["gemma-2-2b"].replace(name="gemma-2-2b-2l", num_layers=2, layer_windows=(4096, 0))
    cfg = EngineConfig(model="gemma-2-2b-2l", load_format="dummy", device="cuda", max_num_seqs=4,
                       max_num_batched_tokens=256, max_model_len=512, num_kv_blocks=64)
    eng = LLMEngine(cfg, tp=TPGroup(0, 1, None, torch.device("cuda", 0)), model_cfg=mcfg)
    assert eng.runner.model.cfg.attn_softcap == 50 and eng.runner.model.cfg.final_softcap == 30
    res = eng.generate([[2, 10, 11, 12], [2] + list(range(20, 60))],
                       SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True))
    eng.shutdown()
    for toks, _text, reason in res:
        assert len(toks) == 4 and reason == "length" and all(0 <= t < mcfg.vocab_size for t in toks)
