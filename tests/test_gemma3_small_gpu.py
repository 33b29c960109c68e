"""Gemma-3 at head_dim 256 (the 1B / 4B / 12B head size) end to end on the GPU: a tiny HF
checkpoint written by ``transformers`` on the CPU, served by the bf16 GPU engine (prefill
v1 and paged decode at 256, sliding-window layers past their window, chunked prefill),
against the fp32 CPU reference engine loading the same files. Pattern and criteria of
test_families_gpu.py; head layouts 4 / 2 (the 4B / 12B group of 2) and 4 / 1 (the 1B's 4)."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from hipserve.config import EngineConfig  # noqa: E402
from hipserve.engine.llm_engine import LLMEngine  # noqa: E402
from hipserve.engine.request import SamplingParams  # noqa: E402
from hipserve.parallel.comm import TPGroup  # noqa: E402

pytestmark = pytest.mark.gpu

PROMPTS = [[1] + list(range(10, 300)), [1, 7, 8, 9], [1] + [42] * 40, list(range(3, 600))]


def _cfg(nkv):
    return transformers.Gemma3TextConfig(
        hidden_size=256, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=nkv, vocab_size=1024,
        max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=True, intermediate_size=512,
        head_dim=256, query_pre_attn_scalar=256, sliding_window=64,
        rope_parameters={"sliding_attention": {"rope_type": "default", "rope_theta": 1e4},
                         "full_attention": {"rope_type": "linear", "factor": 2.0, "rope_theta": 1e6}},
        layer_types=["sliding_attention", "sliding_attention", "full_attention"])


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    out = {}
    for nkv in (2, 1):
        torch.manual_seed(7)
        m = transformers.AutoModelForCausalLM.from_config(_cfg(nkv), torch_dtype=torch.float32)
        with torch.no_grad():
            for _name, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(torch.randn_like(p) * 0.1)
        path = tmp_path_factory.mktemp(f"gemma3-d256-kv{nkv}")
        m.save_pretrained(str(path), safe_serialization=True)
        out[nkv] = str(path)
    return out


def _engine(path, device, eager, kv="auto"):
    dt = "bfloat16" if device == "cuda" else "float32"
    cfg = EngineConfig(model=path, device=device, dtype=dt, max_num_seqs=16, max_num_batched_tokens=256,
                       max_model_len=2048, num_kv_blocks=512, enforce_eager=eager, kv_cache_dtype=kv)
    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    return LLMEngine(cfg, tp=TPGroup(0, 1, None, dev))


def _generate(path, device, eager, kv="auto"):
    eng = _engine(path, device, eager, kv)
    if device == "cuda":
        assert eng.runner.model.D == 256
        assert (eng.runner.use_graphs and bool(eng.runner.graphs)) != eager
    res = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    eng.shutdown()
    return res


@pytest.mark.parametrize("nkv", [2, 1])
def test_gemma3_d256_gpu_matches_cpu(ckpts, nkv):
    rg, re_ = _generate(ckpts[nkv], "cuda", False), _generate(ckpts[nkv], "cuda", True)
    rc = _generate(ckpts[nkv], "cpu", True)
    for a, b in zip(rg, re_):
        assert len(a[0]) == 6 and a[0][:2] == b[0][:2], (nkv, rg, re_)
    first = sum(a[0][0] == b[0][0] for a, b in zip(rg, rc))
    assert first >= len(PROMPTS) - 1, (nkv, rg, rc)


def test_gemma3_d256_fp8_kv_graph_equals_eager(ckpts):
    rg, re_ = _generate(ckpts[2], "cuda", False, "fp8"), _generate(ckpts[2], "cuda", True, "fp8")
    for a, b in zip(rg, re_):
        assert len(a[0]) == 6 and a[0][:2] == b[0][:2], (rg, re_)
