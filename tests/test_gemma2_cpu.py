"""Gemma-2 (attention and final-logit soft-capping) on the CPU: greedy and log-prob parity
with ``transformers`` on a tiny checkpoint whose caps bite, the config mapping (Hub-style
dict, null caps, presets, the unchanged refusal of cap keys on a gemma3 config) and TP = 2.
Pattern and criterion of test_hf_parity.py::test_greedy_matches_transformers."""
import pytest
import torch

from hipserve.config import PRESETS, EngineConfig, ModelConfig
from hipserve.engine.llm_engine import LLMEngine
from hipserve.engine.request import SamplingParams
from hipserve.parallel.comm import TPGroup

PROMPTS = [[1, 5, 9, 33, 70, 100, 4, 250, 17, 64, 3], list(range(3, 40)), [7] * 11 + [9, 200, 31]]


def _hf_config(attn_cap=1.5, final_cap=2.0):
    transformers = pytest.importorskip("transformers")
    # 4 layers: both layer types twice; window 8 < every prompt
    return transformers.Gemma2Config(
        hidden_size=64, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, vocab_size=320,
        max_position_embeddings=512, rms_norm_eps=1e-6, tie_word_embeddings=True, intermediate_size=128,
        head_dim=32, query_pre_attn_scalar=24, sliding_window=8, attn_logit_softcapping=attn_cap,
        final_logit_softcapping=final_cap, attn_implementation="eager")


def _hf_model(attn_cap=1.5, final_cap=2.0):
    """The same weights for any caps (one seed): norm weights off their init, q_proj and the
    tied embedding scaled up so that scores and logits reach past the caps."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(7)
    m = transformers.AutoModelForCausalLM.from_config(_hf_config(attn_cap, final_cap), dtype=torch.float32).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
            elif name.endswith("q_proj.weight"):
                p.mul_(150.0)
            elif name.endswith("embed_tokens.weight"):
                p.mul_(6.0)
    return m


def _hf_logits(m, seq):
    with torch.no_grad():
        return m(torch.tensor([seq])).logits[0].float()


def _hf_greedy(m, prompt, n):
    seq = list(prompt)
    for _ in range(n):
        seq.append(int(_hf_logits(m, seq)[-1].argmax()))
    return seq[len(prompt):]


def _engine(path, **kw):
    return LLMEngine(EngineConfig(model=path, device="cpu", dtype="float32", max_num_seqs=4,
                                  max_num_batched_tokens=24, num_kv_blocks=128, max_model_len=256, **kw),
                     tp=TPGroup())


def _generate_with_logprobs(eng, prompts, sp):
    ids = [eng.add_request(None, p, sp).request_id for p in prompts]
    toks, lps = {i: [] for i in ids}, {i: [] for i in ids}
    while eng.has_unfinished():
        for o in eng.step():
            toks[o.request_id].extend(o.new_token_ids)
            lps[o.request_id].append(o.logprobs[0])  # the chosen token's log-probability
    return [(toks[i], lps[i]) for i in ids]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    m = _hf_model()
    path = str(tmp_path_factory.mktemp("gemma2") / "tiny")
    m.save_pretrained(path, safe_serialization=True)
    return m, path


def test_greedy_and_logprobs_match_transformers(ckpt):
    m, path = ckpt
    eng = _engine(path)
    mc = eng.runner.model.cfg
    assert mc.family == "gemma2" and mc.attn_softcap == 1.5 and mc.final_softcap == 2.0 and not mc.qk_norm
    assert mc.layer_windows == (8, 0, 8, 0)
    n = 8
    res = _generate_with_logprobs(eng, PROMPTS, SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True))
    # the caps bite: the same weights without them choose other tokens
    plain = _hf_model(None, None)
    moved = sum(_hf_greedy(plain, p, n) != toks for p, (toks, _) in zip(PROMPTS, res))
    assert moved >= 2, moved
    far = 0.0
    for p, (toks, lps) in zip(PROMPTS, res):
        assert len(toks) == n and len(lps) == n
        lg = _hf_logits(m, list(p) + list(toks))
        # the final cap is monotonic (no greedy token moves): its effect shows in the log-probs
        cap = m.config.final_logit_softcapping
        raw = torch.atanh((lg / cap).clamp(-1 + 1e-7, 1 - 1e-7)) * cap
        for i, t in enumerate(toks):
            row = lg[len(p) - 1 + i]
            assert row[t] >= row.max() - 1e-4, (i, t, int(row.argmax()), float(row.max() - row[t]))
            want = float(torch.log_softmax(row, -1)[t])
            # fp32 on both sides; 1e-4 of per-logit noise (the criterion above) over a 320-term log-softmax
            assert abs(lps[i] - want) <= 1e-3, (i, lps[i], want)
            far = max(far, abs(float(torch.log_softmax(raw[len(p) - 1 + i], -1)[t]) - want))
    assert far > 0.05, far


def test_hub_config_mapping():
    """Hub config.json (no layer_types): even layers slide, odd layers are global."""
    d = {"architectures": ["Gemma2ForCausalLM"], "model_type": "gemma2", "hidden_size": 3584,
         "num_hidden_layers": 42, "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 256,
         "intermediate_size": 14336, "vocab_size": 256000, "query_pre_attn_scalar": 224, "rope_theta": 10000.0,
         "sliding_window": 4096, "rms_norm_eps": 1e-6, "attn_logit_softcapping": 50.0,
         "final_logit_softcapping": 30.0, "hidden_activation": "gelu_pytorch_tanh", "max_position_embeddings": 8192,
         "eos_token_id": 1, "bos_token_id": 2}
    c = ModelConfig.from_hf_dict(d)
    assert c.family == "gemma2" and c.architecture == "llama"
    assert c.layer_windows[:4] == (4096, 0, 4096, 0) and len(c.layer_windows) == 42 and c.sliding_window == 4096
    assert c.attn_softcap == 50.0 and c.final_softcap == 30.0
    assert not c.qk_norm and c.rope_local_theta == 0.0 and c.rope_theta == 10000.0 and c.rope_scaling is None
    assert abs(c.attn_scale - 224 ** -0.5) < 1e-12 and abs(c.embed_scale - 3584 ** 0.5) < 1e-9
    assert c.hidden_act == "gelu_tanh" and c.sandwich_norm and c.norm_offset and c.tie_word_embeddings
    c0 = ModelConfig.from_hf_dict({**d, "attn_logit_softcapping": None, "final_logit_softcapping": None})
    assert c0.attn_softcap == 0.0 and c0.final_softcap == 0.0
    c1 = ModelConfig.from_hf_dict({**d, "layer_types": ["full_attention", "sliding_attention"] * 21})
    assert c1.layer_windows[:2] == (0, 4096)


def test_transformers_config_mapping():
    """What ``transformers`` writes (layer_types present) maps like the Hub form."""
    c = ModelConfig.from_hf_dict(_hf_config().to_dict())
    assert c.family == "gemma2" and c.layer_windows == (8, 0, 8, 0)
    assert c.attn_softcap == 1.5 and c.final_softcap == 2.0 and abs(c.attn_scale - 24 ** -0.5) < 1e-12


@pytest.mark.parametrize("name,hidden,layers,nq,nkv,D,inter,scalar",
                         [("gemma-2-2b", 2304, 26, 8, 4, 256, 9216, 256), ("gemma-2-9b", 3584, 42, 16, 8, 256, 14336, 256),
                          ("gemma-2-27b", 4608, 46, 32, 16, 128, 36864, 144)])
def test_presets(name, hidden, layers, nq, nkv, D, inter, scalar):
    c = PRESETS[name]
    assert (c.family, c.hidden_size, c.num_layers, c.num_heads, c.num_kv_heads, c.head_dim, c.intermediate_size) == \
        ("gemma2", hidden, layers, nq, nkv, D, inter)
    assert c.vocab_size == 256000 and c.max_position_embeddings == 8192 and c.rms_norm_eps == 1e-6
    assert c.attn_softcap == 50.0 and c.final_softcap == 30.0 and c.sliding_window == 4096
    assert c.layer_windows == tuple(0 if i % 2 else 4096 for i in range(layers))
    assert abs(c.attn_scale - scalar ** -0.5) < 1e-12 and c.tie_word_embeddings and not c.qk_norm
    assert c.hidden_act == "gelu_tanh" and c.sandwich_norm and c.norm_offset and c.rope_theta == 1e4
    assert hidden % 256 == 0 and inter % 256 == 0  # every projection has decode-GEMM candidates


def test_gemma3_with_cap_keys_still_refused():
    d = {"architectures": ["Gemma3ForCausalLM"], "model_type": "gemma3_text", "hidden_size": 64,
         "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 128, "vocab_size": 320,
         "attn_logit_softcapping": 50.0}
    with pytest.raises(NotImplementedError, match=r"logit soft-capping \(Gemma-2\) is not supported"):
        ModelConfig.from_hf_dict(d)


def test_tp2_matches_tp1(ckpt):
    """Vocabulary-parallel logits are capped after the all-gather; kv heads split 1 + 1."""
    from tests.test_tp_cpu import PROMPTS as TP_PROMPTS
    from tests.test_tp_cpu import _cfg, _run_tp

    _, path = ckpt
    ref = LLMEngine(_cfg(path, 1), tp=TPGroup())
    want = [r[0] for r in ref.generate(TP_PROMPTS, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))]
    assert _run_tp(path, 2) == want
