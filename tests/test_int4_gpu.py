"""4-bit group-quantised weights kept 4-bit on the GPU (kernel format INT4, gguf_tiles.h):
``QuantPart.from_int4`` through the decode GEMM, its split-K partials, the tiled -> bf16
dequantiser and the expert GEMM against fp32 oracles of (u - z) * f16(scale); AutoAWQ gemm /
compressed-tensors 4-bit checkpoints loaded natively against the same checkpoints
dequantised to bf16 at load; and a synthetic ``--quantization int4`` engine, hipGraph
decode against eager decode."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, K = 272, 1024  # 17 row groups: a ragged last 128-row workgroup


@pytest.fixture(autouse=True, scope="module")
def _lib():
    from hipserve.ops import load_library

    load_library()


def _oracle(u, scale, zero, G):
    """fp32 (u - z) * f16(scale) [N, K]; ``zero`` None = 8."""
    z = zero.float().repeat_interleave(G, 1) if zero is not None else 8.0
    return (u.float() - z) * scale.half().float().repeat_interleave(G, 1)


@functools.lru_cache(maxsize=None)
def _case(group, asym, wide=False):
    """(QuantWeight, fp32 oracle on the device) of one [N, K] matrix, built once per
    (group, zero point kind) and shared by the M sweep. ``wide``: group scales log-uniform
    over 2^-16 .. 2^-1, with one group at 0.5 and one at 2^-16."""
    from hipserve.ops import quant as Q

    g = torch.Generator().manual_seed(1000 * group + 10 * asym + wide)
    G = group or K
    u = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    if wide:
        scale = torch.exp2(-1.0 - 15.0 * torch.rand(N, K // G, generator=g))
        scale[3, 1], scale[200, 7] = 0.5, 2.0 ** -16
    else:
        scale = torch.rand(N, K // G, generator=g) * 4e-3 + 1e-3
    zero = torch.randint(0, 16, (N, K // G), generator=g) if asym else None
    qw = Q.QuantWeight([Q.QuantPart.from_int4(u, scale, zero, DEV)])
    return qw, _oracle(u, scale, zero, G).to(DEV)


def _check(qw, wref, M, seed):
    from hipserve.ops import quant as Q

    assert qw.parts[0].kqt == Q.KERNEL_QT[Q.INT4] and qw.v2
    torch.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    want = x.float() @ wref.T
    err = (Q.quant_linear(x, qw).float() - want).abs().max().item()
    tol = 1e-2 * want.abs().max().item() + 1e-4
    print(f"int4 linear M={M}: err {err:.3e} tol {tol:.3e}")
    assert err < tol
    assert torch.allclose(Q.dequantize(qw).float(), wref.to(torch.bfloat16).float(), rtol=1e-2, atol=1e-6)


@pytest.mark.parametrize("group", [32, 128, 0])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("M", [1, 24, 64])
def test_int4_linear_matches_fp32(group, asym, M):
    """from_int4 -> quant_linear vs an fp32 matmul of (u - z) * f16(s); group 0 = per
    channel, zero None = 8 (the symmetric compressed-tensors case)."""
    qw, wref = _case(group, asym)
    _check(qw, wref, M, M + group)


@pytest.mark.parametrize("M", [1, 24, 64])
def test_int4_scale_range(M):
    """Group scales from 2^-16 (an f16 subnormal) to 0.5: the dequant has no scale-range
    limit (the magic-number form (1024 + u + off) * s rounds once in f16)."""
    qw, wref = _case(32, True, True)
    _check(qw, wref, M, M)


def test_int4_group_errors():
    from hipserve.ops import quant as Q

    u = torch.zeros(16, 256, dtype=torch.uint8)
    with pytest.raises(ValueError):
        Q.QuantPart.from_int4(u, torch.ones(16, 16), None, DEV)  # group 16
    with pytest.raises(ValueError):
        Q.QuantPart.from_int4(u[:, :128], torch.ones(16, 1), None, DEV)  # K % 256


def _parts(rows, Kp, G, seed):
    from hipserve.ops import quant as Q

    g = torch.Generator().manual_seed(seed)
    parts, refs = [], []
    for n in rows:
        u = torch.randint(0, 16, (n, Kp), generator=g, dtype=torch.uint8)
        scale = torch.rand(n, Kp // G, generator=g) * 4e-3 + 1e-3
        zero = torch.randint(0, 16, (n, Kp // G), generator=g)
        parts.append(Q.QuantPart.from_int4(u, scale, zero, DEV))
        refs.append(_oracle(u, scale, zero, G).to(DEV))
    return parts, refs


def test_int4_merged_projection_columns():
    """q | k | v as three INT4 parts of one launch: each part's output in its own columns."""
    from hipserve.ops import quant as Q

    rows = [256, 48, 48]
    parts, refs = _parts(rows, 512, 128, 3)
    qw = Q.QuantWeight(parts)
    torch.manual_seed(3)
    x = torch.randn(5, 512, device=DEV, dtype=torch.bfloat16)
    got = Q.quant_linear(x, qw).float()
    assert got.shape == (5, sum(rows))
    off = 0
    for n, ref in zip(rows, refs):
        want = x.float() @ ref.T
        assert (got[:, off:off + n] - want).abs().max().item() < 1e-2 * want.abs().max().item() + 1e-4
        off += n


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("M", [1, 24, 64])
def test_int4_split_k_partials(S, M, monkeypatch):
    """The fp32 split-K partials the fused decode epilogues consume, summed, equal
    quant_linear within the decode bound."""
    from hipserve.ops import quant as Q

    qw, wref = _case(128, True)
    monkeypatch.setitem(Q.SPLIT_TABLE, (Q._sig(qw), Q._bucket(M)), S)
    torch.manual_seed(S + M)
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    ws, s = Q.quant_partial(x, qw)
    assert s == S
    got = ws.view(S, M, N).sum(0)
    want = x.float() @ wref.T
    tol = 1e-2 * want.abs().max().item() + 1e-4
    assert (got - want).abs().max().item() < tol
    assert (got - Q.quant_linear(x, qw).float()).abs().max().item() < tol


# ---------------------------------------------------------------- experts
@functools.lru_cache(maxsize=None)
def _experts(E):
    """(w13 k-major, w2, fp32 oracles [E, 512, 256] / [E, 256, 256]), group 128."""
    from hipserve.ops import quant as Q

    out = []
    for rows, seed, km in ((512, 13, True), (256, 2, False)):
        g = torch.Generator().manual_seed(seed + E)
        u = torch.randint(0, 16, (E, rows, 256), generator=g, dtype=torch.uint8)
        scale = torch.rand(E, rows, 2, generator=g) * 8e-3 + 2e-3
        zero = torch.randint(0, 16, (E, rows, 2), generator=g)
        parts = [Q.QuantPart.from_int4(u[e], scale[e], zero[e], DEV) for e in range(E)]
        out += [Q.QuantMoE(parts, kmajor=km), torch.stack([_oracle(u[e], scale[e], zero[e], 128) for e in range(E)]).to(DEV)]
    return out[0], out[2], out[1], out[3]


@pytest.mark.parametrize("T,E,k", [(5, 16, 4), (48, 16, 4), (64, 128, 8)])
def test_int4_expert_gemm_vs_fp32(T, E, k):
    """qmoe_gemm on INT4 experts: w13 super-chunk major with the SiLU-GLU epilogue, then w2,
    against the fp32 routed computation on the dequantised experts."""
    from hipserve.ops import quant as Q

    op = torch.ops.hipserve
    w13, w2, d13, d2 = _experts(E)
    assert w13.kqt == w2.kqt == Q.KERNEL_QT[Q.INT4] and w13.kmajor and not w2.kmajor
    H, I = 256, 256
    torch.manual_seed(T + E)
    P = T * k
    tile = 16 if P <= 8 * E else 32
    cap = -(-(P + E * (tile - 1)) // tile) * tile
    ids = torch.topk(torch.rand(T, E, device=DEV), k, dim=-1).indices.int()
    slots = torch.empty(cap, dtype=torch.int32, device=DEV)
    te = torch.empty(cap // tile, dtype=torch.int32, device=DEV)
    nt = torch.empty(1, dtype=torch.int32, device=DEV)
    ps = torch.empty(P, dtype=torch.int32, device=DEV)
    op.moe_align(ids, E, tile, slots, te, nt, ps)
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    f32 = torch.empty(0, dtype=torch.float32, device=DEV)
    act = torch.zeros(cap, I, device=DEV, dtype=torch.bfloat16)
    op.qmoe_gemm(act, f32, x, w13.q, w13.rs, w13.kqt, w13.N, w13.K, slots, te, tile, k, 1, True, 1)
    y = torch.zeros(cap, H, device=DEV, dtype=torch.bfloat16)
    op.qmoe_gemm(y, f32, act, w2.q, w2.rs, w2.kqt, w2.N, w2.K, slots, te, tile, 0, 1, False)
    sl = slots.cpu()
    real = (sl >= 0).nonzero().flatten()
    pair = sl[real].long()
    tok = (pair // k).to(DEV)
    ex = ids.flatten()[pair.to(DEV)].long()
    xf = x.float()[tok]                                        # [R, H]
    gu = torch.einsum("rh,rnh->rn", xf, d13[ex])
    a_want = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
    y_want = torch.einsum("ri,rni->rn", a_want, d2[ex])
    rd = real.to(DEV)
    e1 = (act[rd].float() - a_want).abs().max().item()
    e2 = (y[rd].float() - y_want).abs().max().item()
    print(f"int4 experts T={T} E={E}: act err {e1:.3e} / {a_want.abs().max().item():.3e}, "
          f"y err {e2:.3e} / {y_want.abs().max().item():.3e}")
    assert e1 <= 3e-2 * a_want.abs().max().item() + 1e-3
    assert e2 <= 3e-2 * y_want.abs().max().item() + 1e-3


def test_int4_quantmoe_dequantize_both_layouts():
    w13, w2, d13, d2 = _experts(16)
    assert torch.allclose(w13.dequantize().float(), d13.to(torch.bfloat16).float(), rtol=1e-2, atol=1e-6)
    assert torch.allclose(w2.dequantize().float(), d2.to(torch.bfloat16).float(), rtol=1e-2, atol=1e-6)


# ---------------------------------------------------------------- checkpoints
def _tiq():
    spec = importlib.util.spec_from_file_location("tiq", os.path.join(os.path.dirname(__file__), "test_int_quant.py"))
    tiq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tiq)
    return tiq


def _first_logits(path, native, prompts, check):
    import hipserve.models.llama as L
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    L.LlamaModel.native_fp8 = native
    try:
        eng = LLMEngine(EngineConfig(model=str(path), device="cuda", max_num_seqs=4, max_num_batched_tokens=128,
                                     num_kv_blocks=64, max_model_len=256),
                        tp=TPGroup(0, 1, None, torch.device("cuda", 0)))
    finally:
        L.LlamaModel.native_fp8 = True
    mm = eng.runner.model
    check(mm)
    got, orig = [], mm.compute_logits

    def cap(h):
        out = orig(h)
        got.append(out.float().cpu().clone())
        return out

    mm.compute_logits = cap
    eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True))
    eng.shutdown()
    return torch.cat(got)


def _llama(path, fmt, group, seed=11):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                   head_dim=64, intermediate_size=512, vocab_size=320, max_position_embeddings=512,
                                   rms_norm_eps=1e-6, tie_word_embeddings=False)
    torch.manual_seed(seed)
    m = transformers.AutoModelForCausalLM.from_config(cfg, dtype=torch.float32).eval()
    _tiq()._quantise_ckpt(m, path, fmt, bits=4, group=group)


@pytest.mark.parametrize("fmt,group", [("awq", 32), ("awq", 128), ("ct", 32)])
def test_int4_checkpoint_native(tmp_path, fmt, group):
    """An AutoAWQ gemm / compressed-tensors 4-bit checkpoint loads with its projections as
    INT4 QuantWeights; its first-token logits match the same checkpoint dequantised to
    bf16 at load."""
    from hipserve.ops import quant as Q

    path = tmp_path / f"llama-{fmt}{group}"
    _llama(path, fmt, group)
    prompts = [[1, 5, 9, 33, 70, 100], list(range(3, 60))]

    def native(mm):
        for lw in mm.layers:
            for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd):
                assert isinstance(w, Q.QuantWeight) and all(p.kqt == Q.KERNEL_QT[Q.INT4] for p in w.parts)
        assert not isinstance(mm.lm_head, Q.QuantWeight)  # lm_head and the embeddings stay bf16

    def dense(mm):
        for lw in mm.layers:
            assert not any(isinstance(w, Q.QuantWeight) for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd))

    a = _first_logits(path, True, prompts, native)
    b = _first_logits(path, False, prompts, dense)
    err = (a - b).abs().max().item()
    print(f"int4 {fmt} g{group}: logit err {err:.3e} of {b.abs().max().item():.3e}")
    assert err < 5e-2 * b.abs().max().item() + 1e-3


def test_int4_gptq_named_checkpoint_is_not_native(tmp_path):
    """``.qweight`` tensors under a config that says gptq: the INT4 path leaves them alone."""
    from hipserve.ops import quant as Q

    path = tmp_path / "llama-gptq"
    _llama(path, "awq", 32)
    c = json.loads((path / "config.json").read_text())
    c["quantization_config"]["quant_method"] = "gptq"
    (path / "config.json").write_text(json.dumps(c))

    def check(mm):
        for lw in mm.layers:
            for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd):
                assert not isinstance(w, (Q.QuantWeight, Q.QuantMoE))

    _first_logits(path, True, [[1, 5, 9]], check)


def _per_expert_int4_ckpt(path, group=32):
    """Tiny Qwen3-MoE written like an llm-compressor W4A16 export: every decoder Linear
    (attention and per-expert gate / up / down) compressed-tensors pack-quantized 4-bit."""
    import transformers
    from safetensors.torch import load_file, save_file

    from hipserve.weights import int_quant as iq

    cfg = transformers.Qwen3MoeConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                      num_key_value_heads=2, head_dim=64, intermediate_size=512,
                                      moe_intermediate_size=256, num_experts=16, num_experts_per_tok=4,
                                      norm_topk_prob=True, vocab_size=320, max_position_embeddings=512,
                                      rms_norm_eps=1e-6, tie_word_embeddings=False)
    torch.manual_seed(5)
    m = transformers.AutoModelForCausalLM.from_config(cfg, dtype=torch.float32).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("gate.weight"):
                p.mul_(20.0)
    m.save_pretrained(str(path), safe_serialization=True)
    sd = {}
    for f in sorted(path.glob("*.safetensors")):
        sd.update(load_file(str(f)))
        f.unlink()
    out = {}

    def q4(base, w):
        Nw, Kw = w.shape
        scale = w.reshape(Nw, Kw // group, group).abs().amax(-1).clamp_min(1e-8) / 7
        q = torch.round(w / scale.repeat_interleave(group, 1)).clamp(-8, 7).to(torch.int64)
        out[base + ".weight_packed"] = iq.pack_pack_quantized(q, 4)
        out[base + ".weight_scale"] = scale.to(torch.bfloat16)
        out[base + ".weight_shape"] = torch.tensor([Nw, Kw], dtype=torch.int32)

    I = cfg.moe_intermediate_size
    for k, w in sd.items():
        if ".layers." in k and k.endswith("_proj.weight") and w.dim() == 2:  # attention / per-expert Linear
            q4(k[: -len(".weight")], w)
        elif k.endswith("experts.gate_up_proj"):  # fused in this transformers: written per expert
            base = k[: -len("gate_up_proj")]
            for e in range(w.shape[0]):
                q4(f"{base}{e}.gate_proj", w[e, :I])
                q4(f"{base}{e}.up_proj", w[e, I:])
        elif k.endswith("experts.down_proj"):
            base = k[: -len("down_proj")]
            for e in range(w.shape[0]):
                q4(f"{base}{e}.down_proj", w[e])
        else:
            out[k] = w
    save_file(out, str(path / "model.safetensors"))
    c = json.loads((path / "config.json").read_text())
    c["quantization_config"] = {"quant_method": "compressed-tensors", "format": "pack-quantized",
                                "config_groups": {"group_0": {"targets": ["Linear"], "weights": {
                                    "num_bits": 4, "group_size": group, "symmetric": True, "strategy": "group",
                                    "type": "int"}}}, "ignore": ["lm_head"]}
    (path / "config.json").write_text(json.dumps(c))


def test_int4_expert_checkpoint_native(tmp_path):
    pytest.importorskip("transformers")
    from hipserve.ops import quant as Q

    path = tmp_path / "qwen3moe-int4"
    _per_expert_int4_ckpt(path)
    prompts = [[1, 5, 9, 33, 70, 100], list(range(3, 40)), [7] * 12]

    def native(mm):
        for lw in mm.layers:
            assert isinstance(lw.w13, Q.QuantMoE) and lw.w13.kqt == Q.KERNEL_QT[Q.INT4] and lw.w13.kmajor
            assert isinstance(lw.w2, Q.QuantMoE) and lw.w2.kqt == Q.KERNEL_QT[Q.INT4]
            assert isinstance(lw.wqkv, Q.QuantWeight) and lw.wqkv.parts[0].kqt == Q.KERNEL_QT[Q.INT4]

    def dense(mm):
        lw = mm.layers[0]
        assert not isinstance(lw.w13, Q.QuantMoE) and not isinstance(lw.w2, Q.QuantMoE)
        assert not isinstance(lw.wqkv, Q.QuantWeight)

    a = _first_logits(path, True, prompts, native)
    b = _first_logits(path, False, prompts, dense)
    err = (a - b).abs().max().item()
    print(f"int4 qwen3-moe: logit err {err:.3e} of {b.abs().max().item():.3e}")
    assert err < 5e-2 * b.abs().max().item() + 1e-3


# ---------------------------------------------------------------- engine
def test_int4_engine_graph_equals_eager():
    """Synthetic ``quantization: int4`` model: hipGraph decode == eager decode, token for token."""
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.ops import quant as Q
    from hipserve.parallel.comm import TPGroup

    prompts = [[1] + list(range(100, 150)), [1, 5, 6, 7], list(range(3, 30))]
    sp = SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True)
    out = {}
    for eager in (False, True):
        eng = LLMEngine(EngineConfig(model="small-llama", load_format="dummy", device="cuda", max_num_seqs=4,
                                     max_num_batched_tokens=256, max_model_len=256, num_kv_blocks=64,
                                     enforce_eager=eager, extra={"quantization": "int4"}),
                        tp=TPGroup(0, 1, None, torch.device("cuda", 0)))
        lw = eng.runner.model.layers[0]
        for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd):
            assert isinstance(w, Q.QuantWeight) and all(p.kqt == Q.KERNEL_QT[Q.INT4] for p in w.parts)
        assert eng.runner.use_graphs != eager
        res = eng.generate(prompts, sp)
        assert all(len(r[0]) == 16 for r in res)
        assert (eng.runner.stats["graph_steps"] > 0) != eager
        out[eager] = [r[0] for r in res]
        eng.shutdown()
        del eng
        torch.cuda.synchronize()
    assert out[False] == out[True], out
