"""MXFP4 MoE experts on the GPU (csrc/kernels/mxfp4.hip mxfp4_moe_gemm): the W4A8 expert
GEMM over hand-written routing against an fp64 reference of the dequantised operands, the
stack dequantiser against the CPU codec, ``moe()`` end to end, a synthetic MXFP4 MoE model
on hipGraphs against the CPU engine, and a Quark-style per-expert checkpoint."""
import functools

import pytest
import torch

from hipserve.config import PRESETS, EngineConfig
from hipserve.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = (1, 2, 3, 4, 6, 7, 8, 14, 16)


@pytest.fixture(autouse=True, scope="module")
def _lib():
    from hipserve.ops import load_library

    load_library()


@functools.lru_cache(maxsize=None)
def _experts(E, N, K):
    """(QuantMoE, [(nibbles, scales)], fp64 dequantised [E, N, K]): uniform codes (all 16
    occur), every 32-block with its own E8M0 byte from [110, 130]."""
    g = torch.Generator().manual_seed(E * 1000 + N + K)
    raw = []
    for _ in range(E):
        codes = torch.randint(0, 16, (N, K), generator=g)
        assert codes.unique().numel() == 16
        raw.append(((codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8),
                    torch.randint(110, 131, (N, K // 32), generator=g).to(torch.uint8)))
    w = Q.QuantMoE([Q.QuantPart.from_mxfp4(nib, sc, DEV) for nib, sc in raw])
    return w, raw, torch.stack([Q.mxfp4_dequantize(nib, sc) for nib, sc in raw]).double().to(DEV)


@functools.lru_cache(maxsize=None)
def _routing(tile, T):
    """E = 4, k = 2 by hand: token t goes to expert 0 and to expert 1 (token 0: expert 2), so
    expert 0 has T pairs, expert 1 T - 1, expert 2 a single pair and expert 3 none."""
    E, k = 4, 2
    ids = torch.tensor([[0, 2 if t == 0 else 1] for t in range(T)], dtype=torch.int32, device=DEV)
    cap = -(-(T * k + E * (tile - 1)) // tile) * tile
    slots = torch.empty(cap, dtype=torch.int32, device=DEV)
    tile_expert = torch.empty(cap // tile, dtype=torch.int32, device=DEV)
    ntiles = torch.empty(1, dtype=torch.int32, device=DEV)
    pair_slot = torch.empty(T * k, dtype=torch.int32, device=DEV)
    torch.ops.hipserve.moe_align(ids, E, tile, slots, tile_expert, ntiles, pair_slot)
    te, per_tile = tile_expert.cpu(), (slots.cpu() >= 0).view(-1, tile).sum(1)
    assert (te == 3).sum() == 0 and (te == 2).sum() == 1 and per_tile[te == 2].item() == 1
    assert (te == 0).sum() == -(-T // tile) and (te < 0).any()
    # an expert's tiles are contiguous, so only its LAST tile can be padded: every expert's is.
    # Expert 0 spans two tiles wherever T pairs can (T > tile: 40 / 32 and 70 / 64; 5 < 16 cannot)
    assert all(per_tile[te == e][-1] < tile for e in range(3)) and ((te == 0).sum() == 2) == (T > tile)
    return slots, tile_expert, cap


def _act(rows, K, seed):
    from hipserve.ops import pgemm

    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.rand(rows, K, device=DEV, generator=g) * 2 - 1) * torch.logspace(-1, 1, rows, device=DEV).unsqueeze(1)
    xq, xs = pgemm.act_quant(x.to(torch.bfloat16))
    return xq, xs, xq.view(torch.float8_e4m3fn).double() * xs.double().unsqueeze(1)


def _check(tile, T, N, K, gather_k, glu):
    """Every legal S of one case. Bound: test_mxfp4_gemm_vs_fp64's per-row-normalised 1e-4
    (exact products, only the fp32 summation order differs); the GLU form adds the one bf16
    rounding of its output, rtol 2^-8. Padded slots' rows must keep their NaN pre-fill."""
    slots, tile_expert, cap = _routing(tile, T)
    w, _, wd = _experts(4, N, K)
    xq, xs, xd = _act(T if gather_k else cap, K, tile + N + K + gather_k)
    valid = slots >= 0
    s_idx = valid.nonzero().squeeze(1)
    rows = slots[s_idx].long() // gather_k if gather_k else s_idx
    expert = tile_expert[s_idx // tile]
    want = torch.zeros(s_idx.numel(), N, dtype=torch.float64, device=DEV)
    for e in range(3):
        want[expert == e] = xd[rows[expert == e]] @ wd[e].T
    I = N // 2
    if glu:
        want = torch.nn.functional.silu(want[:, :I]) * want[:, I:]
    scale = want.abs().amax(1, keepdim=True).clamp_min(1e-30)
    nsb = K // 256
    for S in [1] if glu else [S for S in range(1, nsb + 1) if nsb % S == 0 and nsb // S in STEPS]:
        out = (torch.full((cap, I), float("nan"), dtype=torch.bfloat16, device=DEV) if glu
               else torch.full((S, cap, N), float("nan"), device=DEV))
        torch.ops.hipserve.mxfp4_moe_gemm(out, xq, xs, w.q, N, K, slots, tile_expert, tile, gather_k, S, glu)
        rows_out = out if glu else out.permute(1, 0, 2).reshape(cap, S * N)
        assert rows_out[~valid].isnan().all() and not rows_out[valid].isnan().any()
        got = (out if glu else out.sum(0))[valid].double()
        err = ((got - want) / scale).abs().max().item()
        print(f"tile={tile} T={T} N={N} K={K} gather_k={gather_k} glu={glu} S={S} max normalised error {err:.3e}")
        torch.testing.assert_close(got / scale, want / scale, rtol=2.0 ** -8 if glu else 0, atol=1e-4)


# idle waves in a tile | three steps or three slices | two N tiles and a wrap of the 5-slot ring
@pytest.mark.parametrize("gather_k", [2, 0])
@pytest.mark.parametrize("N,K", [(32, 256), (144, 768), (256, 1536)])
@pytest.mark.parametrize("tile,T", [(16, 5), (32, 40), (64, 70)])
def test_mxfp4_moe_partials_vs_fp64(tile, T, N, K, gather_k):
    _check(tile, T, N, K, gather_k, 0)


@pytest.mark.parametrize("I,K", [(16, 256), (144, 768)])
@pytest.mark.parametrize("tile,T", [(16, 5), (32, 40), (64, 70)])
def test_mxfp4_moe_glu_vs_fp64(tile, T, I, K):
    _check(tile, T, 2 * I, K, 2, 1)


def test_quant_moe_dequantize_is_the_codec():
    w, raw, _ = _experts(3, 32, 512)
    with pytest.raises(ValueError, match="k-major"):
        Q.QuantMoE([Q.QuantPart.from_mxfp4(nib, sc, DEV) for nib, sc in raw], kmajor=True)
    assert w.kqt == Q.MXFP4_KQT and w.rs.numel() == 0 and not w.kmajor and Q.QuantMoE.supported(w.kqt, 32, 512)
    want = torch.stack([Q.mxfp4_dequantize(nib, sc) for nib, sc in raw]).to(torch.bfloat16)
    assert torch.equal(w.dequantize().cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("T,E,k,I", [(6, 8, 2, 768), (40, 8, 2, 512), (33, 64, 4, 256), (1100, 8, 2, 512)])
def test_mxfp4_moe_vs_fp64(T, E, k, I):
    """``moe()`` on MXFP4 experts (tests/test_quant_moe_gpu.py's set-up and bound) against fp64
    with the kernel path's two e4m3 roundings (x, and the bf16-rounded act); the last case has
    more pairs than the expert kernels take and runs the dequantised bf16 experts instead."""
    from hipserve.models.llama import LayerWeights, LlamaModel
    from hipserve.models.moe import MOE_KERNEL_MAX_PAIRS
    from hipserve.ops import KernelOps, pgemm
    from hipserve.parallel.comm import TPGroup

    H, w4a8 = 512, T * k <= MOE_KERNEL_MAX_PAIRS
    cfg = PRESETS["tiny-mixtral"].replace(hidden_size=H, intermediate_size=I, num_experts=E, num_experts_per_tok=k)
    m = LlamaModel(cfg, TPGroup(0, 1, None, torch.device(DEV)), DEV, torch.bfloat16, KernelOps())
    torch.manual_seed(T + E + I)
    router = torch.randn(E, H, device=DEV, dtype=torch.bfloat16) * 0.3

    def stack(w):
        raw = [Q.mxfp4_quantize(w[e]) for e in range(E)]
        return (Q.QuantMoE([Q.QuantPart.from_mxfp4(nib, sc, DEV) for nib, sc in raw]),
                torch.stack([Q.mxfp4_dequantize(nib, sc) for nib, sc in raw]).double().to(DEV))

    (w13, d13), (w2, d2) = stack(torch.randn(E, 2 * I, H) * 0.05), stack(torch.randn(E, H, I) * 0.05)
    lw = LayerWeights(ln1=None, wqkv=None, wo=None, ln2=None, router=router, w13=w13, w2=w2)
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)

    def e4m3(t):  # the per-row dynamic e4m3 copy the W4A8 kernel reads, as fp64
        tq, ts = pgemm.act_quant(t.contiguous())
        return tq.view(torch.float8_e4m3fn).double() * ts.double().unsqueeze(1)

    got = m.moe(x, lw).double()
    wts, idx = torch.topk(torch.softmax(torch.nn.functional.linear(x, router).float(), -1), k, -1)
    wts = (wts / wts.sum(-1, keepdim=True)).double()
    want = torch.zeros(T, H, device=DEV, dtype=torch.float64)
    xd = e4m3(x) if w4a8 else x.double()
    for e in range(E):
        rows, slot = (idx == e).nonzero(as_tuple=True)
        if rows.numel() == 0:
            continue
        gu = xd[rows] @ d13[e].T
        act = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]).to(torch.bfloat16)
        want.index_add_(0, rows, ((e4m3(act) if w4a8 else act.double()) @ d2[e].T) * wts[rows, slot].unsqueeze(-1))
    err = (got - want).abs().max().item()
    print(f"T={T} E={E} k={k} I={I} max error {err:.3e} of max |want| {want.abs().max().item():.3e}")
    assert err <= 3e-2 * want.abs().max().item() + 1e-3, err
    if not w4a8:
        return
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.moe(x, lw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = m.moe(x, lw)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g.double(), got)


CFG = PRESETS["tiny-mixtral"].replace(hidden_size=256, head_dim=64, intermediate_size=256)
# Seed and prompts chosen on the CPU (fp32 engine, these weights) among 14 seeds x 40 random
# prompts of 3-6 tokens: over the prompt and the 8 greedy steps the top-2 logit gap is at least
# 0.109 / 0.080 / 0.067 for the three prompts, and the router's gap between its 2nd and 3rd
# probability at least 1.3 % / 1.3 % / 1.2 % of the 2nd (the dummy router is nearly uniform
# over its 4 experts; the e4m3 activations move a router logit by a few 1e-3)
SEED = 3
PROMPTS = [[1, 321, 41, 397], [1, 39, 192, 84], [1, 330, 73, 96, 364, 415]]


def _engine(device, **kw):
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    cfg = EngineConfig(model="tiny-mixtral", load_format="dummy", device=device, max_num_seqs=4,
                       max_num_batched_tokens=64, max_model_len=256, num_kv_blocks=128, seed=SEED,
                       extra={"quantization": "mxfp4"}, **kw)
    return LLMEngine(cfg, tp=TPGroup(0, 1, None, dev), model_cfg=CFG)


def test_moe_engine_greedy_matches_cpu_on_graphs():
    from hipserve.engine.request import SamplingParams

    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    g = _engine("cuda", dtype="bfloat16", enforce_eager=False)
    for lw in g.runner.model.layers:
        assert all(isinstance(w, Q.QuantMoE) and w.kqt == Q.MXFP4_KQT and not w.kmajor for w in (lw.w13, lw.w2))
    c = _engine("cpu", dtype="float32")
    assert torch.equal(c.runner.model.layers[1].w2, g.runner.model.layers[1].w2.dequantize().float().cpu())
    got, want = g.generate(PROMPTS, sp), c.generate(PROMPTS, sp)
    assert g.runner.use_graphs and g.runner.stats["graph_steps"] >= 7
    assert [r[0] for r in got] == [r[0] for r in want]


def _per_expert_mxfp4_ckpt(path):
    """Tiny Qwen3-MoE written like a Quark MXFP4 export: every attention and per-expert Linear
    as uint8 ``.weight`` (two e2m1 codes per byte) + E8M0 ``.weight_scale``; router and lm_head bf16."""
    import json

    import transformers
    from safetensors.torch import load_file, save_file

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
        out[base + ".weight"], out[base + ".weight_scale"] = Q.mxfp4_quantize(w)

    I = cfg.moe_intermediate_size
    for k, w in sd.items():
        if k.endswith("_proj.weight") and w.dim() == 2:  # attention and per-expert Linear
            q4(k[: -len(".weight")], w)
        elif k.endswith("experts.gate_up_proj"):  # fused layout of newer transformers: written per expert
            for e in range(w.shape[0]):
                q4(f"{k[: -len('gate_up_proj')]}{e}.gate_proj", w[e, :I])
                q4(f"{k[: -len('gate_up_proj')]}{e}.up_proj", w[e, I:])
        elif k.endswith("experts.down_proj"):
            for e in range(w.shape[0]):
                q4(f"{k[: -len('down_proj')]}{e}.down_proj", w[e])
        else:
            out[k] = w.to(torch.bfloat16)
    save_file(out, str(path / "model.safetensors"))
    c = json.loads((path / "config.json").read_text())
    c["quantization_config"] = {"quant_method": "quark", "exclude": ["lm_head"], "global_quant_config": {
        "weight": {"dtype": "fp4", "group_size": 32, "scale_format": "e8m0", "qscheme": "per_group"}}}
    (path / "config.json").write_text(json.dumps(c))


def test_mxfp4_expert_checkpoint_native(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    path = tmp_path / "qwen3moe-mxfp4"
    path.mkdir()
    _per_expert_mxfp4_ckpt(path)
    # chosen on the CPU (fp32 engine on this checkpoint) among 60 random prompts, whose median top-2
    # logit gap over the 4 greedy steps is 0.021: these keep at least 0.272 / 0.171 / 0.116
    prompts = [[1, 3, 157, 314, 99, 101, 16, 289], [1, 295, 72, 34, 90, 54, 142, 218, 91, 255, 112, 27, 54, 82, 219],
               [1, 310, 239, 70, 311, 96, 142, 240, 182, 289, 76, 178, 125, 73, 11, 47, 79, 228, 8, 199, 53]]
    got = {}
    for native in (True, False):
        monkeypatch.setenv("HIPSERVE_MXFP4_MOE_NATIVE", "1" if native else "0")
        eng = LLMEngine(EngineConfig(model=str(path), device="cuda", max_num_seqs=4, max_num_batched_tokens=128,
                                     num_kv_blocks=64, max_model_len=256),
                        tp=TPGroup(0, 1, None, torch.device("cuda", 0)))
        for lw in eng.runner.model.layers:
            assert all((isinstance(w, Q.QuantMoE) and w.kqt == Q.MXFP4_KQT) == native for w in (lw.w13, lw.w2))
        got[native] = [r[0] for r in eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=4,
                                                                          ignore_eos=True))]
        eng.shutdown()
    assert got[True] == got[False]
