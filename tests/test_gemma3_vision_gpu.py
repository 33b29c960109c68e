"""Gemma-3 image input on the gfx950 kernels: ``prefill_attention`` with per-row key limits
(both kernels, bf16 and e4m3 caches, with and without a window) against the fp32 reference,
``vision_pool_rmsnorm``, ``vision_attention`` without RoPE, the SigLIP tower on the GPU against
the CPU ops, a small Gemma-3 image model end to end (hipGraph decode after the image prefill)
against the CPU engine, and the binding's refusals.

Attention tolerance: atol = rtol = 2e-2, the project's (test_kernels_gpu.py). Every attention
case first asserts on the CPU that its fixture discriminates: on the rows of the image blocks
the oracle with the limits and the causal oracle differ by more than 10 x the tolerance in at
least 40 % of the rows (the criterion of test_softcap_gpu.py), and are equal on every row
outside a block, so a kernel that ignored the limits could not pass."""
import functools
import math

import numpy as np
import pytest
import torch

from hipserve.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
TOL = 2e-2
BS = 16
# (context, rows of the chunk, image blocks as [first, last) ROWS of the chunk)
#  0: one 200-row chunk on 48 cached tokens; its blocks straddle a 32-row wave (rows 20..59), a
#     64-key tile and the 128-row workgroup tile (rows 120..135)
#  1: a block that ends the sequence
#  2: no block
#  3: a whole prompt whose block crosses absolute key 64 and a wave, and a 64-token block (the
#     window used below) that starts a 128-row tile
SEQS = [(248, 200, [(20, 60), (120, 136)]), (70, 70, [(40, 70)]), (43, 33, []), (230, 230, [(50, 80), (128, 192)])]
WINDOW = 64


@pytest.fixture(scope="module")
def ops():
    from hipserve.ops import KernelOps

    return KernelOps()


def _close(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    bad = (a - b).abs() > (TOL + TOL * b.abs())
    assert not bad.any(), f"max err {(a - b).abs().max().item()}"


@functools.lru_cache(maxsize=None)
def _case(D, nq, nkv, f8, window):
    """CPU inputs of one case and its fp32 oracle, computed once and shared."""
    g = torch.Generator().manual_seed(211 + D + 3 * nq + nkv)
    max_blocks = 256 // BS
    n = len(SEQS) * max_blocks
    kc, vc = torch.randn(n, nkv, BS, D, generator=g), torch.randn(n, nkv, D, BS, generator=g)
    kc, vc = (ref.to_cache(kc, F8), ref.to_cache(vc, F8)) if f8 else (kc.bfloat16(), vc.bfloat16())
    bt = torch.randperm(n, generator=g).int().view(len(SEQS), max_blocks).contiguous()
    cu, tiles, lim, own, inblock = [0], [], [], [], []
    for i, (c, ql, blocks) in enumerate(SEQS):
        tiles += [(i, r) for r in range(0, ql, 128)]
        cu.append(cu[-1] + ql)
        pos = list(range(c - ql, c))
        own += pos
        row_lim, row_in = list(pos), [False] * ql
        for a, b in blocks:
            assert b - a <= WINDOW  # the engine's guarantee (one limit per row is enough)
            for r in range(a, b):
                row_lim[r], row_in[r] = c - ql + b - 1, r < b - 1
        lim += row_lim
        inblock += row_in
    q = (torch.randn(cu[-1], (nq + 2 * nkv) * D, generator=g) * 2.0).bfloat16()  # sharp scores
    t = dict(kc=kc, vc=vc, bt=bt, cu=torch.tensor(cu, dtype=torch.int32),
             ctx=torch.tensor([c for c, _, _ in SEQS], dtype=torch.int32),
             tiles=torch.tensor(tiles, dtype=torch.int32), q=q,
             limits=torch.tensor(lim, dtype=torch.int32), own=torch.tensor(own, dtype=torch.int32))
    scale = 1.0 / math.sqrt(D)
    want = ref.prefill_attention(q, kc, vc, bt, t["cu"], t["ctx"], nq, nkv, scale, window, 0.0, t["limits"])
    causal = ref.prefill_attention(q, kc, vc, bt, t["cu"], t["ctx"], nq, nkv, scale, window)
    rows = torch.tensor(inblock)
    far = ((want.float() - causal.float()).abs().amax(-1) > 10 * TOL)[rows].float().mean().item()
    same = torch.equal(want[~torch.tensor([l != o for l, o in zip(lim, own)])],
                       causal[~torch.tensor([l != o for l, o in zip(lim, own)])])
    return t, scale, want, far, same


def _run(ops, t, nq, nkv, D, scale, window, limits):
    d = {k: v.to(DEV) for k, v in t.items()}
    out = torch.zeros(d["q"].shape[0], nq * D, device=DEV, dtype=torch.bfloat16)
    lim = None if limits is None else d[limits]
    ops.prefill_attention(out, d["q"], d["kc"], d["vc"], d["bt"], d["cu"], d["ctx"], d["tiles"], nq, nkv, scale,
                          window, 0.0, lim)
    return out


# head_dim 128 with 4 / 2 heads runs v2 (LDS tiles shared by the GQA group), 2 / 2 runs v1; 256 runs v1
@pytest.mark.parametrize("window", [0, WINDOW])
@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("D,nq,nkv", [(128, 4, 2), (128, 2, 2), (256, 4, 2)])
def test_prefill_attention_limits(ops, D, nq, nkv, f8, window):
    t, scale, want, far, same = _case(D, nq, nkv, f8, window)
    assert far >= 0.4 and same, f"fixture does not discriminate: {far:.2f}"
    out = _run(ops, t, nq, nkv, D, scale, window, "limits")
    _close(out.view(-1, nq, D), want)
    # limits equal to each row's own position: the plain causal kernel's output, bit for bit
    assert torch.equal(_run(ops, t, nq, nkv, D, scale, window, "own"), _run(ops, t, nq, nkv, D, scale, window, None))


def test_prefill_attention_limits_refusals(ops):
    t, scale, _, _, _ = _case(128, 4, 2, False, 0)
    d = {k: v.to(DEV) for k, v in t.items()}
    T = d["q"].shape[0]
    out = torch.zeros(T, 4 * 128, device=DEV, dtype=torch.bfloat16)

    def call(limits, softcap=0.0, q=d["q"], kc=d["kc"], vc=d["vc"], o=out, nq=4, nkv=2):
        ops.prefill_attention(o, q, kc, vc, d["bt"], d["cu"], d["ctx"], d["tiles"], nq, nkv, scale, 0, softcap,
                              limits)

    with pytest.raises(RuntimeError, match="limits with softcap"):
        call(d["limits"], softcap=30.0)
    with pytest.raises(RuntimeError, match="limits must be int32"):
        call(d["limits"].long())
    with pytest.raises(RuntimeError, match="limits must have exactly"):
        call(d["limits"][:-1])
    with pytest.raises(RuntimeError, match="limits must be a tensor on"):
        call(t["limits"])
    kc64 = torch.zeros(d["kc"].shape[0], 2, BS, 64, device=DEV, dtype=torch.bfloat16)
    vc64 = torch.zeros(d["kc"].shape[0], 2, 64, BS, device=DEV, dtype=torch.bfloat16)
    q64 = torch.zeros(T, 8 * 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="limits need head_dim 128 or 256"):
        call(d["limits"], q=q64, kc=kc64, vc=vc64, o=torch.zeros(T, 4 * 64, device=DEV, dtype=torch.bfloat16))
    torch.cuda.synchronize()


@pytest.mark.parametrize("g,k", [(8, 4), (4, 2)])
@pytest.mark.parametrize("C", [1152, 64])
def test_vision_pool_rmsnorm_vs_fp32(ops, C, g, k):
    """fp32 pool + norm, one rounding to bf16: within one bf16 ulp (2^-7 relative) of the fp32
    reference (half an ulp of rounding, the rest for the order of the fp32 sums)."""
    torch.manual_seed(C + g)
    images = 3
    x = (torch.randn(images * g * g, C) * 2 + 0.3).bfloat16()
    w = (0.2 * torch.randn(C)).bfloat16()
    want = ref.vision_pool_rmsnorm(x.float(), w.float(), g, k, 1e-6)
    out = torch.full((images * (g // k) ** 2, C), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.vision_pool_rmsnorm(out, x.to(DEV), w.to(DEV), g, k, 1e-6)
    err = (out.float().cpu() - want).abs()
    assert (err <= 2.0 ** -7 * want.abs() + 1e-6).all(), err.max().item()
    with pytest.raises(RuntimeError, match="must divide"):
        ops.vision_pool_rmsnorm(out, x.to(DEV), w.to(DEV), g, 3, 1e-6)


@pytest.mark.parametrize("nh,lens", [(16, [1024, 96, 333]), (2, [16])])
def test_vision_attention_without_rope(ops, nh, lens):
    """cos_sin = None: q and k are left as they are, and the attention is the reference's
    (the tolerance of test_vision_gpu.py's attention test)."""
    from hipserve.models.vision import ImageGeometry

    D = 72
    torch.manual_seed(nh)
    T = sum(lens)
    qkv = torch.randn(T, 3 * nh * D).bfloat16()
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    want = ref.vision_attention(qkv, cu, nh, D, D ** -0.5).float()
    meta = ops.vision_meta(ImageGeometry([], None, None, None, cu), nh, D)
    qd = qkv.to(DEV)
    out = torch.empty(T, nh * D, device=DEV, dtype=torch.bfloat16)
    ops.vision_attention(out, qd, None, meta[0], nh, D, D ** -0.5, meta)
    assert torch.equal(qd.cpu(), qkv)
    err = (out.float().cpu() - want).abs().max().item()
    assert err <= 2e-2 * want.abs().max().item() + 1e-3, err


def _model_cfg(D, nq, nkv):
    from hipserve.config import ModelConfig, VisionConfig

    vis = VisionConfig(kind="siglip", depth=2, hidden_size=144, intermediate_size=320, num_heads=2, patch_size=14,
                       temporal_patch_size=1, spatial_merge_size=1, out_hidden_size=256, num_position_embeddings=64,
                       deepstack_visual_indexes=(), image_size=112, mm_tokens_per_image=16, image_token_id=900,
                       vision_start_token_id=902, vision_end_token_id=903)
    return ModelConfig(name=f"gemma-3-mm-test-{D}", family="gemma3", hidden_size=256, num_layers=2, num_heads=nq,
                       num_kv_heads=nkv, head_dim=D, intermediate_size=512, vocab_size=1024, rms_norm_eps=1e-6,
                       rope_theta=1e6, max_position_embeddings=2048, tie_word_embeddings=True, qk_norm=True,
                       hidden_act="gelu_tanh", sandwich_norm=True, norm_offset=True, embed_scale=16.0,
                       attn_scale=D ** -0.5, sliding_window=64, layer_windows=(64, 0), rope_local_theta=1e4,
                       bos_token_id=2, eos_token_id=(1,), vision=vis)


def _engine(device, mcfg):
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    dt = "bfloat16" if device == "cuda" else "float32"
    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    return LLMEngine(EngineConfig(model=mcfg.name, load_format="dummy", device=device, dtype=dt, max_num_seqs=4,
                                  max_num_batched_tokens=512, max_model_len=1024, num_kv_blocks=256),
                     tp=TPGroup(0, 1, None, dev), model_cfg=mcfg)


def _images(vc, n):
    PIL = pytest.importorskip("PIL.Image")
    from hipserve.multimodal import preprocess_image

    rng = np.random.default_rng(0)
    return [preprocess_image(PIL.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), vc)
            for w, h in ((300, 200), (160, 256))[:n]]


def test_siglip_tower_gpu_vs_cpu():
    """The bf16 tower + projector on the kernels against the fp32 tower on the reference ops,
    same (keyed) random weights; the criterion of test_vision_gpu.py's tower test."""
    mcfg = _model_cfg(128, 4, 2)
    g, c = _engine("cuda", mcfg), _engine("cpu", mcfg)
    vg, vc_ = g.runner.model.visual, c.runner.model.visual
    assert torch.equal(vg.blocks[1].fc1_w.float().cpu(), vc_.blocks[1].fc1_w)
    ims = _images(mcfg.vision, 2)
    pix = torch.from_numpy(np.concatenate([i.pixels for i in ims]))
    eg, _ = vg.forward(pix)
    ec, _ = vc_.forward(pix)
    assert eg.shape == (32, 256) and ec.norm() > 0
    rel = (eg.float().cpu() - ec).norm() / ec.norm()
    assert rel < 0.03, rel


@pytest.mark.parametrize("D,nq,nkv", [(256, 2, 1), (128, 4, 2)])
def test_gemma3_image_engine_gpu_vs_cpu(D, nq, nkv):
    """Image prefill (limits in both prefill kernels, window 64 < prompt) then hipGraph decode:
    the bf16 GPU engine's first greedy token is the fp32 CPU engine's, as in test_vision_gpu.py."""
    from hipserve.engine.request import SamplingParams
    from hipserve.multimodal import MultiModalPrompt, expand_image_tokens

    mcfg = _model_cfg(D, nq, nkv)
    g, c = _engine("cuda", mcfg), _engine("cpu", mcfg)
    assert g.runner.use_graphs
    ims = _images(mcfg.vision, 2)
    rng = np.random.default_rng(1)
    ids = expand_image_tokens([2] + rng.integers(4, 890, 70).tolist() + [902, 900, 903] +
                              rng.integers(4, 890, 20).tolist() + [902, 900, 903] + rng.integers(4, 890, 9).tolist(),
                              ims, mcfg.vision)
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    rg = g.generate([MultiModalPrompt(ids, ims)], sp)
    rc = c.generate([MultiModalPrompt(ids, ims)], sp)
    assert len(rg[0][0]) == 6 and g.runner.stats["graph_steps"] > 0
    assert rg[0][0][0] == rc[0][0][0]
    g.shutdown()
    c.shutdown()
