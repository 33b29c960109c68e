"""Attention at head_dim 256 (Gemma-3 1B / 4B / 12B) on the gfx950 kernels: paged decode
(bf16 and e4m3 caches, its one-wave-per-SIMD register plan), prefill v1, the cache writers,
and the engine's refusal of a head size without a kernel. Oracles and tolerances are those
of test_kernels_gpu.py / test_kv_fp8_gpu.py at 64 / 96 / 128."""
import functools
import math

import pytest
import torch

from hipserve.ops import KernelOps
from hipserve.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
D = 256
# test_paged_decode's contexts, then one below / at / above the e4m3 kernel's 64-key chunk
# and the 512-key partition (the bf16 kernel's chunk is 32 keys, as at the other sizes)
CTX = [1, 17, 100, 600, 1300, 512, 33, 63, 64, 65, 511, 513]
MAX_BLOCKS = 96
SHAPES = [(8, 4), (4, 1), (16, 1), (8, 8), (16, 8)]
SEQS = [(1, 1), (37, 37), (300, 50), (129, 129), (1100, 1100), (1500, 333)]


@pytest.fixture(scope="module")
def ops():
    return KernelOps()


def _close(a, b, atol, rtol=0.0):
    a, b = a.float().cpu(), b.float().cpu()
    bad = (a - b).abs() > (atol + rtol * b.abs())
    assert not bad.any(), f"max err {(a - b).abs().max().item()}"


@functools.lru_cache(maxsize=None)
def _decode_case(nq, nkv, bs, window, f8):
    """Inputs and the fp32 oracle of one decode case, shared by the partition sizes."""
    g = torch.Generator(device=DEV).manual_seed(2 + nq + 3 * nkv + bs)
    B, nblocks = len(CTX), len(CTX) * MAX_BLOCKS
    kc = torch.randn(nblocks, nkv, bs, D, device=DEV, generator=g)
    vc = torch.randn(nblocks, nkv, D, bs, device=DEV, generator=g)
    kc, vc = (ref.to_cache(kc, F8), ref.to_cache(vc, F8)) if f8 else (kc.bfloat16(), vc.bfloat16())
    bt = torch.randperm(nblocks, device=DEV, generator=g).int().view(B, MAX_BLOCKS).contiguous()
    cl = torch.tensor(CTX, device=DEV, dtype=torch.int32)
    q = torch.randn(B, (nq + 2 * nkv) * D, device=DEV, generator=g).bfloat16()
    scale = 1.0 / math.sqrt(D)
    want = ref.paged_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cl.cpu(), nq, nkv, scale, window)
    return kc, vc, bt, cl, q, scale, want


def _run_decode(ops, case, nq, nkv, bs, part, window, widen=False, out16=None):
    kc, vc, bt, cl, q, scale, _ = case
    if widen:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    B = len(CTX)
    max_parts = math.ceil(MAX_BLOCKS * bs / part)
    tmp_out = torch.empty(B, nq, max_parts, D, device=DEV, dtype=torch.float32)
    tmp_ml = torch.empty(B, nq, max_parts, 2, device=DEV, dtype=torch.float32)
    out = torch.zeros(B, nq * D, device=DEV, dtype=torch.bfloat16)
    ops.paged_decode(out, q, kc, vc, bt, cl, tmp_out, tmp_ml, nq, nkv, part, scale, window, out16)
    return out


@pytest.mark.parametrize("nq,nkv", SHAPES)
@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize("part", [512, 2048])
@pytest.mark.parametrize("window", [0, 100, 512])
def test_paged_decode_d256(ops, nq, nkv, bs, part, window):
    """GQA groups 2, 4, 16, 1, 2 (the 4B, 1B and 12B head layouts among them), one and several
    partitions, sliding windows below and at the partition size, vs the fp32 oracle.
    HIPSERVE_DECODE_WAVES does not apply at 256: the kernel always runs 4 waves."""
    case = _decode_case(nq, nkv, bs, window, False)
    B = len(CTX)
    out16 = torch.full((B, nq * D), float("nan"), device=DEV, dtype=torch.float16)
    out = _run_decode(ops, case, nq, nkv, bs, part, window, out16=out16)
    _close(out.view(B, nq, D), case[-1], atol=2e-2, rtol=2e-2)
    # the f16 pair-order copy of the bf16 output, exactly (attention and merge kernels write it)
    h = out.float().to(torch.float16).view(B, -1, 8)[:, :, [0, 2, 1, 3, 4, 6, 5, 7]].reshape(B, -1)
    assert torch.equal(out16, h)


@pytest.mark.parametrize("nq,nkv", SHAPES)
@pytest.mark.parametrize("part", [512, 2048])
@pytest.mark.parametrize("window", [0, 100, 512])
def test_paged_decode_d256_fp8_cache(ops, nq, nkv, part, window):
    """e4m3 cache (64-key chunks) vs the fp32 oracle over the same cache, and vs the bf16
    kernel on the widened cache (another fp32 summation order)."""
    bs = 16
    case = _decode_case(nq, nkv, bs, window, True)
    out = _run_decode(ops, case, nq, nkv, bs, part, window)
    _close(out.view(len(CTX), nq, D), case[-1], atol=2e-2, rtol=2e-2)
    out_b = _run_decode(ops, case, nq, nkv, bs, part, window, widen=True)
    _close(out, out_b, atol=1e-2, rtol=1e-2)


@functools.lru_cache(maxsize=None)
def _prefill_case(nq, nkv, window):
    g = torch.Generator(device=DEV).manual_seed(4 + nq + nkv)
    bs = 16
    max_blocks = 1536 // bs
    n = len(SEQS) * max_blocks
    kc = ref.to_cache(torch.randn(n, nkv, bs, D, device=DEV, generator=g), F8)
    vc = ref.to_cache(torch.randn(n, nkv, D, bs, device=DEV, generator=g), F8)
    bt = torch.randperm(n, device=DEV, generator=g).int().view(len(SEQS), max_blocks).contiguous()
    cu, tiles = [0], []
    for i, (c, ql) in enumerate(SEQS):
        tiles += [(i, r) for r in range(0, ql, 128)]
        cu.append(cu[-1] + ql)
    q = torch.randn(cu[-1], (nq + 2 * nkv) * D, device=DEV, generator=g).bfloat16() * 2
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    ctx_t = torch.tensor([c for c, _ in SEQS], device=DEV, dtype=torch.int32)
    tiles_t = torch.tensor(tiles, device=DEV, dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    want = ref.prefill_attention(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cu_t.cpu(), ctx_t.cpu(), nq, nkv, scale,
                                 window)
    return kc, vc, bt, cu_t, ctx_t, tiles_t, q, scale, want


@pytest.mark.parametrize("nq,nkv", [(8, 4), (4, 1), (4, 4)])
@pytest.mark.parametrize("window", [0, 200])
def test_prefill_attention_d256(ops, nq, nkv, window):
    """v1 at head_dim 256 (plain, tiny, chunked over a prefix, long) over an e4m3 cache and
    over the same cache widened to bf16: both vs the fp32 oracle, and equal to each other."""
    kc, vc, bt, cu_t, ctx_t, tiles_t, q, scale, want = _prefill_case(nq, nkv, window)
    T = q.shape[0]
    outs = []
    for k, v in ((kc, vc), (kc.to(torch.bfloat16), vc.to(torch.bfloat16))):
        out = torch.zeros(T, nq * D, device=DEV, dtype=torch.bfloat16)
        ops.prefill_attention(out, q, k, v, bt, cu_t, ctx_t, tiles_t, nq, nkv, scale, window)
        _close(out.view(T, nq, D), want, atol=2e-2, rtol=2e-2)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T", [37, 2100])
def test_rope_cache_d256(ops, mode, T):
    """Per-token and 16-token tile writers at head_dim 256 vs the fp32 oracle; the e4m3 cache
    is the rounding of the bf16 kernel's cache, byte for byte."""
    torch.manual_seed(1)
    nq, nkv, bs = 8, 4, 16
    qkv = torch.randn(T, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
    pos = torch.randint(0, 4000, (T,), device=DEV)
    nb = max(64, (T + 2 * bs) // bs + 1)
    slots = torch.randperm(nb * bs, device=DEV)[:T] if T < 2048 else torch.arange(T, device=DEV) + bs
    slots[3] = -1
    cs = ref.rope_cos_sin(D, 4096, 1e6).to(DEV)
    kb = torch.zeros(nb, nkv, bs, D, device=DEV, dtype=torch.bfloat16)
    vb = torch.zeros(nb, nkv, D, bs, device=DEV, dtype=torch.bfloat16)
    k8, v8 = kb.to(F8), vb.to(F8)
    kc_r, vc_r, qkv_r = kb.cpu().clone(), vb.cpu().clone(), qkv.cpu().clone()
    q_b, q_8 = qkv.clone(), qkv.clone()
    ops.rope_cache(q_b, pos, slots, cs, kb, vb, nq, nkv, D, mode)
    ops.rope_cache(q_8, pos, slots, cs, k8, v8, nq, nkv, D, mode)
    ref.rope_cache(qkv_r, pos.cpu(), slots.cpu(), cs.cpu(), kc_r, vc_r, nq, nkv, D, mode)
    _close(q_b[:, : nq * D], qkv_r[:, : nq * D], atol=2e-2, rtol=1e-2)
    _close(kb, kc_r, atol=2e-2, rtol=1e-2)
    _close(vb, vc_r, atol=0)
    assert torch.equal(q_b[:, : nq * D], q_8[:, : nq * D])
    assert torch.equal(k8.view(torch.uint8), ref.to_cache(kb, F8).view(torch.uint8))
    assert torch.equal(v8.view(torch.uint8), ref.to_cache(vb, F8).view(torch.uint8))


@pytest.mark.parametrize("S", [1, 3])
def test_splitk_rope_cache_qk_norm_d256(ops, S):
    """The decode layer's split-K RoPE epilogue with per-head q/k RMSNorm at head_dim 256 ==
    bf16 reduce -> qk_rmsnorm -> rope_cache, bit for bit; e4m3 cache = rounded bf16 cache."""
    T, nq, nkv, bs = 29, 8, 4, 16
    N = (nq + 2 * nkv) * D
    g = torch.Generator(device=DEV).manual_seed(11 + S)
    ws = torch.randn(S, T, N, device=DEV, generator=g)
    h = ws[0].clone()
    for s in range(1, S):
        h = h + ws[s]
    qkv1 = h.to(torch.bfloat16)
    qw = 1 + 0.2 * torch.randn(D, device=DEV, generator=g)
    kw = 1 + 0.2 * torch.randn(D, device=DEV, generator=g)
    ops.qk_rmsnorm(qkv1, qw, kw, nq, nkv, D, 1e-6)
    pos = torch.randint(0, 4000, (T,), device=DEV, generator=g)
    slots = torch.randperm(64 * bs, device=DEV, generator=g)[:T]
    slots[5] = -1
    cs = ref.rope_cos_sin(D, 4096, 1e6).to(DEV)
    kc1 = torch.zeros(64, nkv, bs, D, device=DEV, dtype=torch.bfloat16)
    vc1 = torch.zeros(64, nkv, D, bs, device=DEV, dtype=torch.bfloat16)
    ops.rope_cache(qkv1, pos, slots, cs, kc1, vc1, nq, nkv, D, 0)
    for dt in (torch.bfloat16, F8):
        kc2, vc2 = torch.zeros_like(kc1, dtype=dt), torch.zeros_like(vc1, dtype=dt)
        qkv2 = torch.zeros(T, N, device=DEV, dtype=torch.bfloat16)
        torch.ops.hipserve.splitk_rope_cache(qkv2, ws, S, pos, slots, cs, kc2, vc2, nq, nkv, D, 0, None, qw, kw, 1e-6)
        assert torch.equal(qkv1[:, : nq * D], qkv2[:, : nq * D])
        assert torch.equal(kc2.view(torch.uint8), ref.to_cache(kc1, dt).view(torch.uint8))
        assert torch.equal(vc2.view(torch.uint8), ref.to_cache(vc1, dt).view(torch.uint8))


def test_unsupported_head_dim_is_refused_at_engine_construction():
    """A head size without an attention kernel fails when the engine is built, naming the
    supported sizes, not as a kernel argument check on the first forward."""
    from hipserve.config import EngineConfig, PRESETS
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    mcfg = PRESETS["small-llama"].replace(name="head-80", head_dim=80)
    cfg = EngineConfig(model="head-80", load_format="dummy", device="cuda", max_num_seqs=4,
                       max_num_batched_tokens=256, max_model_len=512, num_kv_blocks=64, enforce_eager=True)
    with pytest.raises(ValueError, match="64, 96, 128, 256"):
        LLMEngine(cfg, tp=TPGroup(0, 1, None, torch.device("cuda", 0)), model_cfg=mcfg)
