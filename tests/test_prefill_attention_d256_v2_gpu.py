"""Prefill attention at head_dim 256 on the LDS-shared K/V kernel (4 waves, one per SIMD, the
wave pipelining its own QK behind the softmax) vs ``reference.prefill_attention`` in fp32 on the
CPU, at the op's tolerance. Every case asks for the kernel with HIPSERVE_PREFILL_ATTN_V1=0 and
checks that the launcher's own predicate (``prefill_attention_variant``) reports it."""
import functools
import math

import pytest
import torch

from hipserve.ops import KernelOps
from hipserve.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
D, TOL = 256, 2e-2
# (ctx, q_len): one row, a sub-tile that returns early, a chunk over a prefix, two host tiles,
# more than 16 key tiles (lazy rescale), a context end off the 64-key tile
SEQS = [(1, 1), (37, 37), (300, 50), (129, 129), (1100, 1100), (1500, 333)]
# limits: a 256-token block at rows [350, 606) of a 700-token prompt: it starts inside a 64-key
# tile and crosses the 128-row host tiles at 384 and 512; the window is shorter than its start
LIM_SEQS = [(700, 700), (37, 37)]
BLOCK, LIM_WINDOW = (350, 606), 300


@pytest.fixture(scope="module")
def ops():
    return KernelOps()


@functools.lru_cache(maxsize=None)
def _case(nq, nkv, bs, window, mode):
    """CPU inputs and the fp32 oracle of one case; mode: plain / cap (soft-capping 50 on scores
    scaled past it) / lim (per-row key limits). `differs`: the oracle with the cap or the limits
    moves off the plain one by more than the tolerance on most rows they touch."""
    seqs = LIM_SEQS if mode == "lim" else SEQS
    g = torch.Generator().manual_seed(17 + nq + 3 * nkv + bs)
    max_blocks = 1536 // bs
    n = len(seqs) * max_blocks
    kc = ref.to_cache(torch.randn(n, nkv, bs, D, generator=g), F8)
    vc = ref.to_cache(torch.randn(n, nkv, D, bs, generator=g), F8)
    bt = torch.randperm(n, generator=g).int().view(len(seqs), max_blocks).contiguous()
    cu, tiles, lim, touched = [0], [], [], []
    for i, (c, ql) in enumerate(seqs):
        tiles += [(i, r) for r in range(0, ql, 128)]
        cu.append(cu[-1] + ql)
        for p in range(c - ql, c):
            inb = mode == "lim" and i == 0 and BLOCK[0] <= p < BLOCK[1]
            lim.append(BLOCK[1] - 1 if inb else p)
            touched.append(inb and p < BLOCK[1] - 1 if mode == "lim" else p >= 1)
    q = (torch.randn(cu[-1], (nq + 2 * nkv) * D, generator=g) * (8.0 if mode == "cap" else 2.0)).bfloat16()
    cu_t, ctx_t = torch.tensor(cu, dtype=torch.int32), torch.tensor([c for c, _ in seqs], dtype=torch.int32)
    cap = 50.0 if mode == "cap" else 0.0
    limits = torch.tensor(lim, dtype=torch.int32) if mode == "lim" else None
    scale = 1.0 / math.sqrt(D)
    want = ref.prefill_attention(q, kc, vc, bt, cu_t, ctx_t, nq, nkv, scale, window, cap, limits)
    differs = 1.0
    if mode != "plain":
        plain = ref.prefill_attention(q, kc, vc, bt, cu_t, ctx_t, nq, nkv, scale, window)
        far = (want.float() - plain.float()).abs().amax((-2, -1)) > 10 * TOL
        differs = far[torch.tensor(touched)].float().mean().item()
    return (kc, vc, bt, cu_t, ctx_t, torch.tensor(tiles, dtype=torch.int32), q), limits, scale, cap, want, differs


CASES = [(nq, nkv, bs, w, "plain") for nq, nkv in [(8, 4), (4, 1), (16, 2)] for bs in (16, 32) for w in (0, 200)]
CASES += [(nq, nkv, 16, w, "cap") for nq, nkv in [(8, 4), (4, 1)] for w in (0, 200)]
CASES += [(nq, nkv, 16, w, "lim") for nq, nkv in [(8, 4), (4, 1)] for w in (0, LIM_WINDOW)]


@pytest.mark.parametrize("nq,nkv,bs,window,mode", CASES)
def test_prefill_attention_d256_shared(ops, monkeypatch, nq, nkv, bs, window, mode):
    """G = 2 (two heads x two row blocks), 4 (four heads) and 8 (two head groups per kv head) over
    an e4m3 cache and the same cache widened to bf16: both vs the oracle, equal to each other."""
    monkeypatch.setenv("HIPSERVE_PREFILL_ATTN_V1", "0")
    tensors, limits, scale, cap, want, differs = _case(nq, nkv, bs, window, mode)
    # 0.4 as in test_softcap_gpu.py / test_gemma3_vision_gpu.py: a row whose few visible keys stay
    # below the cap (or whose block adds little weight) need not move, most touched rows must
    assert differs >= 0.4, f"fixture does not discriminate: {differs:.2f}"
    kc, vc, bt, cu_t, ctx_t, tiles_t, q = (t.to(DEV) for t in tensors)
    assert torch.ops.hipserve.prefill_attention_variant(D, nq, nkv, bs, bt.stride(0)) == 2
    lim = None if limits is None else limits.to(DEV)
    T, outs = q.shape[0], []
    for k, v in ((kc, vc), (kc.to(torch.bfloat16), vc.to(torch.bfloat16))):
        out = torch.zeros(T, nq * D, device=DEV, dtype=torch.bfloat16)
        ops.prefill_attention(out, q, k, v, bt, cu_t, ctx_t, tiles_t, nq, nkv, scale, window, cap, lim)
        a, b = out.view(T, nq, D).float().cpu(), want.float()
        err = (a - b).abs()
        assert not (err > TOL + TOL * b.abs()).any(), f"max err {err.max().item()}"
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_prefill_attention_variant_fallbacks(ops, monkeypatch):
    variant = torch.ops.hipserve.prefill_attention_variant
    monkeypatch.setenv("HIPSERVE_PREFILL_ATTN_V1", "0")
    assert variant(256, 4, 4, 16, 96) == 1  # G = 1
    assert variant(256, 12, 4, 16, 96) == 1  # G = 3
    assert variant(256, 8, 4, 16, 1 << 20) == 1  # block ids past the LDS the ring leaves
    assert variant(128, 32, 8, 16, 96) == 2
    monkeypatch.setenv("HIPSERVE_PREFILL_ATTN_V1", "1")
    assert variant(256, 8, 4, 16, 96) == 1 and variant(128, 32, 8, 16, 96) == 1
