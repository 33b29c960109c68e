"""The wide bf16 decode GEMM (csrc/kernels/decode_gemm_wide.hip, 65-256 rows on the packed
weights): every (nw, mh) body against fp64, its GLU forms, the decoder forward with the wide
partials feeding the fused epilogues, and the tuner wiring."""
import math

import pytest
import torch
import torch.nn.functional as F

from hipserve.ops import KernelOps, gemm
from hipserve.ops import reference as ref

from .test_fused_decode_gpu import _small_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP = torch.ops.hipserve


@pytest.fixture(scope="module", autouse=True)  # loads the kernel library for every test
def ops():
    return KernelOps()


def _inputs(M, N, K, seed):
    """x as test_fp8_decode_gpu._x (row magnitudes over two decades), a column slice of a
    wider tensor (row stride K + 64); w [N, K] bf16."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.rand(M, K + 64, device=DEV, generator=g) * 2 - 1) * torch.logspace(-1, 1, M, device=DEV).unsqueeze(1)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.05
    return x.to(torch.bfloat16)[:, 32:32 + K], w.to(torch.bfloat16)


def _configs(M):
    return [(128, 1), (256, 1)] if M <= 128 else [(128, 2), (256, 2), (256, 1)]


def _max_split(K):
    return max(S for S in range(1, K // 128 + 1) if K % (128 * S) == 0 and K // (128 * S) in gemm.WIDE_STEPS)


@pytest.mark.parametrize("N,K", [(136, 256), (384, 1024), (1024, 1792), (512, 4096)])
@pytest.mark.parametrize("M", [65, 80, 128, 129, 200, 256])
def test_wide_gemm_vs_fp64(M, N, K):
    """Partials and bf16 out of every (nw, mh) at S = 1 and the largest S against
    x.double() @ w.double().T. Bounds from the arithmetic: fp32 accumulation of K products is
    within K 2^-24 (|x| |w|^T) elementwise; the bf16 output adds one rounding, 2^-8 |ref|."""
    x, w = _inputs(M, N, K, M * 7 + N + K)
    wp = gemm.pack(w)
    want = x.double() @ w.double().T
    bound = K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().T)
    for nw, mh in _configs(M):
        for S in (1, _max_split(K)):
            ws = torch.full((S, M, N), float("nan"), device=DEV)
            OP.decode_gemm_wide_partial(ws, x, wp, N, nw, mh, S)
            assert torch.isfinite(ws).all(), (nw, mh, S)
            err = (ws.double().sum(0) - want).abs()
            print(f"M {M} N {N} K {K} nw {nw} mh {mh} S {S}: partial err / bound {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), (nw, mh, S)
            wide = torch.full((M, N + 24), 7.0, device=DEV, dtype=torch.bfloat16)
            gemm.decode_gemm_wide(wide[:, :N], x, wp, N, nw, mh, S)
            assert (wide[:, N:] == 7.0).all(), (nw, mh, S)
            assert ((wide[:, :N].double() - want).abs() <= bound + 2.0 ** -8 * want.abs()).all(), (nw, mh, S)
            if S > 1:
                red = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
                OP.splitk_reduce(red, ws, S)
                assert torch.equal(wide[:, :N], red), (nw, mh, S)


@pytest.mark.parametrize("M", [65, 256])
def test_wide_glu_forms(ops, M):
    """GLU epilogue (S = 1) and GLU reduce (S = 2) of every (nw, mh). As the narrow kernel's
    test_glu_gemm_bit_exact: equal to the plain GEMM of that config + silu_and_mul, bit for bit.
    Against silu(bf16(g)) * bf16(u) of the fp64 product: g and u are each within the fp32
    accumulation bound plus one bf16 rounding (dg, du); |silu'| <= 1.1, so the product moves by
    at most 1.1 dg (|u| + du) + |silu(g)| du, plus the output's own rounding (2^-7 |ref| covers
    it on both sides)."""
    N, K = 512, 1024
    x, w = _inputs(M, N, K, M + 3)
    wp, wg = gemm.pack(w), gemm.pack(w, glu=True)
    gu = x.double() @ w.double().T
    acc = K * 2.0 ** -24 * (x.double().abs() @ w.double().abs().T) + 2.0 ** -8 * gu.abs()
    want = ref.silu_and_mul(gu.to(torch.bfloat16)).double()
    g, u, dg, du = gu[:, :N // 2], gu[:, N // 2:], acc[:, :N // 2], acc[:, N // 2:]
    bound = 1.1 * dg * (u.abs() + du) + F.silu(g).abs() * du + 2.0 ** -7 * want.abs()
    for nw, mh in _configs(M):
        for S in (1, 2):
            plain = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            gemm.decode_gemm_wide(plain, x, wp, N, nw, mh, S)
            chain = torch.empty(M, N // 2, device=DEV, dtype=torch.bfloat16)
            ops.silu_and_mul(chain, plain)
            act = gemm.gemm_glu(x, w, (nw, mh, S, wg))
            assert torch.equal(act, chain), (nw, mh, S)
            assert ((act.double() - want).abs() <= bound).all(), (nw, mh, S)
        ws = torch.empty(2, M, N, device=DEV)
        OP.decode_gemm_wide_partial(ws, x, wg, N, nw, mh, 2)
        red = torch.empty(M, N // 2, device=DEV, dtype=torch.bfloat16)
        OP.splitk_reduce_glu(red, ws, 2)
        assert torch.equal(act, red), (nw, mh)


@pytest.mark.parametrize("family,qkv_attn", [("llama", False), ("llama", True), ("gemma3", False)])
@pytest.mark.parametrize("B", [72, 200])
def test_wide_decode_forward_bit_exact(ops, B, family, qkv_attn):
    """Decode forward above 64 rows: wide GEMM + reduce + unfused tails vs the wide partials
    into the split-K epilogues (set-up of test_fused_decode_forward_bit_exact). qkv_attn: the
    qkv partials go straight into paged_decode_qkv, as the engine runs them."""
    from hipserve.models.llama import AttnMeta

    m, cfg = _small_model(ops, family=family)
    m.fused_qkv_attention = qkv_attn
    if qkv_attn:
        assert m.fused_qkv_attn_ok()
        m.decode_partition = 2048  # one context partition: the fused kernel's regime
    old = dict(gemm.TUNER.table)
    try:
        gemm.TUNER.table.clear()
        shapes = m.gemm_shapes()
        for (N, K) in shapes:
            for mm in gemm.WIDE_MS:
                gemm.TUNER.table[(mm, N, K)] = ("dgw", 256, 1, 2 if K >= 1024 else 1)
        m.pack_decode_weights(set(shapes))
        for lw in m.layers:  # the unfused path multiplies the plain packing of gate|up
            gemm.register_packed(lw.wgu)
        bs, D, nblk = 16, cfg.head_dim, 64
        ctx = torch.randint(1, 300, (B,), device=DEV, dtype=torch.int32)
        bt = torch.randperm(B * nblk, device=DEV).int().view(B, nblk)
        pos = (ctx - 1).long()
        slots = (bt.gather(1, (pos // bs).view(-1, 1).int()).view(-1).long() * bs + pos % bs)
        ids = torch.randint(0, cfg.vocab_size, (B,), device=DEV)
        kv1 = m.allocate_kv_cache(B * nblk, bs)
        for kc, vc in kv1:
            kc.normal_()
            vc.normal_()
        kv2 = [(k.clone(), v.clone()) for k, v in kv1]
        parts = math.ceil(nblk * bs / 512)
        mk = lambda: AttnMeta(num_prefill_tokens=0, num_decode=B, positions=pos, slot_mapping=slots,
                              bt_decode=bt, ctx_decode=ctx,
                              tmp_out=torch.empty(B, m.nq, parts, D, device=DEV),
                              tmp_ml=torch.empty(B, m.nq, parts, 2, device=DEV))
        assert gemm.fused_choice(B, m.layers[0].wo)[0][0] == "dgw"
        assert gemm.fused_choice(B, m.layers[0].wqkv)[0][0] == "dgw"
        if cfg.hidden_act == "silu":  # the GLU form must not fall back to linear() quietly
            assert gemm.glu_choice(B, m.layers[0].wgu) is not None
        m.fused_decode = False
        out1 = m.forward(ids, mk(), kv1).clone()
        m.fused_decode = True
        out2 = m.forward(ids, mk(), kv2).clone()
        assert torch.equal(out1, out2)
        for (k1, v1), (k2, v2) in zip(kv1, kv2):
            assert torch.equal(k1, k2) and torch.equal(v1, v2)
    finally:
        gemm.TUNER.table.clear()
        gemm.TUNER.table.update(old)


def test_wide_choice_wiring():
    N, K = 384, 1024
    x, w = _inputs(100, N, K, 5)
    x = x.contiguous()
    old = dict(gemm.TUNER.table)
    try:
        gemm.TUNER.table.clear()
        for mm in gemm.TUNE_MS:  # a table filled for the narrow rows only behaves as before
            gemm.TUNER.table[(mm, N, K)] = ("dgp", 1, 2)
        assert gemm.TUNER.choose(100, N, K) == "blas" and gemm.fused_choice(100, w) is None
        gemm.TUNER.table[(128, N, K)] = ("dgw", 128, 1, 2)
        wp = gemm.register_packed(w)
        fc = gemm.fused_choice(100, w)
        assert fc[0] == ("dgw", 128, 1, 2) and fc[1] is wp
        want = torch.empty(100, N, device=DEV, dtype=torch.bfloat16)
        gemm.decode_gemm_wide(want, x, wp, N, 128, 1, 2)
        assert torch.equal(gemm.linear(x, w), want)
    finally:
        gemm.TUNER.table.clear()
        gemm.TUNER.table.update(old)
