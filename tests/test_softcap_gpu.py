"""Logit soft-capping (Gemma-2) on the gfx950 kernels: ``cap * tanh(s / cap)`` on the attention
scores of paged decode (bf16 / e4m3 caches, one and several partitions), its fused-qkv form
and both prefill kernels, and ``logit_softcap_`` on the final logits. Oracle: the fp32
reference ops with the cap applied before the masks; tolerance atol = rtol = 2e-2 as in
test_kernels_gpu.py / test_attention_d256_gpu.py.

With unit-normal q / k and Gemma's cap of 50 the capped and uncapped outputs differ by less
than the tolerance, so a kernel that ignored the cap would pass. The inputs are therefore two
sets, (a) softcap 2 with q scaled by 2 and (b) softcap 50 with q scaled by 24, and every test
first asserts on the CPU that its fixture discriminates: the oracle with the cap and the
oracle without it differ by more than 10 x the tolerance (0.2) somewhere in at least 40 % of
the rows (sequence or token, head) that see more than one key. Inputs are drawn on the CPU
(one seed base, chosen so that this holds for every case below)."""
import functools
import math

import pytest
import torch

from hipserve.ops import KernelOps
from hipserve.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
TOL = 2e-2
SETS = {"a": (2.0, 2.0), "b": (50.0, 24.0)}  # name -> (softcap, q scale)
# one below / at / above the 32- and 64-key chunks and the 512-key partition, and several partitions
CTX = [1, 17, 100, 600, 1300, 33, 63, 64, 65, 511, 512, 513]
MAX_BLOCKS = 96
BS = 16
SEQS = [(1, 1), (37, 37), (300, 50), (129, 129), (1100, 1100), (1500, 333)]  # (context, new tokens)
SEED = 103


@pytest.fixture(scope="module")
def ops():
    return KernelOps()


def _close(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    bad = (a - b).abs() > (TOL + TOL * b.abs())
    assert not bad.any(), f"max err {(a - b).abs().max().item()}"


def _discriminates(capped, plain, rows):
    """Fraction of the rows [.., heads] (mask ``rows``) whose capped and uncapped oracle
    outputs differ by more than 10 x the tolerance."""
    far = ((capped.float() - plain.float()).abs().amax(-1) > 10 * TOL)[rows]
    return far.float().mean().item()


@functools.lru_cache(maxsize=None)
def _decode_case(D, nq, nkv, window, f8, sname):
    """CPU inputs and the two fp32 oracles (capped, uncapped) of one decode case, shared by
    the partition sizes."""
    cap, qs = SETS[sname]
    g = torch.Generator().manual_seed(SEED + nq + 3 * nkv + D)
    B, nblocks = len(CTX), len(CTX) * MAX_BLOCKS
    kc = torch.randn(nblocks, nkv, BS, D, generator=g)
    vc = torch.randn(nblocks, nkv, D, BS, generator=g)
    kc, vc = (ref.to_cache(kc, F8), ref.to_cache(vc, F8)) if f8 else (kc.bfloat16(), vc.bfloat16())
    bt = torch.randperm(nblocks, generator=g).int().view(B, MAX_BLOCKS).contiguous()
    cl = torch.tensor(CTX, dtype=torch.int32)
    q = (torch.randn(B, (nq + 2 * nkv) * D, generator=g) * qs).bfloat16()
    scale = 1.0 / math.sqrt(D)
    want = ref.paged_decode(q, kc, vc, bt, cl, nq, nkv, scale, window, cap)
    plain = ref.paged_decode(q, kc, vc, bt, cl, nq, nkv, scale, window, 0.0)
    frac = _discriminates(want, plain, cl > 1)
    return (kc, vc, bt, cl, q), scale, cap, want, frac


def _run_decode(ops, tensors, D, nq, nkv, part, scale, window, *cap):
    kc, vc, bt, cl, q = (t.to(DEV) for t in tensors)
    B = len(CTX)
    max_parts = math.ceil(MAX_BLOCKS * BS / part)
    tmp_out = torch.empty(B, nq, max_parts, D, device=DEV, dtype=torch.float32)
    tmp_ml = torch.empty(B, nq, max_parts, 2, device=DEV, dtype=torch.float32)
    out = torch.zeros(B, nq * D, device=DEV, dtype=torch.bfloat16)
    ops.paged_decode(out, q, kc, vc, bt, cl, tmp_out, tmp_ml, nq, nkv, part, scale, window, None, *cap)
    return out


@pytest.mark.parametrize("sname", ["a", "b"])
@pytest.mark.parametrize("window", [0, 100])
@pytest.mark.parametrize("part", [512, 2048])
@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("nq,nkv", [(8, 4), (16, 8), (4, 1)])
@pytest.mark.parametrize("D", [64, 96, 128, 256])
def test_paged_decode_softcap(ops, D, nq, nkv, f8, part, window, sname):
    """Every head size, bf16 and e4m3 caches (the 64-key e4m3 chunks at 64 / 128 / 256), one
    partition and several with the merge, ragged contexts and a window (masks applied after
    the cap: a capped mask value would be a live score of -cap), vs the fp32 oracle."""
    tensors, scale, cap, want, frac = _decode_case(D, nq, nkv, window, f8, sname)
    assert frac >= 0.4, f"fixture does not discriminate: {frac:.2f}"
    out = _run_decode(ops, tensors, D, nq, nkv, part, scale, window, cap)
    _close(out.view(len(CTX), nq, D), want)


@pytest.mark.parametrize("f8", [False, True])
@pytest.mark.parametrize("D", [128, 256])
def test_paged_decode_softcap_zero_is_the_uncapped_kernel(ops, D, f8):
    """softcap = 0.0 passed explicitly == the call without the argument, bit for bit."""
    tensors, scale, _cap, _want, _ = _decode_case(D, 8, 4, 100, f8, "a")
    for part in (512, 2048):
        a = _run_decode(ops, tensors, D, 8, 4, part, scale, 100)
        b = _run_decode(ops, tensors, D, 8, 4, part, scale, 100, 0.0)
        assert torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _prefill_case(D, nq, nkv, window, sname):
    cap, qs = SETS[sname]
    g = torch.Generator().manual_seed(SEED + 1 + nq + nkv + D)
    max_blocks = 1536 // BS
    n = len(SEQS) * max_blocks
    kc = ref.to_cache(torch.randn(n, nkv, BS, D, generator=g), F8)
    vc = ref.to_cache(torch.randn(n, nkv, D, BS, generator=g), F8)
    bt = torch.randperm(n, generator=g).int().view(len(SEQS), max_blocks).contiguous()
    cu, tiles, multi = [0], [], []
    for i, (c, ql) in enumerate(SEQS):
        tiles += [(i, r) for r in range(0, ql, 128)]
        cu.append(cu[-1] + ql)
        multi += [p >= 1 for p in range(c - ql, c)]  # rows that see more than one key
    q = (torch.randn(cu[-1], (nq + 2 * nkv) * D, generator=g) * qs).bfloat16()
    cu_t = torch.tensor(cu, dtype=torch.int32)
    ctx_t = torch.tensor([c for c, _ in SEQS], dtype=torch.int32)
    tiles_t = torch.tensor(tiles, dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    want = ref.prefill_attention(q, kc, vc, bt, cu_t, ctx_t, nq, nkv, scale, window, cap)
    plain = ref.prefill_attention(q, kc, vc, bt, cu_t, ctx_t, nq, nkv, scale, window, 0.0)
    frac = _discriminates(want, plain, torch.tensor(multi))
    return (kc, vc, bt, cu_t, ctx_t, tiles_t, q), scale, cap, want, frac


# head_dim 128 with a GQA group of 2 / 4 runs v2 (its deferred rescale: running max and
# exponent of the CAPPED score), a group of 1 and the other head sizes run v1
@pytest.mark.parametrize("sname", ["a", "b"])
@pytest.mark.parametrize("window", [0, 200])
@pytest.mark.parametrize("D,nq,nkv", [(128, 8, 4), (128, 4, 1), (128, 4, 4), (256, 8, 4), (256, 4, 1), (64, 8, 4),
                                      (96, 8, 4)])
def test_prefill_attention_softcap(ops, D, nq, nkv, window, sname):
    """Whole prompts, chunks over a cached prefix and several key tiles over an e4m3 cache and
    over the same cache widened to bf16: both vs the fp32 oracle, and equal to each other."""
    tensors, scale, cap, want, frac = _prefill_case(D, nq, nkv, window, sname)
    assert frac >= 0.4, f"fixture does not discriminate: {frac:.2f}"
    kc, vc, bt, cu_t, ctx_t, tiles_t, q = (t.to(DEV) for t in tensors)
    T = q.shape[0]
    outs = []
    for k, v in ((kc, vc), (kc.to(torch.bfloat16), vc.to(torch.bfloat16))):
        out = torch.zeros(T, nq * D, device=DEV, dtype=torch.bfloat16)
        ops.prefill_attention(out, q, k, v, bt, cu_t, ctx_t, tiles_t, nq, nkv, scale, window, cap)
        _close(out.view(T, nq, D), want)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("S,part", [(1, 512), (3, 256)])
def test_paged_decode_qkv_softcap_bit_exact(ops, S, part, qk_norm):
    """paged_decode_qkv(..., softcap) == splitk_rope_cache + paged_decode(..., softcap), bit
    for bit (output and both caches), one partition and several; the cap changes the output."""
    D, B, nq, nkv, cap = 128, 9, 16, 4, 0.5
    g = torch.Generator(device=DEV).manual_seed(31 + S)
    nw = (torch.rand(D, device=DEV, generator=g) + 0.5, torch.rand(D, device=DEV, generator=g) + 0.5) \
        if qk_norm else (None, None)
    N = (nq + 2 * nkv) * D
    ws = torch.randn(S, B, N, device=DEV, generator=g) * (2.0 / math.sqrt(S))  # scores ~ N(0, 2^2): far past the cap
    nblk = 40
    ctx = torch.randint(1, nblk * BS, (B,), device=DEV, dtype=torch.int32, generator=g)
    ctx[0] = 1
    ctx[1] = nblk * BS
    bt = torch.randperm(B * nblk, device=DEV, generator=g).int().view(B, nblk)
    pos = (ctx - 1).long()
    slots = bt.gather(1, (pos // BS).view(-1, 1)).view(-1).long() * BS + pos % BS
    slots[4] = -1
    cs = ref.rope_cos_sin(D, 4096, 10000.0).to(DEV)
    kc1 = torch.randn(B * nblk, nkv, BS, D, device=DEV, generator=g).to(torch.bfloat16)
    vc1 = torch.randn(B * nblk, nkv, D, BS, device=DEV, generator=g).to(torch.bfloat16)
    kc2, vc2 = kc1.clone(), vc1.clone()
    parts = math.ceil(nblk * BS / part)
    mk = lambda: (torch.empty(B, nq, parts, D, device=DEV), torch.empty(B, nq, parts, 2, device=DEV))  # noqa: E731
    scale = D ** -0.5
    qkv = torch.zeros(B, N, device=DEV, dtype=torch.bfloat16)
    torch.ops.hipserve.splitk_rope_cache(qkv, ws, S, pos, slots, cs, kc1, vc1, nq, nkv, D, 0, None, nw[0], nw[1], 1e-6)
    out1, out0, out2 = (torch.empty(B, nq * D, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    ops.paged_decode(out1, qkv, kc1, vc1, bt, ctx, *mk(), nq, nkv, part, scale, 0, None, cap)
    ops.paged_decode(out0, qkv, kc1, vc1, bt, ctx, *mk(), nq, nkv, part, scale)
    torch.ops.hipserve.paged_decode_qkv(out2, ws, S, pos, slots, cs, kc2, vc2, bt, ctx, *mk(), nq, nkv, part, scale,
                                        0, 0, None, nw[0], nw[1], 1e-6, cap)
    assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
    assert torch.equal(out1, out2)
    with pytest.raises(AssertionError):  # the capped output is not the uncapped one within the kernel tolerance
        _close(out1, out0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [1000, 32003])
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_logit_softcap(ops, rows, V, dtype):
    """In place on a column slice of a wider padded buffer (row stride > V, V no multiple of
    the 8-wide thread tile), values out to 3 x the cap so both tails saturate; the columns
    past V keep their sentinel. Tolerance vs fp32 cap * tanh(x / cap): one bf16 ulp at
    magnitude cap for bf16 storage, cap * 1e-5 for fp32."""
    cap, sentinel = 30.0, 7.0
    g = torch.Generator().manual_seed(V + rows)
    width = (V + 127) // 128 * 128 + 64
    buf = torch.full((rows, width), sentinel, dtype=dtype)
    buf[:, :V] = ((torch.rand(rows, V, generator=g) * 2 - 1) * 3 * cap).to(dtype)
    want = torch.tanh(buf[:, :V].float() / cap) * cap
    assert (want.abs() > cap * 0.99).any() and (want.abs() < 1.0).any()
    dbuf = buf.to(DEV)
    ops.logit_softcap_(dbuf[:, :V], cap)
    got = dbuf.cpu()
    assert (got[:, V:] == sentinel).all()
    tol = cap * 2.0 ** -8 if dtype == torch.bfloat16 else cap * 1e-5
    err = (got[:, :V].float() - want).abs().max().item()
    assert err <= tol, err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_logit_softcap_saturates_finite(ops, dtype):
    """Magnitudes of 1e4 (exp overflows / underflows inside the tanh) give exactly +-cap, not
    NaN or inf; the op replays from a captured graph."""
    cap = 30.0
    x = torch.tensor([[1e4, -1e4, 0.0, 3e38, -3e38, 88.0, -88.0, 1e-30]], dtype=torch.float32).to(dtype).to(DEV)
    want = (torch.tanh(x.float() / cap) * cap).cpu()
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.logit_softcap_(static.clone(), cap)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.logit_softcap_(static, cap)
    static.copy_(x)
    graph.replay()
    eager = ops.logit_softcap_(x.clone(), cap)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager[0, :2].float().cpu(), torch.tensor([cap, -cap]))
    assert torch.equal(static, eager)
    assert (eager.float().cpu() - want).abs().max().item() <= cap * 2.0 ** -8
