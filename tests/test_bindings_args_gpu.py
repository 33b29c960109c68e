"""The argument checks of csrc/torch_bindings.cpp: a tensor reaches a kernel only after its
device, dtype, layout and extent were checked. Every refusal here is a host-side check made
before any launch, and each refused call stands next to the same call with the offending
tensor repaired, which must go through (on the smallest legal shapes).

A missed check could do no harm either: host tensors are pinned (mapped into the GPU's address
space), short tensors are views of storage of the full size, and the ops that return before
launching at zero rows are called with zero rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
HIDDEN, T, B, NQ, NKV, D, BS, PART, V, N, K = 8, 2, 2, 1, 1, 64, 16, 128, 64, 128, 256
I32, I64, F32, F16, BF16 = torch.int32, torch.int64, torch.float32, torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def op():
    from hipserve.ops import load_library

    load_library()
    yield torch.ops.hipserve
    torch.cuda.synchronize()


def z(*shape, dtype=BF16):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def ones(*shape, dtype=BF16):
    return torch.ones(*shape, dtype=dtype, device="cuda")


def host(t):
    """The same tensor in pinned host memory."""
    return t.cpu().pin_memory()


def check(fn, args: dict, name: str, bad, op_name: str | None = None):
    """fn(**args) goes through; with args[name] = bad it is refused, naming the op and the argument."""
    op_name = op_name or fn.__name__.split(".")[-1]
    fn(**args)
    with pytest.raises(RuntimeError) as e:
        fn(**{**args, name: bad})
    msg = str(e.value)
    assert f"{op_name}: {name}" in msg, msg


def norm_args():
    return dict(out=z(T, HIDDEN), x=ones(T, HIDDEN), weight=ones(HIDDEN), eps=1e-5)


def kv_caches():
    return z(B, NKV, BS, D), z(B, NKV, D, BS)


def decode_args():
    kc, vc = kv_caches()
    return dict(out=z(B, NQ * D), q=ones(B, NQ * D), k_cache=kc, v_cache=vc,
                block_tables=torch.arange(B, dtype=I32, device="cuda").view(B, 1), context_lens=ones(B, dtype=I32),
                tmp_out=z(B, NQ, 1, D, dtype=F32), tmp_ml=z(B, NQ, 1, 2, dtype=F32), nq=NQ, nkv=NKV, part_size=PART,
                scale=0.125)


def sample_args():
    return dict(out_tok=z(B, dtype=I64), out_lp=z(B, dtype=F32), logits=torch.randn(B, V, device="cuda"),
                temperature=ones(B, dtype=F32), top_k=z(B, dtype=I32), top_p=ones(B, dtype=F32),
                seeds=ones(B, dtype=I64), steps=z(B, dtype=I64))


def combine_args():
    return dict(out=z(T, HIDDEN), y=ones(T, HIDDEN), w=ones(T, dtype=F32),
                pair_slot=torch.arange(T, dtype=I32, device="cuda"), k=1)


def splitk_norm_args():
    return dict(out=z(T, HIDDEN), residual=z(T, HIDDEN), ws=ones(T * HIDDEN, dtype=F32), splits=1, weight=ones(HIDDEN),
                eps=1e-5)


# ---- a host tensor among GPU tensors, one case per shared validator

def test_host_norm_weight(op):
    a = norm_args()
    check(op.rmsnorm, a, "weight", host(a["weight"]))


def test_host_rope_slots(op):
    kc, vc = kv_caches()
    a = dict(qkv=ones(T, (NQ + 2 * NKV) * D), positions=z(T, dtype=I64), slots=torch.arange(T, dtype=I64, device="cuda"),
             cos_sin=ones(4, D, dtype=F32), k_cache=kc, v_cache=vc, nq=NQ, nkv=NKV, head_dim=D, mode=0)
    check(op.rope_cache, a, "slots", host(a["slots"]))


@pytest.mark.parametrize("name", ["context_lens", "block_tables"])
def test_host_decode_tables(op, name):
    a = decode_args()
    check(op.paged_decode, a, name, host(a[name]))


def test_host_sample_top_k(op):
    a = sample_args()
    check(op.sample, a, "top_k", host(a["top_k"]))


def test_host_splitk_ws_zero_rows(op):
    a = dict(out=z(0, N), ws=z(N, dtype=F32), splits=1)
    check(op.splitk_reduce, a, "ws", host(a["ws"]))


def test_host_x_f16_pairs_rsc_zero_rows(op):
    a = dict(x16=z(0, K, dtype=F16), rsc=z(1, dtype=F32), x=z(0, K))
    check(op.x_f16_pairs, a, "rsc", host(a["rsc"]))


def test_host_gguf_prefill_rsc_zero_rows(op):
    from hipserve.ops import quant

    f = next(f for f in quant.FORMATS if f.prefill)
    q = z(N // 16 * (K // 256) * f.chunk_bytes, dtype=torch.uint8)
    a = dict(out=z(0, N), x16=z(0, K, dtype=F16), rsc=z(1, dtype=F32), qs=[q], qtypes=[f.kqt], rows=[N], cols=[0], K=K,
             epi=0)
    check(op.gguf_prefill, a, "rsc", host(a["rsc"]))


def test_host_moe_pair_slot(op):
    a = combine_args()
    check(op.moe_combine, a, "pair_slot", host(a["pair_slot"]))


def test_host_decode_gemm_ws(op):
    a = dict(ws=z(T * N, dtype=F32), x=ones(T, K), w=ones(N, K), N=N, rt=1, splits=1, packed=False)
    check(op.decode_gemm_partial, a, "ws", host(a["ws"]))


def test_host_penalty_pres(op):
    a = dict(logits=torch.randn(B, V, device="cuda"), slot=torch.arange(B, dtype=I32, device="cuda"),
             pres=z(B, dtype=F32), freq=z(B, dtype=F32), rep=ones(B, dtype=F32), counts=z(B, V, dtype=I32),
             seen=z(B, (V + 31) // 32, dtype=I32))
    check(op.penalty_apply, a, "pres", host(a["pres"]))


# ---- wrong dtype

def test_fused_add_rmsnorm_f16_weight(op):
    a = dict(norm_args(), residual=z(T, HIDDEN))
    check(op.fused_add_rmsnorm, a, "weight", ones(HIDDEN, dtype=F16))


def test_moe_combine_int64_pair_slot(op):
    a = combine_args()
    check(op.moe_combine, a, "pair_slot", a["pair_slot"].long())


def test_splitk_add_rmsnorm_bf16_ws(op):
    a = splitk_norm_args()
    check(op.splitk_add_rmsnorm, a, "ws", ones(T * HIDDEN))


# ---- short extents: views of storage that is large enough

@pytest.mark.parametrize("name", ["tmp_out", "block_tables", "context_lens"])
def test_paged_decode_short(op, name):
    a = decode_args()
    check(op.paged_decode, a, name, a[name][: B - 1])


def test_sample_short_out_lp(op):
    a = sample_args()
    check(op.sample, a, "out_lp", a["out_lp"][: B - 1])


def test_prefill_attention_narrow_out(op):
    kc, vc = kv_caches()
    a = dict(out=z(T, NQ * D), q=ones(T, NQ * D), k_cache=kc, v_cache=vc,
             block_tables=torch.arange(B, dtype=I32, device="cuda").view(B, 1),
             cu_q=torch.arange(B + 1, dtype=I32, device="cuda"), ctx_lens=ones(B, dtype=I32),
             tiles=torch.tensor([[0, 0], [1, 0]], dtype=I32, device="cuda"), nq=NQ, nkv=NKV, scale=0.125)
    check(op.prefill_attention, a, "out", a["out"][:, : NQ * D - 8])
