"""The boundaries of the tiled ops' format dispatch (csrc/include/hipserve/quant_formats.h):
ids outside the table, FP8B (no expert body) in the expert GEMM, Q2_K (no prefill body) in
the block prefill GEMM. Every refusal is a host-side argument check made before any launch,
so no kernel runs here; the tensors only have to be GPU tensors of the right sizes."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N, K, M_PREFILL = 128, 256, 65


@pytest.fixture(scope="module")
def Q():
    from hipserve.ops import load_library, quant

    load_library()
    return quant


def _calls(kqt: int, chunk_bytes: int) -> dict:
    """The four tiled ops on one [N, K] part (one expert) of kernel format ``kqt``, M = 1."""
    op = torch.ops.hipserve

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    q, rs = z(N // 16 * (K // 256) * chunk_bytes, dtype=torch.uint8), z(N, dtype=torch.float32)
    x, ws = z(1, K), z(0, dtype=torch.float32)
    x16, rsc = z(M_PREFILL, K, dtype=torch.float16), z(M_PREFILL, dtype=torch.float32)
    slots, tile_expert = z(16, dtype=torch.int32), z(1, dtype=torch.int32)
    return {
        "gguf_gemm_parts": lambda: op.gguf_gemm_parts(z(1, N), ws, x, [q], [rs], [kqt], [N], [0], N, K, 1),
        "gguf_prefill": lambda: op.gguf_prefill(z(M_PREFILL, N), x16, rsc, [q], [kqt], [N], [0], K, 0),
        "qmoe_gemm": lambda: op.qmoe_gemm(z(16, N), ws, x, q.view(1, -1), rs.view(1, N), kqt, N, K, slots,
                                          tile_expert, 16, 1, 1),
        "gguf_dequant_tiled": lambda: op.gguf_dequant_tiled(z(N, K), q, rs, kqt, N, K),
    }


@pytest.mark.parametrize("kqt", [-1, 13])
@pytest.mark.parametrize("name", ["gguf_gemm_parts", "gguf_prefill", "qmoe_gemm", "gguf_dequant_tiled"])
def test_unknown_id_raises(Q, name, kqt):
    assert kqt not in Q.BY_KQT
    with pytest.raises(RuntimeError, match=f"{name}: kernel qtype {kqt} "):
        _calls(kqt, 4096)[name]()


def test_fp8b_has_no_expert_body(Q):
    f = Q.BY_KQT[Q.KERNEL_QT[Q.FP8B]]
    assert not f.moe
    with pytest.raises(RuntimeError, match=f"qmoe_gemm: kernel qtype {f.kqt} "):
        _calls(f.kqt, f.chunk_bytes)["qmoe_gemm"]()


def test_q2k_has_no_prefill_body(Q):
    f = Q.BY_KQT[Q.KERNEL_QT[Q.G.Q2_K]]
    assert not f.prefill
    assert _calls(f.kqt, f.chunk_bytes)["gguf_prefill"]() is False


def test_expert_formats_supported(Q):
    for f in Q.FORMATS:
        assert Q.QuantMoE.supported(f.kqt, N, K) == f.moe, f.name
    assert not Q.QuantMoE.supported(Q.KERNEL_QT[Q.FP8B], N, K)
