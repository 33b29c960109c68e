"""Q2_K / Q3_K expert stacks on the GPU: the expert GEMM checks of
tests/test_gguf_moe_gpu.py (fp32 oracle, bit-identity with the dense kernel, GLU epilogue,
both expert layouts, untouched padding slots, split-K) run for the two formats, and the
engine on ``qwen3moe`` files and synthetic models whose experts use them."""
import pytest
import torch

from hipserve.weights import gguf as G

from . import test_gguf_moe_gpu as moe_checks

pytestmark = pytest.mark.gpu
FORMATS = [G.Q2_K, G.Q3_K]
IDS = [G.TYPE_NAMES[t] for t in FORMATS]


@pytest.fixture(scope="module", autouse=True)
def _kernels():
    from hipserve.ops import load_library

    load_library()


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("P,tile", [(6, 16), (48, 32), (160, 64)])
def test_expert_gemm(qt, P, tile):
    """E = 4, N = 288, K = 768, every slot tile: the five checks."""
    moe_checks.test_qmoe_gemm_gguf_formats(qt, P, tile)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("kmajor", [False, True])
def test_expert_gemm_split_k(qt, kmajor):
    moe_checks.test_qmoe_gemm_gguf_split_k(qt, kmajor)


def test_engine_qwen3moe_q23_experts_vs_bf16(tmp_path, monkeypatch):
    """A ``qwen3moe`` file whose layers hold (Q3_K, Q3_K, Q4_K) and (Q2_K, Q2_K, Q3_K) experts:
    they load as QuantMoE stacks of those formats, the engine generates through hipGraph
    decode, and the logits agree with the experts dequantised to bf16 at load."""
    from hipserve.ops import quant as Q

    p = G.write_synthetic_moe_gguf(str(tmp_path / "moe-q23.gguf"), moe_checks._file_cfg("qwen3moe"), "qwen3moe",
                                   mixed_k=True, seed=5,
                                   expert_types={0: (G.Q3_K, G.Q3_K, G.Q4_K), 1: (G.Q2_K, G.Q2_K, G.Q3_K)})
    monkeypatch.setenv("HIPSERVE_GGUF_Q23_NATIVE", "1")
    toks, logits, kqts, stats = moe_checks._run_engine(p, monkeypatch=monkeypatch)
    K = Q.KERNEL_QT
    assert kqts == [(K[G.Q3_K], K[G.Q4_K]), (K[G.Q2_K], K[G.Q3_K])]
    assert all(len(t) == 4 and all(0 <= x < 512 for x in t) for t in toks)
    assert torch.isfinite(logits).all() and stats["graph_steps"] > 0
    _, logits_d, _, _ = moe_checks._run_engine(p, native=False, monkeypatch=monkeypatch)
    a, b = logits, logits_d
    assert a.shape == b.shape
    diff, agree = (a - b).abs().max().item(), (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    print(f"native vs bf16 experts: max |dlogit| {diff:.4e} (|logit| max {b.abs().max().item():.3f}), "
          f"argmax agreement {agree:.3f}")
    assert diff < 5e-2 * b.abs().max().item() + 1e-3
    assert agree >= 0.85
    # HIPSERVE_GGUF_Q23_NATIVE=0 alone also sends both layers' experts to bf16
    monkeypatch.setenv("HIPSERVE_GGUF_Q23_NATIVE", "0")
    # (_run_engine asserts that no layer holds block experts)
    _, logits_0, kqts_0, _ = moe_checks._run_engine(p, monkeypatch=monkeypatch, block_layers=set())
    assert kqts_0 == [] and logits_0.shape == logits_d.shape and torch.isfinite(logits_0).all()


@pytest.mark.parametrize("scheme,want", [("q3_k_m", (G.Q3_K, G.Q4_K)), ("q2_k", (G.Q2_K, G.Q3_K))])
def test_allocate_random_quant_moe(scheme, want):
    """Synthetic MoE weights of the two schemes: w13 / w2 block stacks of the scheme's formats."""
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import KernelOps
    from hipserve.ops import quant as Q
    from hipserve.parallel.comm import TPGroup

    cfg = moe_checks._file_cfg("qwen3moe")
    m = LlamaModel(cfg, TPGroup(0, 1, None, torch.device("cuda")), "cuda", torch.bfloat16, KernelOps())
    m.allocate_random_quant(scheme)
    for lw in m.layers:
        assert isinstance(lw.w13, Q.QuantMoE) and isinstance(lw.w2, Q.QuantMoE) and lw.wgu is None
        assert (lw.w13.kqt, lw.w2.kqt) == tuple(Q.KERNEL_QT[t] for t in want)
        assert lw.w13.kmajor and not lw.w2.kmajor and lw.w13.shape == (8, 512, 512) and lw.w2.shape == (8, 512, 256)
