"""IQ4_NL / IQ4_XS on the GPU: the decode GEMM's bodies, the tiled -> bf16 dequantiser, the
expert GEMM, the range guard and the engines. The dense kernel checks are the ones
tests/test_gguf_gpu.py runs for the other block formats, called here with the two new ones
(same shapes, fp32 oracle and bound 1e-2 max|want| + 1e-3); the rest is written out below."""
import numpy as np
import pytest
import torch

from hipserve.weights import gguf as G

from . import test_gguf_gpu as dense_checks
from .test_gguf_moe_gpu import _file_cfg

pytestmark = pytest.mark.gpu
FORMATS = [G.IQ4_NL, G.IQ4_XS]
IDS = ["IQ4_NL", "IQ4_XS"]


@pytest.fixture(scope="module", autouse=True)
def _kernels():
    from hipserve.ops import load_library

    load_library()


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("M", [1, 16, 33, 64])
def test_decode_gemm_every_body(qt, M):
    """Parts of 512 / 80 / 272 rows, K = 2048: bf16 output and summed split-K partials vs fp32."""
    dense_checks.test_mfma_v2_formats(qt, M)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("S", [1, 2, 3, 5, 7, 11])
def test_m64_every_slice_length(qt, S):
    """K = 2816 (11 super-chunks), M = 64: NaN-filled partials come back finite and right."""
    dense_checks.test_mfma_v2_m64_every_slice_length(qt, S)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_tiled_to_bf16(qt):
    """dequantize(qw) on [48, 512] quantised normal weights: bit-exact against the numpy
    decode rounded once to bf16."""
    from hipserve.ops.quant import QuantWeight, dequantize

    dense_checks.test_dequant_exact(qt)
    w = dense_checks._mat(48, 512)
    want = torch.from_numpy(G.dequantize(G.quantize(w, qt), qt, w.size).reshape(48, 512)).to(torch.bfloat16)
    assert torch.equal(dequantize(QuantWeight.from_float(w, qt, "cuda")).cpu(), want)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_wide_body(qt):
    """N = 32768 + 144, K = 512, M = 33: the 256-row body."""
    dense_checks.test_qgemm_m64_wide_body(qt, 33)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_beyond_f16_activations(qt):
    dense_checks.test_mfma_v2_beyond_f16_range(qt, 16)


def test_mixed_projection_with_q6k():
    """IQ4_XS + Q6_K parts of one merged projection: two launches into one output, as
    split-K partials (S > 1) and as bf16 written by the kernel itself (S == 1)."""
    from hipserve.ops import quant as Q

    K = 2048
    qw, raws = dense_checks._rand_qw([(G.IQ4_XS, 512, K), (G.Q6_K, 256, K)], seed=7)
    assert qw.v2 and len(qw.groups) == 2
    x = torch.randn(8, K, device="cuda", dtype=torch.bfloat16)
    want = x.float() @ dense_checks._dense(raws).T
    tol = 1e-2 * want.abs().max().item() + 1e-3
    ws, S = Q.quant_partial(x, qw)
    assert S > 1 and (ws.view(S, 8, qw.N).sum(0) - want).abs().max().item() < tol
    assert (Q.quant_linear(x, qw).float() - want).abs().max().item() < tol
    old = Q.TARGET_WGS
    try:
        Q.TARGET_WGS = 1
        assert Q.v2_splits(qw, 8) == 1
        y1 = Q.quant_linear(x, qw).float()
    finally:
        Q.TARGET_WGS = old
    assert (y1 - want).abs().max().item() < tol


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_expert_gemm(qt, tile):
    """E = 4 experts [256, 512], 20 tokens routed top-2 over experts 0-2 (expert 3 empty), every
    slot tile, both expert layouts: bf16 output, 2-way split-K partials and the SiLU-GLU
    epilogue (gate = rows 0-127, up = rows 128-255) against an fp32 loop over the experts."""
    from hipserve.ops import quant as Q

    op = torch.ops.hipserve
    E, N, K, T, k = 4, 256, 512, 20, 2
    raw = Q.random_blocks(np.random.default_rng(qt + tile), qt, E * N, K)
    deq = torch.from_numpy(G.dequantize(raw, qt, E * N * K).reshape(E, N, K)).cuda()
    g = torch.Generator().manual_seed(tile)
    ids = torch.stack([torch.randperm(3, generator=g)[:k] for _ in range(T)]).int().cuda()
    cap = -(-(T * k + E * (tile - 1)) // tile) * tile
    slots, te = (torch.empty(n, dtype=torch.int32, device="cuda") for n in (cap, cap // tile))
    op.moe_align(ids, E, tile, slots, te, torch.empty(1, dtype=torch.int32, device="cuda"),
                 torch.empty(T * k, dtype=torch.int32, device="cuda"))
    real = slots >= 0
    pair = slots[real].long()
    assert int(real.sum()) == T * k
    x = torch.randn(T, K, device="cuda", dtype=torch.bfloat16)
    want = torch.full((T * k, N), float("nan"), device="cuda")
    for e in range(E):
        sel = ids.view(-1)[pair] == e
        want[sel] = x.float()[pair[sel] // k] @ deq[e].T
    assert not (ids == 3).any() and torch.isfinite(want).all()
    tol = 1e-2 * want.abs().max().item() + 1e-3
    wantg = torch.nn.functional.silu(want[:, :N // 2]) * want[:, N // 2:]
    f32, bf = torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.bfloat16, device="cuda")
    for kmajor in (False, True):
        w = Q.QuantMoE.from_blocks(raw.reshape(E, -1), qt, E, N, K, "cuda", kmajor=kmajor)
        assert w.kqt == Q.KERNEL_QT[qt] and w.q.shape == (E, N // 16 * (K // 256) * Q.CHUNK_BYTES[qt])
        out = torch.zeros(cap, N, device="cuda", dtype=torch.bfloat16)
        assert op.qmoe_gemm(out, f32, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, k, 1, kmajor) == 1
        assert (out[real].float() - want).abs().max().item() <= tol
        ws = torch.zeros(2, cap, N, device="cuda")
        assert op.qmoe_gemm(bf, ws, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, k, 2, kmajor) == 2
        assert (ws[:, real].sum(0) - want).abs().max().item() <= tol
        if tile <= 32:  # gate and up each within tol; silu is 1.1-Lipschitz, |silu(g)| <= |g|; two bf16 roundings
            act = torch.zeros(cap, N // 2, device="cuda", dtype=torch.bfloat16)
            op.qmoe_gemm(act, f32, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, k, 1, kmajor, 1)
            d = tol + 2.0 ** -8 * want.abs()
            bound = 1.1 * d[:, :N // 2] * (want[:, N // 2:].abs() + d[:, N // 2:]) + want[:, :N // 2].abs() * d[:, N // 2:]
            assert bool(((act[real].float() - wantg).abs() <= bound + 2.0 ** -7 * wantg.abs() + 1e-3).all())
        assert torch.equal(w.dequantize().float(), deq.to(torch.bfloat16).float())


def test_range_guard_hands_back_bf16(tmp_path):
    """An IQ4_XS tensor with one block whose |d (ls - 32)| lies past 65504 / 2^22: that merged
    projection loads as bf16 (there is no v1 kernel for the format) and still matches fp32."""
    from hipserve.ops import quant as Q

    N, K = 64, 512
    w = (np.random.default_rng(1).standard_normal((N, K)) * 0.05).astype(np.float32)
    p = str(tmp_path / "t.gguf")
    G.write_gguf(p, {"general.architecture": "llama"}, [("a.weight", w, G.IQ4_XS), ("ok.weight", w, G.IQ4_XS)])
    gf = G.GGUFFile(p)
    with open(p, "r+b") as f:  # block 5: d = 0.001, every ls = 0: |d (ls - 32)| = 0.032 > 0.0156
        f.seek(gf.data_offset + gf.tensors["a.weight"].offset + 5 * 136)
        f.write(np.float16(0.001).tobytes() + b"\0" * 6)
    gf = G.GGUFFile(p)
    assert not Q.sub_scale_ok(gf.raw("a.weight"), G.IQ4_XS) and Q.sub_scale_ok(gf.raw("ok.weight"), G.IQ4_XS)
    ok = Q.QuantWeight.from_gguf(gf, ["ok.weight"], "cuda")
    assert isinstance(ok, Q.QuantWeight) and ok.v2 and ok.parts[0].kqt == 15
    x = torch.randn(16, K, device="cuda", dtype=torch.bfloat16)
    for names in (["a.weight"], ["ok.weight", "a.weight"]):
        m = Q.QuantWeight.from_gguf(gf, names, "cuda")
        assert isinstance(m, torch.Tensor) and m.dtype == torch.bfloat16 and m.shape == (len(names) * N, K)
        want = x.float() @ torch.cat([torch.from_numpy(gf.tensor_f32(n)) for n in names]).cuda().T
        got = torch.nn.functional.linear(x, m).float()
        assert (got - want).abs().max().item() < 1e-2 * want.abs().max().item() + 1e-3


# ------------------------------------------------------------------ engines
PROMPTS = [[1, 5, 9, 33, 70, 100], list(range(3, 40))]


def _greedy(path, device):
    """(3 greedy tokens per prompt, the engine's model, the smallest top-2 logit margin over the
    sampled positions relative to that position's max |logit|) of the file on ``device``."""
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    cpu = device == "cpu"
    eng = LLMEngine(EngineConfig(model=path, device=device, load_format="gguf", max_num_seqs=4,
                                 max_num_batched_tokens=128, num_kv_blocks=64, max_model_len=256,
                                 **({"dtype": "float32"} if cpu else {})),
                    tp=TPGroup() if cpu else TPGroup(0, 1, None, torch.device("cuda", 0)))
    model, margins = eng.runner.model, []
    orig = model.compute_logits

    def cap(h):
        out = orig(h)
        top = out.float().topk(2, -1).values
        margins.append(((top[:, 0] - top[:, 1]) / out.float().abs().amax(-1)).min().item())
        return out

    model.compute_logits = cap
    res = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    eng.shutdown()
    return [r[0] for r in res], model, min(margins)


# The GPU engine (bf16 activations, f16 MFMA) must pick the CPU engine's (fp32) tokens. The
# suite bounds the logit difference between two loads of one file by 5e-2 max |logit|
# (test_gguf_q23_gpu.py, test_gguf_moe_gpu.py), so the files' seeds are the ones, of 60 tried on
# the CPU engine, whose top-2 margin exceeds that at every sampled position (asserted below:
# 0.095 / 0.064): no rounding inside the bound can flip a token, and no position is excluded.
MARGIN = 5e-2


def test_engine_llama_file_matches_cpu_engine(tmp_path, caplog):
    """small-llama: IQ4_XS projections, IQ4_NL attn_v, Q6_K output."""
    import logging

    from hipserve.config import PRESETS
    from hipserve.ops import quant as Q

    p = G.write_synthetic_llama_gguf(str(tmp_path / "m.gguf"), PRESETS["small-llama"], G.IQ4_XS, seed=35,
                                     tensor_types={"v": G.IQ4_NL, "output": G.Q6_K})
    want, _, margin = _greedy(p, "cpu")
    assert margin > MARGIN, margin
    with caplog.at_level(logging.INFO, logger="hipserve.weights.gguf"):
        got, m, _ = _greedy(p, "cuda")
    lw = m.layers[0]
    assert [[q.kqt for q in w.parts] for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd, m.lm_head)] == \
        [[15, 15, 14], [15], [15, 15], [15], [Q.KERNEL_QT[G.Q6_K]]]
    assert sum("IQ4_NL / IQ4_XS matrices and expert stacks kept as tiled blocks" in r.getMessage()
               for r in caplog.records) == 1
    assert got == want


def test_engine_qwen3moe_file_matches_cpu_engine(tmp_path):
    """A qwen3moe file, IQ4_XS throughout: the expert stacks stay IQ4_XS blocks (w13 k-major)."""
    from hipserve.ops import quant as Q

    p = G.write_synthetic_moe_gguf(str(tmp_path / "moe.gguf"), _file_cfg("qwen3moe"), "qwen3moe", qtype=G.IQ4_XS,
                                   seed=55)
    want, _, margin = _greedy(p, "cpu")
    assert margin > MARGIN, margin
    got, m, _ = _greedy(p, "cuda")
    for lw in m.layers:
        assert isinstance(lw.w13, Q.QuantMoE) and isinstance(lw.w2, Q.QuantMoE)
        assert (lw.w13.kqt, lw.w2.kqt, lw.w13.kmajor) == (15, 15, True) and lw.w13.dense is None
    assert got == want
