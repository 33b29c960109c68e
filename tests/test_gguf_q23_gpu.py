"""Q2_K / Q3_K on the GPU, dense side: the decode GEMM's bodies, the tiled -> bf16
dequantiser, the range guard and the engines. The kernel checks are the ones
tests/test_gguf_gpu.py runs for the other block formats, called here with the two new
ones (same shapes, oracle and bounds); what those do not cover (mixes with Q4_K, the bf16
hand-back, engines on files of the new formats) is written out below."""
import numpy as np
import pytest
import torch

from hipserve.weights import gguf as G

from . import test_gguf_gpu as dense_checks

pytestmark = pytest.mark.gpu
FORMATS = [G.Q2_K, G.Q3_K]
IDS = [G.TYPE_NAMES[t] for t in FORMATS]


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


@pytest.mark.parametrize("specs", [[(G.Q3_K, 1024, 4096), (G.Q3_K, 256, 4096), (G.Q4_K, 256, 4096)],
                                   [(G.Q2_K, 512, 2048), (G.Q3_K, 256, 2048)]], ids=["q3k+q4k", "q2k+q3k"])
def test_mixed_projection(specs):
    """A merged projection of two formats: two launches into one output, direct bf16 (S == 1)
    and split-K partials."""
    from hipserve.ops import quant as Q

    qw, raws = dense_checks._rand_qw(specs, seed=7)
    assert qw.v2 and len(qw.groups) == 2
    K = specs[0][2]
    x = torch.randn(8, K, device="cuda", dtype=torch.bfloat16)
    want = x.float() @ dense_checks._dense(raws).T
    tol = 1e-2 * want.abs().max().item() + 1e-3
    assert Q.v2_splits(qw, 8) > 1
    ws, S = Q.quant_partial(x, qw)
    assert S > 1 and (ws.view(S, 8, qw.N).sum(0) - want).abs().max().item() < tol
    assert (Q.quant_linear(x, qw).float() - want).abs().max().item() < tol
    old = Q.TARGET_WGS
    try:
        Q.TARGET_WGS = 1  # forces S == 1: bf16 written by the kernel itself
        assert Q.v2_splits(qw, 8) == 1
        y1 = Q.quant_linear(x, qw).float()
    finally:
        Q.TARGET_WGS = old
    assert (y1 - want).abs().max().item() < tol


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_x16_staging_is_bit_identical(qt):
    dense_checks.test_x16_staging_matches_conversion(qt)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
@pytest.mark.parametrize("M", [16, 64])
def test_beyond_f16_activations(qt, M):
    dense_checks.test_mfma_v2_beyond_f16_range(qt, M)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_wide_body(qt):
    """N = 32768 + 144, K = 512, M = 33: the 256-row body."""
    dense_checks.test_qgemm_m64_wide_body(qt, 33)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_tiled_to_bf16(qt):
    """dequantize(qw) vs the numpy decode rounded to bf16 on [48, 512] (quantised normal
    weights), and a prefill-sized batch (M = 200: no block prefill GEMM for these formats)."""
    from hipserve.ops import quant as Q

    dense_checks.test_dequant_exact(qt)
    qw, raws = dense_checks._rand_qw([(qt, 320, 1024)], seed=qt)
    assert not Q.qprefill_ok(qw, 200, timed=False) and not Q.qprefill_ok(qw, 1024, timed=False)
    x = torch.randn(200, 1024, device="cuda", dtype=torch.bfloat16)
    want = x.float() @ dense_checks._dense(raws).T
    tol = 1e-2 * want.abs().max().item() + 1e-3
    assert (Q.quant_linear(x, qw).float() - want).abs().max().item() < tol
    assert (Q.quant_linear_dequant(x, qw).float() - want).abs().max().item() < tol
    # no resident bf16 shadow unless asked for, like the other GGUF formats
    assert Q.make_dense_shadows([qw], "cuda", 0, gguf=False) == 0 and qw.dense is None


def test_range_guard_hands_back_bf16(tmp_path):
    """A Q3_K tensor with one block whose d * 31 lies past 65504 / 2^17: sub_scale_ok is
    false and from_gguf yields a bf16 matrix (there is no v1 kernel for the format) that
    still matches fp32; so does a tensor whose rows are no multiple of 16."""
    from hipserve.ops import quant as Q

    N, K = 64, 512
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    p = str(tmp_path / "t.gguf")
    G.write_gguf(p, {"general.architecture": "llama"}, [("a.weight", w, G.Q3_K), ("odd.weight", w[:40], G.Q3_K),
                                                        ("ok.weight", w, G.Q3_K)])
    gf = G.GGUFFile(p)
    t = gf.tensors["a.weight"]
    with open(p, "r+b") as f:  # block 5: every scale 63 (s - 32 = 31), d = 0.02: 0.62 > 0.4998
        f.seek(gf.data_offset + t.offset + 5 * 110 + 96)
        f.write(b"\xff" * 12 + np.float16(0.02).tobytes())
    gf = G.GGUFFile(p)
    assert not Q.sub_scale_ok(gf.raw("a.weight"), G.Q3_K) and Q.sub_scale_ok(gf.raw("ok.weight"), G.Q3_K)
    x = torch.randn(16, K, device="cuda", dtype=torch.bfloat16)
    for name, rows in (("a.weight", N), ("odd.weight", 40)):
        m = Q.QuantWeight.from_gguf(gf, [name], "cuda")
        assert isinstance(m, torch.Tensor) and m.dtype == torch.bfloat16 and m.shape == (rows, K)
        want = x.float() @ torch.from_numpy(gf.tensor_f32(name)).cuda().T
        got = torch.nn.functional.linear(x, m).float()
        assert (got - want).abs().max().item() < 1e-2 * want.abs().max().item() + 1e-3
    ok = Q.QuantWeight.from_gguf(gf, ["ok.weight"], "cuda")
    assert isinstance(ok, Q.QuantWeight) and ok.v2 and ok.parts[0].kqt == Q.KERNEL_QT[G.Q3_K]
    # a merged projection with one such tensor is bf16 as a whole
    both = Q.QuantWeight.from_gguf(gf, ["ok.weight", "a.weight"], "cuda")
    assert isinstance(both, torch.Tensor) and both.shape == (2 * N, K)


# ------------------------------------------------------------------ engines
PROMPTS = [[1, 5, 9, 33, 70, 100], list(range(3, 40)), [7] * 12]


def _run_engine(path, eager=False):
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    eng = LLMEngine(EngineConfig(model=path, device="cuda", load_format="gguf", max_num_seqs=4,
                                 max_num_batched_tokens=128, num_kv_blocks=64, max_model_len=256,
                                 enforce_eager=eager),
                    tp=TPGroup(0, 1, None, torch.device("cuda", 0)))
    mm = eng.runner.model
    logits = []
    orig = mm.compute_logits

    def cap(h):
        out = orig(h)
        logits.append(out.float().cpu().clone())
        return out

    mm.compute_logits = cap
    res = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True))
    stats = dict(eng.runner.stats)
    layer0 = mm.layers[0]
    # the part formats of each quantised matrix; None where it is held dense
    kinds = {n: ([p.kqt for p in w.parts] if hasattr(w, "parts") else None)
             for n, w in (("wqkv", layer0.wqkv), ("wo", layer0.wo), ("wgu", layer0.wgu), ("wd", layer0.wd),
                          ("lm_head", mm.lm_head), ("embed", mm.embed))}
    eng.shutdown()
    return [r[0] for r in res], torch.cat(logits), kinds, stats


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_engine_llama_file_graph_vs_eager_and_bf16(tmp_path, monkeypatch, caplog, qt):
    """A small-llama file, every matrix and token_embd in the format: the layers hold
    QuantWeights of the new kernel format, hipGraph decode == eager decode token for token,
    and the logits agree with the same file held as bf16 (HIPSERVE_GGUF_Q23_NATIVE=0)."""
    import logging

    from hipserve.config import PRESETS
    from hipserve.ops import quant as Q

    p = G.write_synthetic_llama_gguf(str(tmp_path / "m.gguf"), PRESETS["small-llama"], qt, embd_type=qt, seed=4)
    kqt = Q.KERNEL_QT[qt]
    monkeypatch.setenv("HIPSERVE_GGUF_Q23_NATIVE", "1")
    with caplog.at_level(logging.INFO, logger="hipserve.weights.gguf"):
        toks_g, logits_g, kinds, stats_g = _run_engine(p)
    assert kinds == {"wqkv": [kqt] * 3, "wo": [kqt], "wgu": [kqt] * 2, "wd": [kqt], "lm_head": [kqt],
                     "embed": None}  # token_embd: decoded by numpy into the bf16 table
    assert sum("kept as tiled blocks" in r.getMessage() for r in caplog.records) == 1
    assert stats_g["graph_steps"] > 0 and all(len(t) == 4 for t in toks_g)
    toks_e, _, _, stats_e = _run_engine(p, eager=True)
    assert stats_e["graph_steps"] == 0 and toks_g == toks_e
    monkeypatch.setenv("HIPSERVE_GGUF_Q23_NATIVE", "0")
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="hipserve.weights.gguf"):
        _, logits_d, kinds_d, _ = _run_engine(p)
    assert all(v is None for v in kinds_d.values())
    assert sum("HIPSERVE_GGUF_Q23_NATIVE=0" in r.getMessage() for r in caplog.records) == 1
    a, b = logits_g, logits_d
    assert a.shape == b.shape and torch.isfinite(a).all()
    diff, agree = (a - b).abs().max().item(), (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    print(f"{G.TYPE_NAMES[qt]} native vs bf16: max |dlogit| {diff:.4e} (|logit| max {b.abs().max().item():.3f}), "
          f"argmax agreement {agree:.3f}")
    assert diff < 5e-2 * b.abs().max().item() + 1e-3
    assert agree >= 0.85


def test_engine_phi3_fused_projections(tmp_path):
    """A phi3-arch file (fused attn_qkv, ffn_up = [gate; up]) in Q3_K with Q2_K ffn_down: each
    fused tensor is one tiled part of the new format, and the engine generates."""
    from hipserve.config import PRESETS
    from hipserve.ops import quant as Q

    cfg = PRESETS["small-llama"]
    H, I, D, nq, nkv, V = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim, cfg.num_heads, cfg.num_kv_heads, \
        cfg.vocab_size
    rng = np.random.default_rng(8)

    def r(*s):
        return (rng.standard_normal(s) * 0.05).astype(np.float32)

    toks = ["<unk>", "<s>", "</s>"] + [f"<0x{b:02X}>" for b in range(256)] + [f"▁w{i}" for i in range(V - 259)]
    md = {"general.architecture": "phi3", "general.name": "phi3-q3k", "phi3.context_length": 2048,
          "phi3.embedding_length": H, "phi3.block_count": 2, "phi3.feed_forward_length": I,
          "phi3.attention.head_count": nq, "phi3.attention.head_count_kv": nkv, "phi3.attention.key_length": D,
          "phi3.rope.freq_base": 10000.0, "phi3.rope.dimension_count": D,
          "phi3.attention.layer_norm_rms_epsilon": 1e-5, "tokenizer.ggml.model": "llama",
          "tokenizer.ggml.tokens": toks, "tokenizer.ggml.scores": [float(-i) for i in range(V)],
          "tokenizer.ggml.token_type": [3 if i < 3 else (6 if i < 259 else 1) for i in range(V)],
          "tokenizer.ggml.bos_token_id": 1, "tokenizer.ggml.eos_token_id": 2}
    t = [("token_embd.weight", r(V, H), G.Q3_K), ("output_norm.weight", 1 + r(H), G.F32),
         ("output.weight", r(V, H), G.Q6_K)]
    for i in range(2):
        b = f"blk.{i}."
        t += [(b + "attn_norm.weight", 1 + r(H), G.F32), (b + "ffn_norm.weight", 1 + r(H), G.F32),
              (b + "attn_qkv.weight", r((nq + 2 * nkv) * D, H), G.Q3_K), (b + "attn_output.weight", r(H, nq * D), G.Q3_K),
              (b + "ffn_up.weight", r(2 * I, H), G.Q3_K), (b + "ffn_down.weight", r(H, I), G.Q2_K)]
    p = str(tmp_path / "phi3.gguf")
    G.write_gguf(p, md, t)
    toks_g, logits, kinds, stats = _run_engine(p)
    k2, k3 = Q.KERNEL_QT[G.Q2_K], Q.KERNEL_QT[G.Q3_K]
    assert kinds == {"wqkv": [k3], "wo": [k3], "wgu": [k3], "wd": [k2], "lm_head": [Q.KERNEL_QT[G.Q6_K]], "embed": None}
    assert all(len(x) == 4 and all(0 <= v < V for v in x) for x in toks_g)
    assert torch.isfinite(logits).all() and stats["graph_steps"] > 0


def test_synthetic_q3_k_m_engine():
    """--quantization q3_k_m: q|k|v of layer 0 is Q3_K, Q3_K, Q4_K; 10 tokens, the same for
    identical prompts."""
    from hipserve.config import PRESETS, EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.ops.quant import QuantWeight
    from hipserve.parallel.comm import TPGroup

    cfg = PRESETS["small-llama"]
    eng = LLMEngine(EngineConfig(model="small-llama", load_format="dummy", device="cuda", num_kv_blocks=256,
                                 max_model_len=1024, max_num_batched_tokens=256, max_num_seqs=8,
                                 extra={"quantization": "q3_k_m"}),
                    tp=TPGroup(0, 1, None, torch.device("cuda", 0)), model_cfg=cfg)
    m = eng.runner.model
    assert isinstance(m.layers[0].wqkv, QuantWeight) and m.cfg.rope_mode == 1
    assert [p.qtype for p in m.layers[0].wqkv.parts] == [G.Q3_K, G.Q3_K, G.Q4_K]
    assert [p.qtype for p in m.layers[0].wgu.parts] == [G.Q3_K, G.Q3_K] and m.layers[0].wd.parts[0].qtype == G.Q4_K
    res = eng.generate([[1] + list(range(300, 400)), [1, 5, 6]] * 3,
                       SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True))
    eng.shutdown()
    assert all(len(r[0]) == 10 for r in res)
    assert res[0][0] == res[2][0] == res[4][0]
