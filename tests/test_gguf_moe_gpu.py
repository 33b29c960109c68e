"""GGUF-block MoE experts on the GPU: the expert GEMM (``qmoe_gemm``, gguf_mfma.hip MoE
mode) on Q4_0 / Q4_1 / Q8_0 / Q4_K / Q5_K / Q6_K expert stacks against the numpy block
decoders in fp32 and, bit for bit, against the dense decode kernel, its GLU epilogue and
its two expert layouts; the f16-range second pass; the MoE layer on Q4_K + Q6_K experts
(decode, prefill, hipGraph); and the engine on synthetic ``qwen3moe`` / Mixtral-style
GGUF files."""
import numpy as np
import pytest
import torch

from hipserve.weights import gguf as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = [G.Q4_0, G.Q4_1, G.Q8_0, G.Q4_K, G.Q5_K, G.Q6_K]
SENTINEL = 777.0  # exactly representable in bf16 and fp32: what padding rows must still hold


@pytest.fixture(scope="module", autouse=True)
def _kernels():
    from hipserve.ops import load_library

    load_library()


def _experts(qt, E, N, K, seed, kmajor=False):
    """(QuantMoE of random valid blocks, their fp32 decode [E, N, K], the raw blocks [E, bytes])."""
    from hipserve.ops import quant as Q

    raw = Q.random_blocks(np.random.default_rng(seed), qt, E * N, K)
    deq = torch.from_numpy(G.dequantize(raw, qt, E * N * K).reshape(E, N, K)).to(DEV)
    return Q.QuantMoE.from_blocks(raw, qt, E, N, K, DEV, kmajor=kmajor), deq, raw.reshape(E, -1)


def _routing(P, E, tile, k, seed):
    """Pair -> expert ids [P / k, k]: expert 0 takes three quarters of the pairs (more than
    a tile once P allows), the last expert none, one expert a single pair; and the
    expert-sorted slot table of moe_align."""
    n0 = 3 * P // 4
    flat = torch.cat([torch.zeros(n0), torch.full((1,), E - 2), torch.ones(P - n0 - 1)]).int()
    g = torch.Generator().manual_seed(seed)
    ids = flat[torch.randperm(P, generator=g)].view(P // k, k).contiguous().to(DEV)
    cap = -(-(P + E * (tile - 1)) // tile) * tile
    slots = torch.empty(cap, dtype=torch.int32, device=DEV)
    te = torch.empty(cap // tile, dtype=torch.int32, device=DEV)
    nt = torch.empty(1, dtype=torch.int32, device=DEV)
    ps = torch.empty(P, dtype=torch.int32, device=DEV)
    torch.ops.hipserve.moe_align(ids, E, tile, slots, te, nt, ps)
    counts = torch.bincount(ids.view(-1).long(), minlength=E).tolist()
    assert counts[E - 1] == 0 and counts[E - 2] == 1 and (P <= tile or counts[0] > tile)
    return ids, slots, te, cap


@pytest.mark.parametrize("qt", FORMATS, ids=lambda t: G.TYPE_NAMES[t])
@pytest.mark.parametrize("P,tile", [(6, 16), (48, 32), (160, 64)])
def test_qmoe_gemm_gguf_formats(qt, P, tile):
    """w13-like expert GEMM per format and slot tile: (a) fp32 oracle, (b) bit-identical to
    the dense decode kernel on the expert's own tiled part, (c) GLU epilogue == bf16
    gate|up then silu_and_mul, (d) k-major == row-group-major, (e) padding slots untouched."""
    from hipserve.ops import quant as Q

    op = torch.ops.hipserve
    E, N, K, k = 4, 288, 768, 2
    w, deq, raw = _experts(qt, E, N, K, seed=qt * 100 + tile)
    wk, _, _ = _experts(qt, E, N, K, seed=qt * 100 + tile, kmajor=True)
    assert w.kqt == Q.KERNEL_QT[qt] and w.rs.numel() == 0 and not w.kmajor and wk.kmajor
    assert w.q.shape == (E, N // 16 * (K // 256) * Q.CHUNK_BYTES[qt])
    ids, slots, te, cap = _routing(P, E, tile, k, seed=P)
    T = P // k
    x = torch.randn(T, K, device=DEV, dtype=torch.bfloat16)
    f32 = torch.empty(0, dtype=torch.float32, device=DEV)
    real = slots >= 0
    pair = slots[real].long()
    tok, exp = pair // k, ids.view(-1)[pair].long()
    assert int(real.sum()) == P

    out = torch.full((cap, N), SENTINEL, device=DEV, dtype=torch.bfloat16)
    assert op.qmoe_gemm(out, f32, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, k, 1) == 1
    # (a) fp32 oracle on the numpy-decoded blocks
    want = torch.einsum("pk,pnk->pn", x.float()[tok], deq[exp])
    tol = 1e-2 * want.abs().max().item() + 1e-3
    err = (out[real].float() - want).abs().max().item()
    print(f"{G.TYPE_NAMES[qt]} tile {tile}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # (e) padding slots are never written
    assert bool((out[~real] == SENTINEL).all())
    # (b) the dense kernel (same body, K loop and fragments) on expert e's part, S = 1
    dense = []
    for e in range(E):
        qw = Q.QuantWeight.from_raw([(qt, N, K, raw[e])], DEV)
        assert qw.v2
        y = torch.empty(T, N, device=DEV, dtype=torch.bfloat16)
        Q._launch_v2(y, f32, x, qw, 1)
        dense.append(y)
    dense = torch.stack(dense)
    assert torch.equal(out[real], dense[exp, tok])
    # (d) k-major experts: the same sums in the same order
    outk = torch.full((cap, N), SENTINEL, device=DEV, dtype=torch.bfloat16)
    op.qmoe_gemm(outk, f32, x, wk.q, wk.rs, wk.kqt, N, K, slots, te, tile, k, 1, True)
    assert torch.equal(outk, out)
    # the dequantised stack of either layout == the block decoders, rounded once to bf16
    d0, dk = w.dequantize(), wk.dequantize()
    assert torch.equal(d0, dk)
    assert (d0.float() - deq).abs().max().item() <= 2 ** -8 * deq.abs().max().item()
    # (c) GLU epilogue (16- and 32-slot bodies), both layouts; SiLU and GELU
    if tile <= 32:
        for glu, act_op in ((1, op.silu_and_mul), (2, op.gelu_and_mul)):
            wantg = torch.full((cap, N // 2), SENTINEL, device=DEV, dtype=torch.bfloat16)
            act_op(wantg, out)
            for ww in (w, wk):
                act = torch.full((cap, N // 2), SENTINEL, device=DEV, dtype=torch.bfloat16)
                op.qmoe_gemm(act, f32, x, ww.q, ww.rs, ww.kqt, N, K, slots, te, tile, k, 1, ww.kmajor, glu)
                assert torch.equal(act[real], wantg[real]), (glu, ww.kmajor)
                assert bool((act[~real] == SENTINEL).all())


@pytest.mark.parametrize("qt", FORMATS, ids=lambda t: G.TYPE_NAMES[t])
@pytest.mark.parametrize("kmajor", [False, True])
def test_qmoe_gemm_gguf_split_k(qt, kmajor):
    """w2-like expert GEMM (x rows = slots, N = 272, K = 512) with 2 K splits through the
    fp32 partial workspace, every slot tile."""
    op = torch.ops.hipserve
    E, N, K, k = 4, 272, 512, 2
    w, deq, _ = _experts(qt, E, N, K, seed=qt + 7, kmajor=kmajor)
    for P, tile in ((6, 16), (48, 32), (160, 64)):
        ids, slots, te, cap = _routing(P, E, tile, k, seed=P + 1)
        real = slots >= 0
        exp = ids.view(-1)[slots[real].long()].long()
        x = torch.randn(cap, K, device=DEV, dtype=torch.bfloat16)
        ws = torch.full((2, cap, N), SENTINEL, device=DEV, dtype=torch.float32)
        out = torch.empty(0, device=DEV, dtype=torch.bfloat16)
        assert op.qmoe_gemm(out, ws, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, 0, 2, kmajor) == 2
        want = torch.einsum("pk,pnk->pn", x.float()[real], deq[exp])
        tol = 1e-2 * want.abs().max().item() + 1e-3
        err = (ws[:, real].sum(0) - want).abs().max().item()
        assert err <= tol, (tile, err, tol)
        # each split is its own K half
        half = torch.einsum("pk,pnk->pn", x.float()[real][:, :256], deq[exp][:, :, :256])
        assert (ws[0, real] - half).abs().max().item() <= tol
        assert bool((ws[:, ~real] == SENTINEL).all())


def test_qmoe_gemm_gguf_beyond_f16_range():
    """One token row with |x| up to 3e6 (beyond f16) in a 16-slot tile of Q4_K experts: the
    pre-scaled second pass keeps every row finite and within the fp32 bound, row by row."""
    op = torch.ops.hipserve
    E, N, K, k, P, tile = 4, 288, 768, 2, 6, 16
    w, deq, _ = _experts(G.Q4_K, E, N, K, seed=11, kmajor=True)
    ids, slots, te, cap = _routing(P, E, tile, k, seed=3)
    x = torch.randn(P // k, K, device=DEV)
    x[1] *= 3e6 / x[1].abs().max()
    x = x.to(torch.bfloat16)
    assert x.float().abs().max().item() > 2e6
    real = slots >= 0
    pair = slots[real].long()
    tok, exp = pair // k, ids.view(-1)[pair].long()
    f32 = torch.empty(0, dtype=torch.float32, device=DEV)
    want = torch.einsum("pk,pnk->pn", x.float()[tok], deq[exp])
    for glu in (0, 1):
        out = torch.full((cap, N // 2 if glu else N), SENTINEL, device=DEV, dtype=torch.bfloat16)
        op.qmoe_gemm(out, f32, x, w.q, w.rs, w.kqt, N, K, slots, te, tile, k, 1, True, glu)
        got = out[real].float()
        assert torch.isfinite(got).all()
        rowmax = want.abs().amax(1, keepdim=True)
        if glu:
            # silu(gate) * up of the fp32 oracle, row by row. Bound from the parts: gate and up
            # each carry the GEMM bound (a) of their row plus one bf16 rounding (2^-8 relative),
            # silu is 1.1-Lipschitz and |silu(g)| <= |g|, and the product is rounded to bf16 once
            # more: |d(s u)| <= 1.1 dg (|u| + du) + |g| du + 2^-8 |s u| (doubled to 2^-7 below
            # for the rounding of the slightly different product). A wrong power-of-two
            # un-scale of the big row would miss it by orders of magnitude.
            g_, u_ = want[:, :N // 2], want[:, N // 2:]
            dg = 1e-2 * rowmax + 1e-3 + 2.0 ** -8 * g_.abs()
            du = 1e-2 * rowmax + 1e-3 + 2.0 ** -8 * u_.abs()
            wantg = torch.nn.functional.silu(g_) * u_
            tol = 1.1 * dg * (u_.abs() + du) + g_.abs() * du + 2.0 ** -7 * wantg.abs() + 1e-3
            assert bool(((got - wantg).abs() <= tol).all()), ((got - wantg).abs() / tol).max().item()
            assert wantg[tok == 1].abs().max().item() > 1e6  # the big row's products are far past f16
            assert bool((out[~real] == SENTINEL).all())
            continue
        assert bool(((got - want).abs() <= 1e-2 * rowmax + 1e-3).all())
        assert (got - want).abs().max().item() <= 1e-2 * want.abs().max().item() + 1e-3
        assert bool((out[~real] == SENTINEL).all())


# ------------------------------------------------------------------ layer level
def _moe_model(H, I, E, k):
    from hipserve.config import PRESETS
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import KernelOps
    from hipserve.parallel.comm import TPGroup

    cfg = PRESETS["tiny-mixtral"].replace(hidden_size=H, intermediate_size=I, num_experts=E, num_experts_per_tok=k)
    return LlamaModel(cfg, TPGroup(0, 1, None, torch.device(DEV)), DEV, torch.bfloat16, KernelOps())


def _layer(H, I, E, seed):
    from hipserve.models.llama import LayerWeights

    torch.manual_seed(seed)
    router = torch.randn(E, H, device=DEV, dtype=torch.bfloat16) * 0.3
    w13, d13, _ = _experts(G.Q4_K, E, 2 * I, H, seed, kmajor=True)
    w2, d2, _ = _experts(G.Q6_K, E, H, I, seed + 1)
    return LayerWeights(ln1=None, wqkv=None, wo=None, ln2=None, router=router, w13=w13, w2=w2), d13, d2


def _moe_fp32(x, router, d13, d2, k, I):
    T, H = x.shape
    logits = torch.nn.functional.linear(x, router).float()
    wts, idx = torch.topk(torch.softmax(logits, -1), k, -1)
    wts = wts / wts.sum(-1, keepdim=True)
    want = torch.zeros(T, H, device=DEV)
    xf = x.float()
    for e in range(d13.shape[0]):
        rows, slot = (idx == e).nonzero(as_tuple=True)
        if rows.numel() == 0:
            continue
        gu = xf[rows] @ d13[e].T
        act = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        want.index_add_(0, rows, (act @ d2[e].T) * wts[rows, slot].unsqueeze(-1))
    return want


@pytest.mark.parametrize("T,E,k,I", [(6, 8, 2, 768), (200, 8, 2, 512)])
def test_gguf_moe_layer_vs_fp32(T, E, k, I):
    """Q4_K w13 + Q6_K w2 experts through ``MoEMixin.moe`` (16- and 64-slot tiles) against
    the fp32 routed computation on the decoded blocks; the call captures into a hipGraph
    whose replay equals the eager output."""
    H = 512
    m = _moe_model(H, I, E, k)
    assert m._decode_tile(T * k) == (16 if T == 6 else 64)
    lw, d13, d2 = _layer(H, I, E, T + E + I)
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    got = m.moe(x, lw).float()
    want = _moe_fp32(x, lw.router, d13, d2, k, I)
    err = (got - want).abs().max().item()
    assert err <= 3e-2 * want.abs().max().item() + 1e-3, err
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.moe(x, lw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = m.moe(x, lw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g.float(), got)


@pytest.mark.parametrize("packed", [False, True])
def test_gguf_moe_layer_prefill_paths_vs_fp32(packed):
    """Prefill-sized routing of GGUF experts: the row-major dequantised scratch with the
    streaming expert kernel (``MOE_PACKED_PREFILL = "0"``) and the dequantised + packed
    scratch with the grouped GEMM (``"1"``), both against fp32."""
    from hipserve.models import llama as L
    from hipserve.ops import gemm
    from hipserve.ops import quant as Q

    H, I, E, k = 512, 512, 16, 4
    T = L.MOE_KERNEL_MAX_PAIRS // k + 300
    m = _moe_model(H, I, E, k)
    m.MOE_PACKED_PREFILL = "1" if packed else "0"
    lw, d13, d2 = _layer(H, I, E, 7)
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    got = m.moe(x, lw).float()
    want = _moe_fp32(x, lw.router, d13, d2, k, I)
    err = (got - want).abs().max().item()
    assert err <= 3e-2 * want.abs().max().item() + 1e-3, err
    if packed:  # the packed dequant equals packing the row-major dequant, bit for bit
        p13 = Q.moe_packed_scratch(lw.w13, 0, True).clone()
        p2 = Q.moe_packed_scratch(lw.w2, 1, False).clone()
        d13r, d2r = Q.moe_dense(lw.w13, 0), Q.moe_dense(lw.w2, 1)
        for e in range(E):
            assert torch.equal(p13[e], gemm.pack(d13r[e].contiguous(), glu=True))
            assert torch.equal(p2[e], gemm.pack(d2r[e].contiguous()))


# ------------------------------------------------------------------ engine
def _file_cfg(arch):
    from hipserve.config import PRESETS

    return PRESETS["small-mixtral"].replace(
        name=f"synthetic-{arch}", num_layers=2, hidden_size=512, num_heads=8, num_kv_heads=2, head_dim=64,
        intermediate_size=1024 if arch == "qwen3moe" else 256, moe_intermediate_size=256 if arch == "qwen3moe" else 0,
        num_experts=8, num_experts_per_tok=2, vocab_size=512, max_position_embeddings=2048, rope_theta=1e6,
        qk_norm=arch == "qwen3moe")


PROMPTS = [[1, 5, 9, 33, 70, 100], list(range(3, 40)), [7] * 12]


def _run_engine(path, eager=False, native=True, monkeypatch=None, block_layers=None):
    """(greedy tokens per prompt, captured logits, (w13.kqt, w2.kqt) per block layer, runner
    stats). ``block_layers``: the layers expected to hold block experts (default: all when
    ``native``, none otherwise)."""
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.ops import quant as Q
    from hipserve.parallel.comm import TPGroup

    if monkeypatch is not None:
        monkeypatch.setenv("HIPSERVE_GGUF_MOE_NATIVE", "1" if native else "0")
    eng = LLMEngine(EngineConfig(model=path, device="cuda", load_format="gguf", max_num_seqs=4,
                                 max_num_batched_tokens=128, num_kv_blocks=64, max_model_len=256,
                                 enforce_eager=eager),
                    tp=TPGroup(0, 1, None, torch.device("cuda", 0)))
    mm = eng.runner.model
    kqts = []
    for li, lw in enumerate(mm.layers):
        blocks = native and (block_layers is None or li in block_layers)
        assert isinstance(lw.w13, Q.QuantMoE) == blocks and isinstance(lw.w2, Q.QuantMoE) == blocks, li
        assert lw.wgu is None and lw.wd is None and lw.router.dtype == torch.bfloat16
        if blocks:
            assert lw.w13.dense is None and lw.w2.dense is None  # resident as blocks only
            kqts.append((lw.w13.kqt, lw.w2.kqt))
        else:  # bf16 experts: row-major, or already replaced by their packed copy
            assert lw.w13 is None or (lw.w13.dtype == torch.bfloat16 and lw.w13.shape == (8, 512, 512))
    logits = []
    orig = mm.compute_logits

    def cap(h):
        out = orig(h)
        logits.append(out.float().cpu().clone())
        return out

    mm.compute_logits = cap
    res = eng.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True))
    stats = dict(eng.runner.stats)
    eng.shutdown()
    return [r[0] for r in res], torch.cat(logits), kqts, stats


@pytest.fixture(scope="module")
def qwen3moe_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("gguf_moe") / "qwen3moe-q4km.gguf"
    return G.write_synthetic_moe_gguf(str(p), _file_cfg("qwen3moe"), "qwen3moe", mixed_k=True, seed=1)


def test_engine_qwen3moe_q4km_graph_vs_eager_and_bf16_fallback(qwen3moe_file, monkeypatch):
    """A Q4_K_M-mix ``qwen3moe`` file: experts load as Q4_K / Q6_K ``QuantMoE`` stacks,
    hipGraph decode == eager decode token for token, and the block experts agree with the
    same file's experts dequantised to bf16 at load (HIPSERVE_GGUF_MOE_NATIVE=0) within the
    two bounds of test_quant_moe_gpu.py::test_int8_expert_checkpoint_native."""
    from hipserve.ops import quant as Q

    toks_g, logits_g, kqts, stats_g = _run_engine(qwen3moe_file, eager=False, monkeypatch=monkeypatch)
    assert kqts == [(Q.KERNEL_QT[G.Q4_K], Q.KERNEL_QT[G.Q6_K])] * 2
    assert stats_g["graph_steps"] > 0
    toks_e, _, _, stats_e = _run_engine(qwen3moe_file, eager=True, monkeypatch=monkeypatch)
    assert stats_e["graph_steps"] == 0
    assert toks_g == toks_e
    _, logits_d, _, _ = _run_engine(qwen3moe_file, eager=False, native=False, monkeypatch=monkeypatch)
    a, b = logits_g, logits_d
    assert a.shape == b.shape
    diff, agree = (a - b).abs().max().item(), (a.argmax(-1) == b.argmax(-1)).float().mean().item()
    print(f"native vs bf16 experts: max |dlogit| {diff:.4e} (|logit| max {b.abs().max().item():.3f}), argmax agreement {agree:.3f}")
    assert diff < 5e-2 * b.abs().max().item() + 1e-3
    assert agree >= 0.85


def test_engine_mixtral_style_gguf(tmp_path, monkeypatch):
    """A llama-arch (Mixtral-style) MoE file, Q8_0 throughout, loads as block experts and generates."""
    from hipserve.ops import quant as Q

    p = G.write_synthetic_moe_gguf(str(tmp_path / "mixtral-q8.gguf"), _file_cfg("llama"), "llama", qtype=G.Q8_0, seed=2)
    toks, logits, kqts, stats = _run_engine(p, monkeypatch=monkeypatch)
    assert kqts == [(Q.KERNEL_QT[G.Q8_0],) * 2] * 2
    assert all(len(t) == 4 and all(0 <= x < 512 for x in t) for t in toks)
    assert torch.isfinite(logits).all() and stats["graph_steps"] > 0


def test_engine_layers_that_fall_back_to_bf16(tmp_path, monkeypatch, caplog):
    """One file, three layers: Q4_K / Q6_K experts (blocks), Q4_K gate|up with Q5_0 down (no
    Q5_0 kernel) and Q4_K gate with Q5_K up (formats differ). The two odd layers get bf16
    experts for BOTH stacks, each with one log line naming the tensor and the reason; the
    engine serves the mix through hipGraph decode, and agrees with the all-bf16 load of the
    same file within the bounds of the native-vs-bf16 test above."""
    import logging

    from hipserve.ops import quant as Q

    cfg = _file_cfg("qwen3moe").replace(num_layers=3)
    p = G.write_synthetic_moe_gguf(str(tmp_path / "mixed.gguf"), cfg, "qwen3moe", mixed_k=True, seed=3,
                                   expert_types={1: (G.Q4_K, G.Q4_K, G.Q5_0), 2: (G.Q4_K, G.Q5_K, G.Q6_K)})
    with caplog.at_level(logging.INFO, logger="hipserve.weights.gguf"):
        toks, logits, kqts, stats = _run_engine(p, monkeypatch=monkeypatch, block_layers={0})
    msgs = [r.getMessage() for r in caplog.records if "dequantised" in r.getMessage()]
    assert len(msgs) == 2, msgs
    assert "blk.1.ffn_down_exps.weight" in msgs[0] and "Q5_0" in msgs[0] and "no expert kernel" in msgs[0]
    assert "blk.2.ffn_gate_exps.weight" in msgs[1] and "differ in format" in msgs[1] and "Q5_K" in msgs[1]
    assert kqts == [(Q.KERNEL_QT[G.Q4_K], Q.KERNEL_QT[G.Q6_K])]
    assert all(len(t) == 4 for t in toks) and torch.isfinite(logits).all() and stats["graph_steps"] > 0
    _, logits_d, _, _ = _run_engine(p, native=False, monkeypatch=monkeypatch)
    assert logits.shape == logits_d.shape
    assert (logits - logits_d).abs().max().item() < 5e-2 * logits_d.abs().max().item() + 1e-3
    assert (logits.argmax(-1) == logits_d.argmax(-1)).float().mean().item() >= 0.85


def test_allocate_random_quant_moe_on_gpu():
    """Synthetic Q4_K_M MoE weights on the GPU: Q4_K w13 (k-major) and Q6_K w2 block stacks in
    every layer, each layer with its own bytes, served by the MoE layer."""
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import KernelOps
    from hipserve.ops import quant as Q
    from hipserve.parallel.comm import TPGroup

    cfg = _file_cfg("qwen3moe").replace(num_layers=3)
    m = LlamaModel(cfg, TPGroup(0, 1, None, torch.device(DEV)), DEV, torch.bfloat16, KernelOps())
    m.allocate_random_quant("q4_k_m")
    for lw in m.layers:
        assert isinstance(lw.w13, Q.QuantMoE) and isinstance(lw.w2, Q.QuantMoE) and lw.wgu is None
        assert (lw.w13.kqt, lw.w2.kqt) == (Q.KERNEL_QT[G.Q4_K], Q.KERNEL_QT[G.Q6_K])
        assert lw.w13.kmajor and not lw.w2.kmajor and lw.w13.shape == (8, 512, 512) and lw.w2.shape == (8, 512, 256)
    assert len({lw.w13.q.data_ptr() for lw in m.layers}) == 3 and len(m.quant_moes()) == 6
    assert torch.equal(m.layers[0].w13.q, m.layers[2].w13.q)  # layer 2 copies layer 0's generated stack
    x = torch.randn(5, 512, device=DEV, dtype=torch.bfloat16)
    y = m.moe(x, m.layers[1])
    assert y.shape == (5, 512) and torch.isfinite(y).all() and y.abs().max().item() > 0
