"""MXFP4 on the GPU (csrc/kernels/mxfp4.hip): the W4A8 GEMM on the scaled FP4 MFMA against
an fp64 reference of the dequantised operands, the dequantiser against the CPU codec bit
for bit, and a synthetic MXFP4 model decoding on hipGraphs against the CPU engine."""
import functools

import pytest
import torch

from hipserve.config import PRESETS, EngineConfig
from hipserve.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one step | a last tile with idle waves | three parts in one 128-row tile | two tiles (256 rows:
# a wrap of the 3-slot ring) | six steps: a wrap of the 5-slot ring
SHAPES = [([128], 256), ([144], 512), ([32, 16, 16], 768), ([256, 128], 1024), ([64], 1536)]


@pytest.fixture(autouse=True, scope="module")
def _lib():
    from hipserve.ops import load_library

    load_library()


@functools.lru_cache(maxsize=None)
def _weight(rows, K):
    """(QuantWeight, [(nibbles, scales)], fp64 dequantised [N, K]): uniform codes (all 16
    occur), every 32-block with its own E8M0 byte from [110, 130]."""
    g = torch.Generator().manual_seed(K + sum(rows))
    raw = []
    for n in rows:
        codes = torch.randint(0, 16, (n, K), generator=g)
        assert codes.unique().numel() == 16
        raw.append(((codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8),
                    torch.randint(110, 131, (n, K // 32), generator=g).to(torch.uint8)))
    w = Q.QuantWeight([Q.QuantPart.from_mxfp4(nib, sc, DEV) for nib, sc in raw])
    return w, raw, torch.cat([Q.mxfp4_dequantize(nib, sc) for nib, sc in raw]).double().to(DEV)


@pytest.mark.parametrize("M", [1, 16, 17, 64, 65, 256])
@pytest.mark.parametrize("rows,K", SHAPES)
def test_mxfp4_gemm_vs_fp64(M, rows, K):
    """Bound: tests/test_fp8_decode_gpu.py's per-row-normalised 1e-4 (the products are exact,
    only the fp32 accumulation order differs), here against fp64."""
    from hipserve.ops import pgemm

    w, _, wd = _weight(tuple(rows), K)
    assert Q.is_mxfp4(w) and Q.f8_decode_ok(w) and not w.v2
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K)
    x = (torch.rand(M, K, device=DEV, generator=g) * 2 - 1) * torch.logspace(-1, 1, M, device=DEV).unsqueeze(1)
    xq, xs = pgemm.act_quant(x.to(torch.bfloat16))
    want = (xq.view(torch.float8_e4m3fn).double() * xs.double().unsqueeze(1)) @ wd.t()
    scale = want.abs().amax(1, keepdim=True).clamp_min(1e-30)
    nsb = K // 256
    splits = [S for S in range(1, nsb + 1) if nsb % S == 0 and nsb // S in Q.F8D_STEPS]
    assert 1 in splits and nsb in splits
    for S in splits:
        ws = torch.full((S * M * w.N,), float("nan"), device=DEV)
        torch.ops.hipserve.mxfp4_gemm(ws, xq, xs, [p.q for p in w.parts], [p.N for p in w.parts], S)
        got = ws.view(S, M, w.N).sum(0).double()
        err = ((got - want) / scale).abs().max().item()
        print(f"rows={rows} K={K} M={M} S={S} max normalised error {err:.3e}")
        torch.testing.assert_close(got / scale, want / scale, rtol=0, atol=1e-4)


@pytest.mark.parametrize("rows,K", SHAPES[:4])
def test_mxfp4_dequant_is_the_codec(rows, K):
    w, raw, _ = _weight(tuple(rows), K)
    for p, (nib, sc) in zip(w.parts, raw):
        out = torch.full((p.N, K), float("nan"), dtype=torch.bfloat16, device=DEV)
        torch.ops.hipserve.mxfp4_dequant(out, p.q, p.N, K)
        want = Q.mxfp4_dequantize(nib, sc).to(torch.bfloat16)
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("M", [48, 256, 300])
def test_quant_linear_routes_mxfp4(M):
    """Up to 256 rows quant_linear is the W4A8 partials reduced; above, dequantise + bf16 GEMM."""
    w, _, wd = _weight((256, 128), 1024)
    g = torch.Generator(device=DEV).manual_seed(M)
    x = torch.randn(M, 1024, device=DEV, generator=g).to(torch.bfloat16)
    y = Q.quant_linear(x, w)
    if M <= Q.F8_DECODE_MAX_M:
        ws, S = Q.quant_partial(x, w)
        r = torch.empty_like(y)
        torch.ops.hipserve.splitk_reduce(r, ws, S)
        assert torch.equal(y, r)
    want = x.double() @ wd.t()
    # e4m3 rounding of x (M <= 256, ~2-3 % RMS per element) or bf16 rounding of the output
    rel = ((y.double() - want).norm() / want.norm()).item()
    assert rel < (5e-2 if M <= Q.F8_DECODE_MAX_M else 1e-2), rel


CFG = PRESETS["tiny-llama"].replace(hidden_size=256, head_dim=64, intermediate_size=512)
# Seed and prompts chosen on the CPU (fp32 engine, these weights) among 60 seeds x 400 random
# prompts: the top-2 logit gap over the 8 greedy steps is at least 0.312 / 0.227 / 0.099 for the
# three prompts (minimum 0.099 > 0.05), so a tie cannot hide a wrong kernel
SEED = 50
PROMPTS = [[1, 125, 86, 65, 125, 12, 178, 181, 377, 270, 304, 472, 422], [1, 183, 427, 87, 150, 162],
           [1, 365, 129, 321, 63, 329, 301]]


def _engine(device, tp=1, **kw):
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    dev = torch.device(device, 0) if device == "cuda" else torch.device("cpu")
    cfg = EngineConfig(model="tiny-llama", load_format="dummy", device=device, max_num_seqs=4,
                       max_num_batched_tokens=64, max_model_len=256, num_kv_blocks=128, seed=SEED,
                       extra={"quantization": "mxfp4"}, **kw)
    return LLMEngine(cfg, tp=TPGroup(0, tp, None, dev), model_cfg=CFG)


def test_engine_greedy_matches_cpu_on_graphs():
    from hipserve.engine.request import SamplingParams

    sp = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    g = _engine("cuda", dtype="bfloat16", enforce_eager=False)
    lw = g.runner.model.layers[0]
    assert all(Q.is_mxfp4(w) for w in (lw.wqkv, lw.wo, lw.wgu, lw.wd))
    c = _engine("cpu", dtype="float32")
    assert torch.equal(c.runner.model.layers[1].wd, Q.dequantize(g.runner.model.layers[1].wd).float().cpu())
    got, want = g.generate(PROMPTS, sp), c.generate(PROMPTS, sp)
    assert g.runner.use_graphs and g.runner.stats["graph_steps"] >= 7
    assert [r[0] for r in got] == [r[0] for r in want]


def test_tp2_is_refused():
    with pytest.raises(ValueError, match="one device"):
        _engine("cuda", tp=2)
