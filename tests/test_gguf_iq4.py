"""IQ4_NL / IQ4_XS on the CPU: the block decoders against scalar decoders written from the
format description, the quantisers' error against the codebook's widest step, the format
table rows, the range guard, and a file of the two formats through the CPU engine."""
import struct

import numpy as np
import pytest
import torch

from hipserve.config import PRESETS
from hipserve.ops import quant as Q
from hipserve.weights import gguf as G

FORMATS = [G.IQ4_NL, G.IQ4_XS]
IDS = ["IQ4_NL", "IQ4_XS"]
KVALUES = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]
# tiny-llama with rows of whole super-blocks (K % 256 == 0)
CFG = PRESETS["tiny-llama"].replace(hidden_size=256, head_dim=64, intermediate_size=512)


def _half(b, off):
    return np.float32(struct.unpack_from("<e", bytes(b[off:off + 2]))[0])


def _scalar_block(blk, qt):
    """One block (18 bytes / 32 weights or 136 bytes / 256 weights), one weight at a time."""
    d = _half(blk, 0)
    if qt == G.IQ4_NL:
        qs = blk[2:18]
        return np.array([d * np.float32(KVALUES[int(qs[j % 16]) >> 4 * (j // 16) & 15]) for j in range(32)], np.float32)
    scales_h, scales_l, qs = int(blk[2]) | int(blk[3]) << 8, blk[4:8], blk[8:136]
    out = np.empty(256, np.float32)
    for ib in range(8):
        ls = ((int(scales_l[ib // 2]) >> 4 * (ib % 2)) & 15) | (((scales_h >> 2 * ib) & 3) << 4)
        dl = d * np.float32(ls - 32)
        for j in range(16):
            out[32 * ib + j] = dl * np.float32(KVALUES[int(qs[16 * ib + j]) & 15])
            out[32 * ib + 16 + j] = dl * np.float32(KVALUES[int(qs[16 * ib + j]) >> 4])
    return out


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_dequantize_matches_scalar_decoder(qt):
    be, bb = G.BLOCK[qt]
    assert (be, bb) == ((32, 18) if qt == G.IQ4_NL else (256, 136)) and list(G.IQ4_VALUES) == KVALUES
    raw = Q.random_blocks(np.random.default_rng(qt), qt, 32, 512)
    b = raw.reshape(-1, bb)
    want = np.concatenate([_scalar_block(blk, qt) for blk in b])
    got = G.dequantize(raw, qt, 32 * 512)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # the generator's blocks: every code, every sub-block scale, all inside the kernel's range
    assert len(np.unique(np.concatenate([b[:, bb - be // 2:] & 15, b[:, bb - be // 2:] >> 4]))) == 16
    assert qt == G.IQ4_NL or len(np.unique(G.iq4xs_scales(b[:, 2:8]))) == 64
    assert Q.sub_scale_ok(raw, qt) and 0.01 < np.abs(got).mean() < 0.04


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_quantize_within_widest_table_step(qt):
    """Nearest entry under an absmax scale: every block's error stays below absmax / 127 (the
    block's unit) times 24, one more than the widest gap of the table (-127 to -104 is 23) and
    more than the 14 units by which a +absmax element overshoots the table's short end 113."""
    be, bb = G.BLOCK[qt]
    x = (np.random.default_rng(5).standard_normal((16, 512)) * 0.05).astype(np.float32)
    raw = G.quantize(x, qt)
    assert raw.dtype == np.uint8 and raw.size == x.size // be * bb
    y = G.dequantize(raw, qt, x.size)
    err = np.abs(x.reshape(-1, be) - y.reshape(-1, be)).max(1)
    assert (err <= np.abs(x.reshape(-1, be)).max(1) / 127 * 24).all()
    assert np.abs(x.reshape(-1) - y).mean() < 0.12 * np.abs(x).mean()  # 16 levels: about 8 % (Q4_0: 10 %)


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_format_row_chunk_and_range_guard(qt):
    f = {f.qtype: f for f in Q.FORMATS}[qt]
    assert (f.name, f.kqt, f.chunk_bytes) == (("IQ4_NL", 14, 2304) if qt == G.IQ4_NL else ("IQ4_XS", 15, 2208))
    assert f.gguf and f.moe and not f.prefill and not f.row_scaled and f.sub_shift == 2 and 13 not in Q.BY_KQT
    be, bb = G.BLOCK[qt]
    raw = Q.random_blocks(np.random.default_rng(1), qt, 32, 512).copy()
    tiled = Q.repack_tiled(raw, qt, 32, 512)
    assert tiled.shape == (2, 2, f.chunk_bytes) and tiled.dtype == np.uint8
    # |s| < 65504 / 2^22, s = d (IQ4_NL) / d (ls - 32) (IQ4_XS: block 3 gets ls = 0, s = -32 d)
    lim, top = 65504.0 / 2.0 ** 22, 1 if qt == G.IQ4_NL else 32
    b = raw.reshape(-1, bb)
    if qt == G.IQ4_XS:
        b[3, 2:8] = 0
    for d, ok in ((np.float16(-lim / top * 0.99), True), (np.float16(lim / top * 1.01), False)):
        b[3, 0:2] = np.frombuffer(d.tobytes(), np.uint8)
        assert Q.sub_scale_ok(raw, qt) == ok
        assert Q.QuantWeight.supported(qt, 512, 32, raw) == ok and Q.QuantMoE.supported(f.kqt, 32, 512, raw) == ok
    # tiled layout only: N % 16 == 0 and K % 256 == 0 (IQ4_NL's 32-element blocks too)
    assert Q.QuantWeight.supported(qt, 512) and not Q.QuantWeight.supported(qt, 512, 40)
    assert not Q.QuantWeight.supported(qt, 384, 32)


def test_file_and_cpu_engine(tmp_path):
    """IQ4_XS projections, IQ4_NL attn_v and token_embd, Q6_K output: the CPU engine decodes every
    tensor to fp32 and generates the dense forward's greedy tokens."""
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    from .test_engine_cpu import dense_greedy

    p = G.write_synthetic_llama_gguf(str(tmp_path / "m.gguf"), CFG, G.IQ4_XS, embd_type=G.IQ4_NL,
                                     tensor_types={"v": G.IQ4_NL, "output": G.Q6_K})
    gf = G.GGUFFile(p)
    kinds = {n: gf.tensors[n].type for n in ("token_embd.weight", "output.weight", "blk.0.attn_q.weight",
                                             "blk.0.attn_v.weight", "blk.1.ffn_down.weight")}
    assert list(kinds.values()) == [G.IQ4_NL, G.Q6_K, G.IQ4_XS, G.IQ4_NL, G.IQ4_XS]
    t = gf.tensors["blk.0.ffn_up.weight"]
    assert t.nbytes == t.n_elements // 256 * 136 and 0.02 < np.abs(gf.tensor_f32("blk.0.ffn_up.weight")).mean() < 0.08
    eng = LLMEngine(EngineConfig(model=p, device="cpu", dtype="float32", num_kv_blocks=128,
                                 max_model_len=256, max_num_batched_tokens=32), tp=TPGroup())
    m = eng.runner.model
    assert isinstance(m.layers[0].wqkv, torch.Tensor)
    assert torch.equal(m.embed, torch.from_numpy(gf.tensor_f32("token_embd.weight")))
    prompts = [[1, 300, 301, 302], list(range(260, 300))]
    res = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    for pr, r in zip(prompts, res):
        assert r[0] == dense_greedy(m, pr, 6)


@pytest.mark.parametrize("scheme", ["iq4_xs", "iq4_nl"])
def test_synthetic_scheme_and_cli(scheme):
    from hipserve.config import GGUF_QUANTS, default_batched_tokens
    from hipserve.models.llama import LlamaModel
    from hipserve.server.cli import build_parser

    a = build_parser().parse_args(["--model", "tiny-llama", "--load-format", "dummy", "--quantization", scheme])
    assert a.quantization == scheme and scheme in GGUF_QUANTS
    assert default_batched_tokens("llama-3-8b", quantization=scheme) == 16384
    types = dict(LlamaModel.QUANT_SCHEMES[scheme])
    assert types.pop("output") == G.Q6_K and set(types.values()) == {G.IQ4_XS if scheme == "iq4_xs" else G.IQ4_NL}
