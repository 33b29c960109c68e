"""Q2_K / Q3_K on the CPU: the vectorised block decoders against scalar decoders written
from the format tables, the quantisers as fixed points of the codec, a numpy model of a
lane's view of the tiled chunks (the offsets and shifts of gguf_tiles.h), and files /
synthetic models of the two formats through the CPU engine."""
import struct

import numpy as np
import pytest
import torch

from hipserve.config import PRESETS
from hipserve.weights import gguf as G

FORMATS = [G.Q2_K, G.Q3_K]
# tiny-llama with rows of whole super-blocks (K % 256 == 0)
CFG = PRESETS["tiny-llama"].replace(hidden_size=256, head_dim=64, intermediate_size=512)
IDS = [G.TYPE_NAMES[t] for t in FORMATS]


def _half(b, off):
    return struct.unpack_from("<e", bytes(b[off:off + 2]))[0]


def _scalar_q2_k(blk):
    """One 84-byte super-block, one element at a time."""
    d, dmin = np.float32(_half(blk, 80)), np.float32(_half(blk, 82))
    out = np.empty(256, np.float32)
    for k in range(256):
        h, j, l = k // 128, (k % 128) // 32, k % 32
        q = (int(blk[16 + 32 * h + l]) >> (2 * j)) & 3
        s = int(blk[k // 16])
        out[k] = d * np.float32(s & 0xF) * np.float32(q) - dmin * np.float32(s >> 4)
    return out


def _scalar_q3_k(blk):
    """One 110-byte super-block, one element at a time."""
    d = np.float32(_half(blk, 108))
    sc = blk[96:108]
    out = np.empty(256, np.float32)
    for k in range(256):
        h, j, l = k // 128, (k % 128) // 32, k % 32
        low = (int(blk[32 + 32 * h + l]) >> (2 * j)) & 3
        hbit = (int(blk[l]) >> (4 * h + j)) & 1
        i = k // 16
        lo4 = int(sc[i]) & 0xF if i < 8 else int(sc[i - 8]) >> 4
        hi2 = (int(sc[8 + i % 4]) >> (2 * (i // 4))) & 3
        s = lo4 | (hi2 << 4)
        out[k] = d * np.float32(s - 32) * np.float32((low | (hbit << 2)) - 4)
    return out


def _random_blocks(qt, nb, seed):
    """Random bytes with finite f16 d / dmin of either sign."""
    rng = np.random.default_rng(seed)
    bb = G.BLOCK[qt][1]
    b = rng.integers(0, 256, size=(nb, bb), dtype=np.uint8)
    offs = (80, 82) if qt == G.Q2_K else (108,)
    for off in offs:
        b[:, off:off + 2] = (rng.standard_normal(nb) * 0.01).astype(np.float16).view(np.uint8).reshape(nb, 2)
    return b


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_dequantize_matches_scalar_decoder(qt):
    nb = 64
    b = _random_blocks(qt, nb, seed=qt)
    assert G.BLOCK[qt] == (256, 84 if qt == G.Q2_K else 110)
    scalar = _scalar_q2_k if qt == G.Q2_K else _scalar_q3_k
    want = np.stack([scalar(b[i]) for i in range(nb)])
    got = G.dequantize(b.reshape(-1), qt, nb * 256).reshape(nb, 256)
    assert got.dtype == np.float32 and np.isfinite(want).all()
    assert np.array_equal(got, want)
    # the random bytes reach every scale field value and every hmask bit
    if qt == G.Q2_K:
        assert len(np.unique(b[:, 0:16] & 0xF)) == 16 and len(np.unique(b[:, 0:16] >> 4)) == 16
    else:
        assert len(np.unique(G.q3k_scales(b[:, 96:108]))) == 64
        assert all(((b[:, 0:32] >> bit) & 1).any() and not ((b[:, 0:32] >> bit) & 1).all() for bit in range(8))


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_quantize_is_a_fixed_point(qt):
    x = np.random.default_rng(5).standard_normal((8, 256)).astype(np.float32)
    q1 = G.quantize(x, qt)
    assert q1.size == 8 * G.BLOCK[qt][1]
    y = G.dequantize(q1, qt, x.size)
    assert np.array_equal(G.quantize(y, qt), q1)
    # round to nearest on 4 / 8 levels per 16-element sub-block
    rel = np.abs(x.reshape(-1) - y).mean() / np.abs(x).mean()
    assert rel < (0.35 if qt == G.Q2_K else 0.2), rel
    b = q1.reshape(8, -1)
    if qt == G.Q2_K:  # scale and min fields vary over the sub-blocks
        assert len(np.unique(b[:, 0:16] & 0xF)) > 4 and len(np.unique(b[:, 0:16] >> 4)) > 4
    else:             # signed scales: both signs, and both values of the two high bits' top bit
        s = G.q3k_scales(b[:, 96:108]).astype(int)
        assert (s < 0).any() and (s > 0).any() and s.min() == -32 and len(np.unique(s)) > 16
        assert len(np.unique(b[:, 104:108])) > 4


def _lane_model(chunk, qt):
    """The [16, 256] weights of one tiled chunk as lane 16 g + c reads them: one 16-byte
    piece of qs (and of hmask), a uint2 of sub-block scales, d (and dmin); per step s the
    bit pair s >> 1 of words 2 (s & 1), 2 (s & 1) + 1 in the pair order {0, 2, 1, 3, 4, 6, 5, 7}
    at k = kbase(g, s)."""
    out = np.full((16, 256), np.nan, np.float32)
    so = 1024 if qt == G.Q2_K else 1536
    for lane in range(64):
        g, c = lane >> 4, lane & 15
        qs = chunk[16 * lane:16 * lane + 16].view("<u4")
        sc8 = chunk[so + 16 * c + 8 * (g >> 1):so + 16 * c + 8 * (g >> 1) + 8]
        if qt == G.Q2_K:
            d, dmin = (np.float32(v) for v in chunk[1280 + 4 * c:1284 + 4 * c].view(np.float16))
        else:
            hm = chunk[1024 + 32 * c + 16 * (g & 1):1024 + 32 * c + 16 * (g & 1) + 16].view("<u4")
            d = np.float32(chunk[1792 + 2 * c:1794 + 2 * c].view(np.float16)[0])
        for s in range(8):
            j = s >> 1
            sb = int(sc8[(g & 1) + 2 * j])
            q = []
            for wi in (2 * (s & 1), 2 * (s & 1) + 1):
                w = int(qs[wi])
                p02, p13 = (w >> (2 * j)) & 0x00030003, (w >> (2 * j + 8)) & 0x00030003
                if qt == G.Q3_K:
                    bit = 4 * (g >> 1) + j
                    p02 |= ((int(hm[wi]) >> bit) & 0x00010001) << 2
                    p13 |= ((int(hm[wi]) >> (bit + 8)) & 0x00010001) << 2
                q += [p02 & 0xFFFF, p02 >> 16, p13 & 0xFFFF, p13 >> 16]
            kb = 128 * (g >> 1) + 32 * j + 16 * (g & 1) + 8 * (s & 1)
            for e, off in enumerate((0, 2, 1, 3, 4, 6, 5, 7)):
                if qt == G.Q2_K:
                    v = d * np.float32(sb & 0xF) * np.float32(q[e]) - dmin * np.float32(sb >> 4)
                else:
                    v = d * np.float32(np.int8(np.uint8(sb))) * np.float32(q[e] - 4)
                assert np.isnan(out[c, kb + off])  # every k written once
                out[c, kb + off] = v
    return out


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_repack_tiled_lane_model(qt):
    from hipserve.ops import quant as Q

    N, K = 32, 512
    assert Q.CHUNK_BYTES[qt] == (1344 if qt == G.Q2_K else 1824) and Q.CHUNK_BYTES[qt] % 16 == 0
    assert Q.KERNEL_QT[qt] == (11 if qt == G.Q2_K else 12)
    raw = _random_blocks(qt, N * K // 256, seed=3 + qt).reshape(-1)
    want = G.dequantize(raw, qt, N * K).reshape(N, K)
    tiled = Q.repack_tiled(raw, qt, N, K)
    assert tiled.shape == (N // 16, K // 256, Q.CHUNK_BYTES[qt]) and tiled.dtype == np.uint8
    got = np.empty((N, K), np.float32)
    for r in range(N // 16):
        for sb in range(K // 256):
            got[16 * r:16 * r + 16, 256 * sb:256 * sb + 256] = _lane_model(tiled[r, sb], qt)
    assert np.array_equal(got, want)


def test_sub_scale_range_and_support():
    """Shifts 8 / 7: d sc < 65504 / 2^16 (Q2_K), |d (s - 32)| < 65504 / 2^17 (Q3_K). The two
    formats exist in the tiled layout only, and the block prefill GEMM does not take them."""
    from hipserve.ops import quant as Q

    assert Q.SUB_SHIFT[G.Q2_K] == 8 and Q.SUB_SHIFT[G.Q3_K] == 7
    rng = np.random.default_rng(0)
    for qt, off in ((G.Q2_K, 80), (G.Q3_K, 108)):
        raw = Q.random_blocks(rng, qt, 32, 512).copy()
        assert Q.sub_scale_ok(raw, qt)
        dense = G.dequantize(raw, qt, 32 * 512)
        assert 0.01 < np.abs(dense).mean() < 0.04
        lim = 65504.0 / 2.0 ** (24 - Q.SUB_SHIFT[qt])
        top = 15 if qt == G.Q2_K else 32
        b = raw.reshape(-1, G.BLOCK[qt][1])
        if qt == G.Q2_K:
            b[3, 0:16] = 0xFF   # sc = m = 15
        else:
            b[3, 96:108] = 0    # every s = 0: s - 32 = -32
        for d, ok in ((np.float16(lim / top * 0.99), True), (np.float16(lim / top * 1.01), False)):
            b[3, off:off + 2] = np.frombuffer(d.tobytes(), np.uint8)
            assert Q.sub_scale_ok(raw, qt) == ok, (G.TYPE_NAMES[qt], d)
            assert Q.QuantWeight.supported(qt, 512, 32, raw) == ok
        assert Q.QuantWeight.supported(qt, 512) and not Q.QuantWeight.supported(qt, 512, 40)
        assert not Q.QuantWeight.supported(qt, 384, 32)
        kqt = Q.KERNEL_QT[qt]
        assert kqt in Q.GGUF_KQT and kqt not in Q.QPG_KQT and kqt in Q.QuantMoE.KERNEL_QTS
        assert Q.QuantMoE.supported(kqt, 512, 256) and not Q.QuantMoE.supported(kqt, 512, 256, raw)
        with pytest.raises(NotImplementedError):
            Q.repack(raw, qt, 32, 512)  # no v1 row layout


@pytest.mark.parametrize("qt", FORMATS, ids=IDS)
def test_file_roundtrip_and_cpu_engine(tmp_path, qt):
    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import TPGroup

    from .test_engine_cpu import dense_greedy

    cfg = CFG
    p = str(tmp_path / "m.gguf")
    G.write_synthetic_llama_gguf(p, cfg, qt, embd_type=qt)
    gf = G.GGUFFile(p)
    for name in ("token_embd.weight", "output.weight", "blk.0.attn_q.weight", "blk.1.ffn_down.weight"):
        t = gf.tensors[name]
        assert t.type == qt and t.nbytes == t.n_elements // 256 * G.BLOCK[qt][1]
    t = gf.tensors["blk.0.ffn_up.weight"]
    w = gf.tensor_f32("blk.0.ffn_up.weight")
    assert w.shape == (cfg.intermediate_size, cfg.hidden_size) and np.isfinite(w).all()
    assert np.array_equal(G.quantize(w, qt), np.asarray(gf.raw("blk.0.ffn_up.weight")))  # the file holds fixed points
    assert 0.02 < np.abs(w).mean() < 0.08  # std 0.05 weights
    # the default keeps the embedding table in F16
    p16 = str(tmp_path / "m16.gguf")
    G.write_synthetic_llama_gguf(p16, cfg, qt)
    assert G.GGUFFile(p16).tensors["token_embd.weight"].type == G.F16
    eng = LLMEngine(EngineConfig(model=p, device="cpu", dtype="float32", num_kv_blocks=128,
                                 max_model_len=256, max_num_batched_tokens=32), tp=TPGroup())
    assert eng.runner.load_format == "gguf"
    m = eng.runner.model
    assert isinstance(m.layers[0].wqkv, torch.Tensor) and m.embed.shape == (cfg.vocab_size, cfg.hidden_size)
    assert torch.equal(m.embed, torch.from_numpy(gf.tensor_f32("token_embd.weight")))
    prompts = [[1, 300, 301, 302], list(range(260, 300))]
    res = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    for pr, r in zip(prompts, res):
        assert r[0] == dense_greedy(m, pr, 6)


@pytest.mark.parametrize("scheme", ["q3_k_m", "q2_k"])
def test_synthetic_scheme_cli_and_cpu_engine(scheme):
    from hipserve.config import GGUF_QUANTS, EngineConfig, default_batched_tokens
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.request import SamplingParams
    from hipserve.models.llama import LlamaModel
    from hipserve.parallel.comm import TPGroup
    from hipserve.server.cli import build_parser

    a = build_parser().parse_args(["--model", "tiny-llama", "--load-format", "dummy", "--quantization", scheme])
    assert a.quantization == scheme and scheme in GGUF_QUANTS
    assert default_batched_tokens("llama-3-8b", quantization=scheme) == 16384
    types = LlamaModel.QUANT_SCHEMES[scheme]
    if scheme == "q3_k_m":
        assert {types[k] for k in ("q", "k", "gate", "up", "gate_exps", "up_exps")} == {G.Q3_K}
        assert {types[k] for k in ("v", "o", "down", "down_exps")} == {G.Q4_K}
    else:
        assert {types[k] for k in ("q", "k", "gate", "up", "gate_exps", "up_exps")} == {G.Q2_K}
        assert {types[k] for k in ("v", "o", "down", "down_exps")} == {G.Q3_K}
    assert types["output"] == G.Q6_K
    eng = LLMEngine(EngineConfig(model="tiny-llama", load_format="dummy", device="cpu", dtype="float32",
                                 num_kv_blocks=128, max_model_len=256, max_num_batched_tokens=64,
                                 max_num_seqs=4, extra={"quantization": scheme}), tp=TPGroup(), model_cfg=CFG)
    m = eng.runner.model
    assert m.cfg.rope_mode == 1 and isinstance(m.layers[0].wqkv, torch.Tensor)
    assert torch.isfinite(m.layers[0].wqkv).all() and torch.isfinite(m.layers[0].wd).all()
    assert 0.005 < m.layers[0].wgu.abs().mean().item() < 0.05
    res = eng.generate([[1, 5, 6, 7]], SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    assert len(res[0][0]) == 6
