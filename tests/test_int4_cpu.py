"""4-bit checkpoints kept 4-bit (INT4), the parts that need no GPU: the loader's
``int4_part`` slicing of both on-disk layouts (compressed-tensors pack-quantized, AutoAWQ
gemm), which checkpoints count as native, the synthetic ``--quantization int4`` model under
TP on gloo, the prefill budget and the CLI flag."""
import json

import pytest
import torch

from hipserve.weights import int_quant as iq
from hipserve.weights.safetensors_loader import _Ckpt

N, K, G = 48, 512, 64


def _write(path, tensors, qcfg):
    from safetensors.torch import save_file

    path.mkdir()
    save_file({k: v.clone().contiguous() for k, v in tensors.items()}, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps({"model_type": "llama", "quantization_config": qcfg}))
    return _Ckpt(str(path))


CT4 = {"quant_method": "compressed-tensors", "format": "pack-quantized",
       "config_groups": {"group_0": {"targets": ["Linear"], "weights": {
           "num_bits": 4, "group_size": G, "symmetric": False, "strategy": "group", "type": "int"}}}}
AWQ4 = {"quant_method": "awq", "bits": 4, "group_size": G, "version": "GEMM", "zero_point": True}


def _rand(seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 16, (N, K), generator=g)
    scale = (torch.rand(N, K // G, generator=g) * 0.01 + 0.001).half()
    zero = torch.randint(0, 16, (N, K // G), generator=g)
    return u, scale, zero


def _same(part, u, scale, zero, rows, cols):
    gcols = slice(cols.start // G, cols.stop // G) if cols != slice(None) else cols
    assert part is not None
    pu, ps, pz = part
    assert pu.dtype == torch.uint8 and torch.equal(pu.long(), u[rows, cols])
    assert torch.equal(ps.float(), scale.float()[rows, gcols])
    if zero is None:
        assert pz is None
    else:
        assert torch.equal(pz.float(), zero.float()[rows, gcols])


def _slices(ck, name, u, scale, zero):
    assert ck.is_int4(name)
    _same(ck.int4_part(name, 0, 0, N), u, scale, zero, slice(0, N), slice(None))
    _same(ck.int4_part(name, 0, 16, 40), u, scale, zero, slice(16, 40), slice(None))
    _same(ck.int4_part(name, 1, 128, 384), u, scale, zero, slice(None), slice(128, 384))
    _same(ck.int4_part(name, 1, 0, 256), u, scale, zero, slice(None), slice(0, 256))
    assert ck.int4_part(name, 1, 32, 288) is None   # splits a group
    assert ck.int4_part(name, 1, 0, 96) is None


def test_int4_part_pack_quantized(tmp_path):
    u, scale, zero = _rand(1)
    shape = torch.tensor([N, K], dtype=torch.int32)
    q = u - 8  # stored signed; the zero point likewise
    t = {"sym.weight_packed": iq.pack_pack_quantized(q, 4), "sym.weight_scale": scale, "sym.weight_shape": shape,
         # zero points packed along N, as llm-compressor writes them
         "zpk.weight_packed": iq.pack_pack_quantized(q, 4), "zpk.weight_scale": scale, "zpk.weight_shape": shape,
         "zpk.weight_zero_point": iq.pack_pack_quantized((zero - 8).t().contiguous(), 4).t().contiguous(),
         # unpacked signed zero points, no weight_shape
         "zun.weight_packed": iq.pack_pack_quantized(q, 4), "zun.weight_scale": scale,
         "zun.weight_zero_point": (zero - 8).to(torch.int8),
         # per channel
         "chn.weight_packed": iq.pack_pack_quantized(q, 4), "chn.weight_scale": scale[:, :1], "chn.weight_shape": shape}
    ck = _write(tmp_path / "ct", t, CT4)
    _slices(ck, "sym.weight", u, scale, None)
    _slices(ck, "zpk.weight", u, scale, zero)
    _slices(ck, "zun.weight", u, scale, zero)
    # the slices dequantise to what the dequantise-at-load path gives
    pu, ps, pz = ck.int4_part("zpk.weight", 0, 0, N)
    w = (pu.float() - pz.repeat_interleave(G, 1)) * ps.repeat_interleave(G, 1)
    assert torch.equal(w, ck.full("zpk.weight").float())
    # per channel: any column slice keeps the one scale
    pu, ps, pz = ck.int4_part("chn.weight", 1, 32, 288)
    assert torch.equal(pu.long(), u[:, 32:288]) and ps.shape == (N, 1) and pz is None
    # honours weight_shape: K not a multiple of 8 values per word would be cut there
    assert ck.int4_part("sym.weight", 0, 0, N)[0].shape == (N, K)


def test_int4_part_awq(tmp_path):
    u, scale, zero = _rand(2)
    t = {"x.qweight": iq.awq_pack(u.t().contiguous()), "x.qzeros": iq.awq_pack(zero.t().contiguous()),
         "x.scales": scale.t().contiguous()}
    ck = _write(tmp_path / "awq", t, AWQ4)
    # AutoAWQ's interleave: nibble 1 of word 0 holds column 2 (output row 2 of the HF layout)
    assert int(t["x.qweight"][0, 0] >> 4 & 0xF) == int(u[2, 0])
    assert int(ck.int4_part("x.weight", 0, 0, N)[0][2, 0]) == int(u[2, 0])
    _slices(ck, "x.weight", u, scale, zero)
    pu, ps, pz = ck.int4_part("x.weight", 0, 0, N)
    w = (pu.float() - pz.repeat_interleave(G, 1)) * ps.repeat_interleave(G, 1)
    assert torch.equal(w, ck.full("x.weight").float())


@pytest.mark.parametrize("qcfg,native", [
    (AWQ4, True), ({**AWQ4, "version": "gemm"}, True), ({k: v for k, v in AWQ4.items() if k != "version"}, True),
    ({**AWQ4, "version": "gemv"}, False), ({**AWQ4, "quant_method": "gptq"}, False), ({}, False)])
def test_qweight_is_native_only_for_awq_gemm(tmp_path, qcfg, native):
    u, scale, zero = _rand(3)
    t = {"x.qweight": iq.awq_pack(u.t().contiguous()), "x.qzeros": iq.awq_pack(zero.t().contiguous()),
         "x.scales": scale.t().contiguous()}
    ck = _write(tmp_path / "c", t, qcfg)
    assert ck.is_int4("x.weight") == native
    assert ck.has("x.weight")  # the dequantise-at-load path still reads it, as before


def test_ct_8bit_is_not_int4(tmp_path):
    q = torch.randint(-128, 128, (N, K))
    cfg8 = json.loads(json.dumps(CT4))
    cfg8["config_groups"]["group_0"]["weights"]["num_bits"] = 8
    ck = _write(tmp_path / "c8", {"x.weight_packed": iq.pack_pack_quantized(q, 8),
                                  "x.weight_scale": torch.ones(N, K // G)}, cfg8)
    assert not ck.is_int4("x.weight") and ck.is_int8_ct("x.weight")


def test_int4_synthetic_tp2_matches_tp1():
    """``quantization: int4`` off the GPU: the same integers dequantised to dense weights,
    sharded so that TP = 2 runs the model TP = 1 runs (nibbles, zero points and groups are
    keyed by the position in the unsharded tensor)."""
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup
    from tests.test_tp_cpu import PROMPTS, _cfg, _run_tp

    from hipserve.engine.request import SamplingParams

    preset = "tiny-llama-tp8:int4"
    ref = LLMEngine(_cfg(preset, 1), tp=TPGroup())
    w = ref.runner.model.layers[0].wd  # 4-bit grid: every weight an integer multiple of the scale
    r = w.float() / 0.00375
    assert (r - r.round()).abs().max().item() < 2e-2 and r.abs().max().item() <= 15.01
    want = [r[0] for r in ref.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))]
    assert _run_tp(preset, 2) == want


def test_int4_budget_and_cli():
    from hipserve.config import default_batched_tokens
    from hipserve.server.cli import build_parser, config_from_args

    assert default_batched_tokens("llama-3-8b", quantization="int4") == 32768
    a = build_parser().parse_args(["--model", "llama-3-8b", "--device", "cpu", "--load-format", "dummy",
                                   "--quantization", "int4"])
    cfg = config_from_args(a)
    assert cfg.extra == {"quantization": "int4"} and cfg.max_num_batched_tokens == 32768
