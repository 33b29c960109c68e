"""Expert-parallel MoE under TP (``--enable-expert-parallel``): the pure sharding
decision (``models.llama.moe_sharding``), the CLI flag, and a gloo TP=2 engine on the CPU
reference ops whose ranks each hold half of tiny-mixtral's experts at full width and must
generate exactly what TP=1 generates from the same checkpoint."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from hipserve.config import PRESETS, EngineConfig
from hipserve.engine.request import SamplingParams
from hipserve.models.llama import moe_sharding

PROMPTS = [[1, 5, 9, 33, 70], list(range(3, 60)), [7] * 20]
SP = dict(temperature=0.0, max_tokens=8, ignore_eos=True)


@pytest.mark.parametrize("tp,n_local", [(2, 64), (4, 32), (8, 16)])
def test_sharding_qwen3_picks_experts_where_width_has_no_kernel(tp, n_local):
    cfg = PRESETS["qwen3-30b-a3b"]  # 128 experts of width 768: 384 / 192 / 96 per rank, none % 256
    for rank in (0, tp - 1):
        assert moe_sharding(cfg, tp, False, True, rank) == ("expert", rank * n_local, n_local)
        assert moe_sharding(cfg, tp, True, True, rank) == ("expert", rank * n_local, n_local)
    # the CPU reference ops multiply any width: the width split stays
    assert moe_sharding(cfg, tp, False, False) == ("width", 768 // tp)
    assert moe_sharding(cfg, tp, True, False, 1) == ("expert", n_local, n_local)


def test_sharding_width_cases_unchanged():
    q3, mx = PRESETS["qwen3-30b-a3b"], PRESETS["mixtral-8x7b"]
    assert moe_sharding(q3, 1, False, True) == ("width", 768)
    assert moe_sharding(q3, 1, True, True) == ("width", 768)  # one rank: nothing to shard
    for hip in (True, False):
        assert moe_sharding(mx, 2, False, hip) == ("width", 14336 // 2)
        assert moe_sharding(mx, 8, False, hip, 3) == ("width", 14336 // 8)
    assert moe_sharding(mx, 2, True, True, 1) == ("expert", 4, 4)
    dense = PRESETS["llama-3-8b"]
    assert moe_sharding(dense, 2, True, True) == ("width", dense.intermediate_size // 2)


def test_sharding_errors_name_the_shape():
    mx = PRESETS["mixtral-8x7b"]
    with pytest.raises(ValueError, match=r"E=8, tp=16"):
        moe_sharding(mx.replace(num_heads=64, num_kv_heads=16), 16, True, True)
    odd = PRESETS["qwen3-30b-a3b"].replace(num_experts=6, num_experts_per_tok=2)  # 6 % 4 != 0, 768 / 4 = 192
    with pytest.raises(ValueError, match=r"E=6, tp=4"):
        moe_sharding(odd, 4, True, False)
    with pytest.raises(ValueError) as ei:
        moe_sharding(odd, 4, False, True)
    msg = str(ei.value)
    assert "6 experts of width 768" in msg and "TP=4" in msg and "--enable-expert-parallel" in msg
    assert moe_sharding(odd, 4, False, False) == ("width", 192)  # CPU ops: still the width split


def test_model_stores_the_decision():
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import get_ops
    from hipserve.parallel.comm import TPGroup

    cfg = PRESETS["tiny-mixtral"]
    ops = get_ops(torch.device("cpu"))
    m = LlamaModel(cfg, TPGroup(1, 2, None, torch.device("cpu")), "cpu", torch.float32, ops,
                   enable_expert_parallel=True)
    E = cfg.num_experts
    assert (m.moe_shard, m.expert_lo, m.num_local_experts, m.inter) == (("expert", E // 2, E // 2), E // 2, E // 2,
                                                                        cfg.expert_size)
    m.allocate_random(seed=3)
    assert m.layers[0].w13.shape == (E // 2, 2 * cfg.expert_size, cfg.hidden_size)
    assert m.layers[0].router.shape == (E, cfg.hidden_size)
    # the same unsharded dummy model: rank 1's experts are TP=1's experts E/2 ..
    one = LlamaModel(cfg, TPGroup(), "cpu", torch.float32, ops)
    one.allocate_random(seed=3)
    assert (one.moe_shard, one.expert_lo, one.num_local_experts) == (("width", cfg.expert_size), 0, E)
    assert torch.equal(m.layers[1].w13, one.layers[1].w13[E // 2:])
    assert torch.equal(m.layers[1].w2, one.layers[1].w2[E // 2:])
    wide = LlamaModel(cfg, TPGroup(1, 2, None, torch.device("cpu")), "cpu", torch.float32, ops)
    assert wide.moe_shard == ("width", cfg.expert_size // 2) and wide.num_local_experts == E


def test_cli_flag_reaches_engine_config():
    from hipserve.server.cli import build_parser, config_from_args

    base = ["--model", "tiny-mixtral", "--device", "cpu", "--load-format", "dummy"]
    assert config_from_args(build_parser().parse_args(base)).enable_expert_parallel is False
    cfg = config_from_args(build_parser().parse_args(base + ["--enable-expert-parallel", "-tp", "2"]))
    assert cfg.enable_expert_parallel is True and cfg.tensor_parallel_size == 2
    assert EngineConfig().enable_expert_parallel is False


class _FakeCkpt:
    """The checkpoint accessors ``_load_experts`` uses, over a dict of tensors."""

    def __init__(self, tensors):
        self.t = tensors

    def has(self, name):
        return name in self.t

    def full(self, name):
        return self.t[name]

    def rows(self, name, a, b):
        return self.t[name][a:b]

    def cols(self, name, a, b):
        return self.t[name][:, a:b]


@pytest.mark.parametrize("layout", ["per_expert", "fused", "fused_transposed"])
def test_loader_takes_the_expert_range_at_full_width(layout):
    """Per-expert tensors and the fused gate_up_proj / down_proj layouts (Qwen3-VL-MoE stores
    them transposed): ("expert", lo, n) gives experts lo .. lo + n - 1 unsliced, and the
    default still gives every expert's width slice."""
    from hipserve.weights.safetensors_loader import _load_experts

    cfg = PRESETS["qwen3-30b-a3b"].replace(hidden_size=16, moe_intermediate_size=24, num_experts=8)
    E, H, I = 8, 16, 24
    g = torch.Generator().manual_seed(0)
    gate, up, down = (torch.randn(E, I, H, generator=g), torch.randn(E, I, H, generator=g),
                      torch.randn(E, H, I, generator=g))
    p = "model.layers.0."
    t = {p + "mlp.gate.weight": torch.randn(E, H, generator=g)}
    if layout == "per_expert":
        for e in range(E):
            t.update({f"{p}mlp.experts.{e}.gate_proj.weight": gate[e], f"{p}mlp.experts.{e}.up_proj.weight": up[e],
                      f"{p}mlp.experts.{e}.down_proj.weight": down[e]})
    else:
        gu = torch.cat([gate, up], 1)
        tr = layout == "fused_transposed"
        t[p + "mlp.experts.gate_up_proj"] = gu.transpose(1, 2).contiguous() if tr else gu
        t[p + "mlp.experts.down_proj"] = down.transpose(1, 2).contiguous() if tr else down
    ck = _FakeCkpt(t)
    router, w13, w2 = _load_experts(ck, p, cfg, 1, I, lambda x: x.contiguous(), None, ("expert", 4, 4))
    assert router.shape == (E, H)
    assert torch.equal(w13, torch.cat([gate[4:], up[4:]], 1)) and torch.equal(w2, down[4:])
    _, w13, w2 = _load_experts(ck, p, cfg, 1, I // 2, lambda x: x.contiguous(), None, ("width", I // 2))
    sl = slice(I // 2, I)
    assert torch.equal(w13, torch.cat([gate[:, sl], up[:, sl]], 1)) and torch.equal(w2, down[:, :, sl])


def _cfg(ckpt, tp, ep):
    ckpt, _, quant = ckpt.partition(":")
    fmt = "safetensors" if os.path.isdir(ckpt) else "dummy"
    return EngineConfig(model=ckpt, load_format=fmt, device="cpu", dtype="float32", tensor_parallel_size=tp,
                        num_kv_blocks=128, max_model_len=256, max_num_batched_tokens=32, max_num_seqs=4,
                        enable_expert_parallel=ep, extra={"quantization": quant} if quant else {})


def _worker(rank, world, port, ckpt, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from hipserve.config import resolve_model_config
    from hipserve.engine.llm_engine import LLMEngine, worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.parallel.comm import init_tp

    tp = init_tp(world, backend="gloo", device_type="cpu")
    cfg = _cfg(ckpt, world, True)
    try:
        if rank == 0:
            eng = LLMEngine(cfg, tp=tp)
            m = eng.runner.model
            res = eng.generate(PROMPTS, SamplingParams(**SP))
            eng.shutdown()
            q.put(([r[0] for r in res], m.moe_shard, tuple(m.layers[0].w13.shape)))
        else:
            worker_loop(ModelRunner(cfg, resolve_model_config(ckpt.partition(":")[0]), tp), tp)
    finally:
        dist.destroy_process_group()
    # skip interpreter teardown (a joinable gloo helper thread can abort() at static destruction)
    q.close()
    q.join_thread()
    os._exit(0)


def _run_ep(ckpt, world):
    from tests.test_tp_cpu import _port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ckpt, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return out


@pytest.mark.parametrize("source", ["checkpoint", "dummy", "dummy:int8"])
def test_expert_parallel_tp2_matches_tp1(tmp_path, source):
    """fp32, greedy: the TP=2 engine with whole experts per rank generates TP=1's 8 tokens per
    prompt, from a checkpoint (the loader's expert range) and from dummy weights (keyed by
    the unsharded position; int8: per-channel scales with no cross-rank max for the experts)."""
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup
    from hipserve.weights.safetensors_loader import random_hf_tensors, save_hf_checkpoint

    cfg = PRESETS["tiny-mixtral"]
    if source == "checkpoint":
        ckpt = str(tmp_path / "tiny-mixtral")
        save_hf_checkpoint(ckpt, cfg, random_hf_tensors(cfg, seed=7))
    else:
        ckpt = "tiny-mixtral" + source[len("dummy"):]
    ref = LLMEngine(_cfg(ckpt, 1, True), tp=TPGroup())  # the flag is a no-op on one rank
    assert ref.runner.model.moe_shard[0] == "width"
    want = [r[0] for r in ref.generate(PROMPTS, SamplingParams(**SP))]
    got, shard, w13_shape = _run_ep(ckpt, 2)
    E = cfg.num_experts
    assert shard == ("expert", 0, E // 2) and w13_shape == (E // 2, 2 * cfg.expert_size, cfg.hidden_size)
    assert got == want
