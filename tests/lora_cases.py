"""Shared by test_lora_cpu.py / test_lora_gpu.py: a tiny Llama (2 layers, hidden 256, GQA), two
random PEFT adapters and the checkpoints with an adapter merged into the weights."""
import json
import os

import torch
from safetensors.torch import save_file

from hipserve.config import PRESETS, EngineConfig
from hipserve.engine.llm_engine import LLMEngine
from hipserve.parallel.comm import TPGroup
from hipserve.weights.safetensors_loader import random_hf_tensors, save_hf_checkpoint

CFG = PRESETS["tiny-llama"].replace(name="tiny-llama-lora", hidden_size=256, num_heads=4, num_kv_heads=2, head_dim=64,
                                    intermediate_size=512, vocab_size=1024)
ATTN, MLP = ("q_proj", "k_proj", "v_proj", "o_proj"), ("gate_proj", "up_proj", "down_proj")
# name -> (rank, alpha, modules): rank 8 on q and v only; rank 16 on all seven
ADAPTERS = {"ad1": (8, 32, ("q_proj", "v_proj")), "ad2": (16, 64, ATTN + MLP)}
SEED = 4  # picked on the CPU: see test_lora_gpu.test_engine_mixed_batch
PROMPTS = [[1, 5, 9, 33, 70], list(range(3, 60)), [7] * 20, [1] + list(range(100, 140))]


def write_all(root):
    """Base checkpoint, the adapters as PEFT directories, and one merged checkpoint each."""
    base = random_hf_tensors(CFG, seed=SEED)
    paths = {"base": os.path.join(root, "base")}
    save_hf_checkpoint(paths["base"], CFG, base)
    g = torch.Generator().manual_seed(SEED)
    for name, (r, alpha, mods) in ADAPTERS.items():
        t, merged = {}, dict(base)
        for i in range(CFG.num_layers):
            for m in mods:
                w = f"model.layers.{i}.{'self_attn' if m in ATTN else 'mlp'}.{m}"
                N, K = base[w + ".weight"].shape
                A, B = torch.randn(r, K, generator=g) / K ** 0.5, torch.randn(N, r, generator=g) * 0.1
                t[f"base_model.model.{w}.lora_A.weight"], t[f"base_model.model.{w}.lora_B.weight"] = A, B
                merged[w + ".weight"] = base[w + ".weight"] + (alpha / r) * (B @ A)
        paths[name] = write_adapter(os.path.join(root, name), t, r=r, lora_alpha=alpha, target_modules=list(mods))
        paths[name + "-merged"] = os.path.join(root, name + "-merged")
        save_hf_checkpoint(paths[name + "-merged"], CFG, merged)
    return paths


def write_adapter(path, tensors, **cfg):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "bias": "none", **cfg}, f)
    save_file(tensors, os.path.join(path, "adapter_model.safetensors"))
    return path


def engine(model, device="cpu", lora=None, eager=True, **kw):
    cfg = EngineConfig(model=model, device=device, dtype="float32" if device == "cpu" else "bfloat16",
                       max_num_seqs=16, max_num_batched_tokens=256, max_model_len=512, num_kv_blocks=256,
                       enforce_eager=eager, enable_lora=lora is not None, lora_modules=lora or {}, **kw)
    dev = torch.device("cuda", 0) if device == "cuda" else torch.device("cpu")
    return LLMEngine(cfg, tp=TPGroup(0, 1, None, dev))


def tp_worker(rank, world, port, model, lora, name, q):
    """One TP rank on gloo: rank 0 generates PROMPTS under adapter ``name`` and reports
    (tokens, log-probs); the others follow its steps."""
    import torch.distributed as dist

    from hipserve.config import resolve_model_config
    from hipserve.engine.llm_engine import worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.engine.request import SamplingParams
    from hipserve.parallel.comm import init_tp

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    tp = init_tp(world, backend="gloo", device_type="cpu")
    cfg = EngineConfig(model=model, device="cpu", dtype="float32", tensor_parallel_size=world, max_num_seqs=16,
                       max_num_batched_tokens=256, max_model_len=512, num_kv_blocks=256, enable_lora=True,
                       lora_modules=lora)
    try:
        if rank == 0:
            eng = LLMEngine(cfg, tp=tp)
            sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True, lora=name)
            seqs = [eng.add_request(None, p, sp) for p in PROMPTS]
            while eng.has_unfinished():
                eng.step()
            eng.shutdown()
            q.put([(s.output_token_ids, s.output_logprobs) for s in seqs])
        else:
            worker_loop(ModelRunner(cfg, resolve_model_config(model), tp), tp)
    finally:
        dist.destroy_process_group()
    q.close()
    q.join_thread()
    os._exit(0)  # as tests/test_tp_cpu.py: no interpreter teardown under gloo's helper threads
