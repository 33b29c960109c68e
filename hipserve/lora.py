"""Multi-LoRA serving: PEFT adapters resident next to one base model.

Every listed adapter is read at start-up (``adapter_config.json`` + ``adapter_model
.safetensors``) into fixed-shape, zero-filled device tensors per layer and merged
projection: ``A [slots, R, K]``, ``B [slots, N, r]`` and ``scale [slots]``. The merged
``wqkv`` is block-diagonal over q | k | v (A matrices stacked along R, one r-column block of
t per slice), ``wgu`` over gate | up; a missing module or a smaller rank is a zero block.
A batch row names its adapter by slot (-1: the base model) and the kernels of
``csrc/kernels/lora.hip`` apply each row's own pair (``LoraBatch.apply``): one shrink and
one expand launch per projection that any resident adapter targets, none for the others.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass

import torch

# PEFT module name -> (merged projection, slice); Phi-3's fused modules are one-slice projections
MODULES = {"q_proj": ("qkv", 0), "k_proj": ("qkv", 1), "v_proj": ("qkv", 2), "qkv_proj": ("qkv", None),
           "o_proj": ("o", 0), "gate_proj": ("gu", 0), "up_proj": ("gu", 1), "gate_up_proj": ("gu", None),
           "down_proj": ("d", 0)}
PROJS = ("qkv", "o", "gu", "d")
MAX_LORA_RANKS = (8, 16, 32, 64)


@dataclass
class LoraProj:
    """One merged projection of one layer over all slots."""
    A: torch.Tensor       # [slots, R, K]
    B: torch.Tensor       # [slots, N, r]
    scale: torch.Tensor   # fp32 [slots]
    slices: tuple         # ((n_begin, t_offset), ...)
    r: int


def _pad_rank(r: int) -> int:
    return 16 if r <= 16 else 32 if r <= 32 else 64


def read_adapter(name: str, path: str, max_rank: int):
    """(config, {(layer, module): (A [r, K], B [N, r])}) of a PEFT directory, or a
    ``ValueError`` that names the adapter and what it uses that is not served."""
    def refuse(why):
        raise ValueError(f"LoRA adapter {name!r} ({path}): {why}")

    cfile = os.path.join(path, "adapter_config.json")
    if not os.path.exists(cfile):
        refuse("no adapter_config.json")
    with open(cfile) as f:
        cfg = json.load(f)
    if cfg.get("peft_type", "LORA") != "LORA":
        refuse(f"peft_type {cfg.get('peft_type')} is not LORA")
    if cfg.get("use_dora"):
        refuse("DoRA (use_dora) is not supported")
    if cfg.get("bias", "none") != "none":
        refuse(f"bias={cfg['bias']!r} is not supported (only \"none\")")
    if cfg.get("modules_to_save"):
        refuse(f"modules_to_save {cfg['modules_to_save']} is not supported")
    r = int(cfg["r"])
    if r > max_rank:
        refuse(f"rank {r} is above --max-lora-rank {max_rank}")
    from safetensors import safe_open

    mods = {}
    with safe_open(os.path.join(path, "adapter_model.safetensors"), framework="pt") as f:
        for key in f.keys():
            parts = key.split(".")
            if "layers" not in parts or parts[-2] not in ("lora_A", "lora_B") or parts[-3] not in MODULES \
                    or parts[-4] not in ("self_attn", "mlp"):
                refuse(f"tensor {key} targets a module that takes no adapter (embeddings, lm_head, the router "
                       "and the experts do not; DoRA magnitudes and biases neither)")
            layer = int(parts[parts.index("layers") + 1])
            mods.setdefault((layer, parts[-3]), {})[parts[-2]] = f.get_tensor(key)
    out = {}
    for k, ab in mods.items():
        if set(ab) != {"lora_A", "lora_B"} or ab["lora_A"].shape[0] != ab["lora_B"].shape[1]:
            refuse(f"layer {k[0]} {k[1]}: lora_A and lora_B do not pair up")
        if ab["lora_A"].shape[0] > max_rank:
            refuse(f"layer {k[0]} {k[1]}: rank {ab['lora_A'].shape[0]} is above --max-lora-rank {max_rank}")
        out[k] = (ab["lora_A"], ab["lora_B"])
    scale = float(cfg.get("lora_alpha", r)) / (math.sqrt(r) if cfg.get("use_rslora") else r)
    return scale, out


class LoraSet:
    """All resident adapters of an engine on one model (the handle ``AttnMeta.lora`` carries)."""

    def __init__(self, model, modules: dict, max_loras: int | None = None, max_rank: int = 16):
        if max_rank not in MAX_LORA_RANKS:
            raise ValueError(f"--max-lora-rank must be one of {MAX_LORA_RANKS}, got {max_rank}")
        if not modules:
            raise ValueError("--enable-lora needs at least one --lora-modules name=path")
        slots = max_loras or len(modules)
        if len(modules) > slots:
            raise ValueError(f"{len(modules)} adapters listed but --max-loras is {slots}: all adapters are resident")
        if os.environ.get("HIPSERVE_SINGLE_LAYOUT") == "1":
            raise ValueError("--enable-lora keeps row-major gate|up weights: it cannot run with a forced "
                             "single layout (HIPSERVE_SINGLE_LAYOUT=1)")
        self.names = list(modules)
        self.num_slots = slots
        cfg, dev, dt = model.cfg, model.device, model.dtype
        D, H = model.D, cfg.hidden_size
        moe = bool(cfg.num_experts)
        # this rank's (K, slice widths) of each merged projection, and where its share lies in the
        # checkpoint's: column-parallel projections (qkv, gate|up) replicate A and take their rows of
        # B; row-parallel ones (o, down) take their columns of A and the whole of B, so each rank
        # expands its partial t into its partial output and the existing cross-rank sum adds them up
        geo = {"qkv": (H, (model.nq * D, model.nkv * D, model.nkv * D)), "o": (model.nq * D, (H,)),
               "gu": (H, (model.inter, model.inter)), "d": (model.inter, (H,))}
        W, rank = model.tp.world_size, model.tp.rank
        kv0 = rank * model.nkv if cfg.num_kv_heads >= W else rank // (W // cfg.num_kv_heads)  # as the weight loader
        qs, ks = (rank * model.nq * D, model.nq * D), (kv0 * D, model.nkv * D)
        inter = 0 if moe else cfg.intermediate_size
        ms = (rank * model.inter, model.inter)
        full = {"qkv": (H, (cfg.num_heads * D, cfg.num_kv_heads * D, cfg.num_kv_heads * D)), "o": (cfg.num_heads * D, (H,)),
                "gu": (H, (inter, inter)), "d": (inter, (H,))}
        share = {"qkv": (qs, ks, ks), "gu": (ms, ms), "o": (qs,), "d": (ms,)}  # (start, length) per slice

        def local(proj, sl, A, B):
            """This rank's share of a checkpoint-sized pair."""
            if proj in ("o", "d"):
                a, n = share[proj][0]
                return A[:, a:a + n], B
            begins = [sum(full[proj][1][:j]) for j in range(len(full[proj][1]))]
            js = range(len(begins)) if sl is None else (sl,)
            return A, torch.cat([B[(0 if sl is not None else begins[j]) + share[proj][j][0]:][:share[proj][j][1]] for j in js])

        read = [(n, *read_adapter(n, p, max_rank)) for n, p in modules.items()]
        L = len(model.layers)
        fusedm = {}  # projection -> True if targeted through Phi-3's fused module
        for n, _, mods in read:
            for (layer, mod), (A, B) in mods.items():
                proj, sl = MODULES[mod]
                if layer >= L:
                    raise ValueError(f"LoRA adapter {n!r}: layer {layer} does not exist in the base model")
                if moe and proj in ("gu", "d"):
                    raise ValueError(f"LoRA adapter {n!r}: {mod} targets the experts of a MoE model (q/k/v/o only)")
                if fusedm.setdefault(proj, sl is None) != (sl is None):
                    raise ValueError(f"LoRA adapter {n!r}: {mod} mixes fused and split modules of one projection")
                K, widths = full[proj]
                N = sum(widths) if sl is None else widths[sl]
                if tuple(A.shape[1:]) != (K,) or B.shape[0] != N:
                    raise ValueError(f"LoRA adapter {n!r}: layer {layer} {mod} is {tuple(B.shape)} x {tuple(A.shape)}, "
                                     f"the base projection is [{N}, {K}]")
                K, widths = geo[proj]
                N = sum(widths) if sl is None else widths[sl]
                if K % 64 or N % 16:
                    raise ValueError(f"LoRA adapter {n!r}: {mod} [{N}, {K}] (per rank) needs K % 64 == 0 and N % 16 == 0")
        self.layers: list[dict] = [dict() for _ in range(L)]
        for layer in range(L):
            for proj in PROJS:
                hit = [(s, scale, MODULES[mod][1], *local(proj, MODULES[mod][1], A, B)) for s, (n, scale, mods) in enumerate(read)
                       for (ly, mod), (A, B) in mods.items() if ly == layer and MODULES[mod][0] == proj]
                if not hit:
                    continue  # no resident adapter targets it: nothing is launched
                K, widths = geo[proj]
                if fusedm[proj]:
                    widths = (sum(widths),)
                r = _pad_rank(max(A.shape[0] for *_, A, _ in hit))
                begins = [sum(widths[:j]) for j in range(len(widths))]
                At = torch.zeros(slots, r * len(widths), K, dtype=dt)
                Bt = torch.zeros(slots, sum(widths), r, dtype=dt)
                sc = torch.zeros(slots, dtype=torch.float32)
                for s, scale, sl, A, B in hit:
                    j = sl or 0
                    At[s, j * r:j * r + A.shape[0]] = A.to(dt)
                    Bt[s, begins[j]:begins[j] + B.shape[0], :B.shape[1]] = B.to(dt)
                    sc[s] = scale
                self.layers[layer][proj] = LoraProj(At.to(dev), Bt.to(dev), sc.to(dev),
                                                    tuple((b, j * r) for j, b in enumerate(begins)), r)
        self.targets = sorted({p for ly in self.layers for p in ly})
        rmax = max((p.A.shape[1] for ly in self.layers for p in ly.values()), default=16)
        ops = model.ops
        self.ws = (torch.empty(ops.LORA_WS_ROWS * rmax, dtype=torch.float32, device=dev)
                   if hasattr(ops, "LORA_WS_ROWS") else None)

    def slot(self, name: str) -> int:
        return self.names.index(name)

    def bytes(self) -> int:
        return sum(t.numel() * t.element_size() for ly in self.layers for p in ly.values() for t in (p.A, p.B))


@dataclass
class LoraBatch:
    """``AttnMeta.lora``: the step's per-row slot (int32 [T], -1: base) and the slot tensors."""
    idx: torch.Tensor
    set: LoraSet

    def has(self, layer: int, proj: str) -> bool:
        return proj in self.set.layers[layer]

    def apply(self, ops, layer: int, proj: str, x: torch.Tensor, out: torch.Tensor):
        """out += scale * B (A x) per row, in place; ``out`` is the projection's output
        (the model's dtype) or slice 0 of its fp32 split-K partials."""
        p = self.set.layers[layer].get(proj)
        if p is None:
            return out
        M = x.shape[0]
        t = torch.empty(M, p.A.shape[1], device=x.device, dtype=x.dtype)
        ops.lora_shrink(t, x, p.A, self.idx[:M], self.set.ws)
        ops.lora_expand(out, t, p.B, p.scale, self.idx[:M], p.slices)
        return out

    def apply_partial(self, ops, layer: int, proj: str, x: torch.Tensor, pt):
        """The same into slice 0 of a decode GEMM's fp32 split-K partials ``pt`` = (ws [S, M, N],
        S), ahead of the epilogue that sums the slices."""
        p = self.set.layers[layer].get(proj)
        if p is not None:
            M, N = x.shape[0], p.B.shape[1]
            self.apply(ops, layer, proj, x, pt[0].reshape(-1)[:M * N].view(M, N))
