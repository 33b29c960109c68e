"""Gemma-3 image side on the hipserve op set: the SigLIP vision tower and the
multimodal projector (HF ``Gemma3ForConditionalGeneration``: ``vision_tower`` =
``SiglipVisionModel`` without its pooling head, ``multi_modal_projector``).

Per image (prefill only; the language model never sees pixels):

* patch embedding: the Conv2d of HF (kernel = stride = patch over 3 channels) is a GEMM
  over the unfolded patches with the bias in its epilogue, plus the learned position
  table — the image size is fixed, so the table is added as it is (no resampling);
* ``depth`` pre-LN blocks: LayerNorm -> q/k/v GEMM with bias -> bidirectional attention
  over the image's patches (``vision_attention`` without RoPE) -> out projection ->
  residual; LayerNorm -> fc1 -> tanh-GELU -> fc2 -> residual; then ``post_layernorm``;
* projector: ``vision_pool_rmsnorm`` (the k x k average pool of the patch grid down to
  ``mm_tokens_per_image`` and Gemma's RMSNorm in one kernel) and one GEMM with
  ``mm_input_projection_weight`` into the language model's hidden size.

The projected rows replace the embeddings of the image placeholder tokens after the
embedding scale (``LlamaModel.forward``). Parity with transformers is pinned by
``tests/test_gemma3_vision_cpu.py``.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from ..config import VisionConfig
from .vision import VisionBlock

_TANH = ("gelu_pytorch_tanh", "gelu_tanh")


class SiglipTower:
    def __init__(self, cfg: VisionConfig, device, dtype, ops):
        assert cfg.kind == "siglip"
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.ops = ops
        self.eps = cfg.layer_norm_eps
        self.blocks: list[VisionBlock] = []
        self.patch_w = self.patch_b = self.pos_embed = None
        self.post_w = self.post_b = None
        self.soft_norm = None    # mm_soft_emb_norm.weight [C]
        self.proj_w = None       # mm_input_projection_weight transposed: [hidden, C]

    # ------------------------------------------------------------ weights
    def load(self, get, tower_prefix: str, proj_prefix: str):
        """``get(name) -> tensor`` over a checkpoint; prefixes e.g.
        "vision_tower.vision_model." and "multi_modal_projector." (or both under "model.")."""
        c = self.cfg

        def t(name):
            return get(name).to(device=self.device, dtype=self.dtype).contiguous()

        tp = tower_prefix
        self.patch_w = t(tp + "embeddings.patch_embedding.weight").reshape(c.hidden_size, -1).contiguous()
        self.patch_b = t(tp + "embeddings.patch_embedding.bias")
        self.pos_embed = t(tp + "embeddings.position_embedding.weight")
        if self.pos_embed.shape[0] != c.grid * c.grid:
            raise ValueError(f"SigLIP position table has {self.pos_embed.shape[0]} rows, "
                             f"the {c.grid} x {c.grid} patch grid needs {c.grid * c.grid}")
        self.blocks = []
        for i in range(c.depth):
            p = f"{tp}encoder.layers.{i}."
            a = p + "self_attn."
            qkv_w = torch.cat([t(a + f"{n}_proj.weight") for n in "qkv"]).contiguous()
            qkv_b = torch.cat([t(a + f"{n}_proj.bias") for n in "qkv"]).contiguous()
            self.blocks.append(VisionBlock(
                t(p + "layer_norm1.weight"), t(p + "layer_norm1.bias"), qkv_w, qkv_b,
                t(a + "out_proj.weight"), t(a + "out_proj.bias"), t(p + "layer_norm2.weight"),
                t(p + "layer_norm2.bias"), t(p + "mlp.fc1.weight"), t(p + "mlp.fc1.bias"),
                t(p + "mlp.fc2.weight"), t(p + "mlp.fc2.bias")))
        self.post_w, self.post_b = t(tp + "post_layernorm.weight"), t(tp + "post_layernorm.bias")
        self.soft_norm = t(proj_prefix + "mm_soft_emb_norm.weight")
        self.proj_w = t(proj_prefix + "mm_input_projection_weight").t().contiguous()

    def allocate_random(self, seed: int = 0, std: float = 0.02):
        """Random-init tower of the configured shape (benchmarks / smoke tests), filled on the
        tower's device by the keyed generator of the language model's dummy weights
        (``fill_uniform``: the same values on the GPU, on the CPU and on every TP rank)."""
        c = self.cfg
        C, I = c.hidden_size, c.intermediate_size
        scale, n = std * 3.0 ** 0.5, [0]

        def rnd(rows, cols):
            n[0] += 1
            w = torch.empty(rows, cols, device=self.device, dtype=self.dtype)
            return self.ops.fill_uniform(w, 0, 0, cols, (seed * 1000003 + 0x5151 + n[0] * 7919) & 0xFFFFFFFF, scale)

        def ones(n):
            return torch.ones(n, device=self.device, dtype=self.dtype)

        def zeros(n):
            return torch.zeros(n, device=self.device, dtype=self.dtype)

        self.patch_w, self.patch_b = rnd(C, c.patch_dim), zeros(C)
        self.pos_embed = rnd(c.grid * c.grid, C)
        self.blocks = [VisionBlock(ones(C), zeros(C), rnd(3 * C, C), zeros(3 * C), rnd(C, C), zeros(C),
                                   ones(C), zeros(C), rnd(I, C), zeros(I), rnd(C, I), zeros(C))
                       for _ in range(c.depth)]
        self.post_w, self.post_b = ones(C), zeros(C)
        self.soft_norm = zeros(C)
        self.proj_w = rnd(c.out_hidden_size, C)

    # ------------------------------------------------------------ forward
    @torch.inference_mode()
    def forward(self, pixels: torch.Tensor, geo=None):
        """pixels [images * grid^2, patch_dim] (patches row-major per image) ->
        (embeddings [images * mm_tokens_per_image, out_hidden], []) — the second value
        is the (empty) DeepStack list of the Qwen3-VL tower's interface."""
        c, ops, dev = self.cfg, self.ops, self.device
        nh, D, N = c.num_heads, c.head_dim, c.grid * c.grid
        if pixels.shape[0] % N:
            raise ValueError(f"SigLIP tower: {pixels.shape[0]} patches are not whole images of {N}")
        images = pixels.shape[0] // N
        x = F.linear(pixels.to(device=dev, dtype=self.dtype), self.patch_w, self.patch_b)
        x = (x.view(images, N, -1) + self.pos_embed).view(images * N, -1)
        cu = np.arange(images + 1, dtype=np.int32) * N
        meta = ops.vision_meta(SimpleNamespace(cu_seqlens=cu), nh, D) if hasattr(ops, "vision_meta") else None
        cu_t = torch.from_numpy(cu).to(dev)
        scale = D ** -0.5
        tanh = c.hidden_act in _TANH
        xn = torch.empty_like(x)
        attn = torch.empty(images * N, nh * D, device=dev, dtype=self.dtype)
        pending = None  # residual stream update not yet added (fused into the next LayerNorm)
        for b in self.blocks:
            if pending is None:
                ops.layernorm(xn, x, b.n1w, b.n1b, self.eps)
            else:
                ops.layernorm(xn, pending, b.n1w, b.n1b, self.eps, residual=x)
            qkv = F.linear(xn, b.qkv_w, b.qkv_b)
            ops.vision_attention(attn, qkv, None, cu_t, nh, D, scale, meta)  # no RoPE: learned positions
            o = F.linear(attn, b.proj_w, b.proj_b)
            ops.layernorm(xn, o, b.n2w, b.n2b, self.eps, residual=x)
            if xn.is_cuda and tanh:  # fc1 + bias + GELU in one hipBLASLt call (as the Qwen3-VL tower)
                h = torch._addmm_activation(b.fc1_b, xn, b.fc1_w.t(), use_gelu=True)
            else:
                h = F.linear(xn, b.fc1_w, b.fc1_b)
                ops.gelu_(h, tanh)
            pending = F.linear(h, b.fc2_w, b.fc2_b)
        if pending is None:
            ops.layernorm(xn, x, self.post_w, self.post_b, self.eps)
        else:
            ops.layernorm(xn, pending, self.post_w, self.post_b, self.eps, residual=x)
        pooled = torch.empty(images * c.mm_tokens_per_image, c.hidden_size, device=dev, dtype=self.dtype)
        ops.vision_pool_rmsnorm(pooled, xn, self.soft_norm, c.grid, c.pool, self.eps)
        return F.linear(pooled, self.proj_w), []
