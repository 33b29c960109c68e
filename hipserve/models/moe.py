"""Sparse mixture-of-experts MLP (Mixtral, Qwen3-MoE, Qwen3-VL-MoE): ``MoEMixin``, the
MoE half of ``models.llama.LlamaModel``. Per layer: router GEMM -> top-k softmax ->
expert-sorted row tiles (moe_align) -> w13 expert GEMM with the SiLU-GLU -> w2 expert
GEMM -> weighted combine; ``moe`` picks among the three kernel paths. At TP > 1 a rank
holds a width slice of every expert or, expert-sharded (``models.llama.moe_sharding``),
whole experts: routing stays over all experts, moe_align keeps the pairs of the local
expert range, and the all-reduce after the block sums the ranks' partial outputs."""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from ..ops import gemm, pgemm
from ..ops import quant as Q

log = logging.getLogger(__name__)

DG_MOE_STEPS = (1, 2, 3, 4, 6, 7, 8, 16)  # 256-k steps per K slice the expert decode GEMM is built for
MOE_KERNEL_MAX_PAIRS = 2048  # larger (prefill) batches take the packed grouped GEMM (moe_grouped) ...
MOE_KERNEL_MAX_ROWS_PER_EXPERT = 1024  # ... unless the streaming kernel timed faster below this (Qwen3-MoE: 128 x 768)


@dataclass
class ExpertWeights:
    """The ``LayerWeights`` fields the MoE paths read, for experts that are no layer's own."""
    router: torch.Tensor
    w13: torch.Tensor | None = None
    w2: torch.Tensor | None = None
    moe_packed: tuple | None = None


class MoEMixin:
    # experts this rank holds: all of them, width-sliced (the default), or whole experts
    # expert_lo .. expert_lo + num_local_experts - 1 (models.llama.moe_sharding). Routing is
    # over all cfg.num_experts either way; only the local count sizes tiles and buffers
    expert_lo: int = 0
    num_local_experts: int = 0

    def pack_moe_weights(self, drop_plain: bool = False) -> int:
        """Per-expert packed copies of the MoE weights for the decode expert GEMM
        (``moe_hip``): w13 gate/up-interleaved (SiLU-GLU in the GEMM epilogue), w2
        plain. The row-major originals stay unless ``drop_plain`` (single weight layout:
        the packed copy serves the grouped prefill GEMM too), so this doubles the expert
        bytes (Mixtral-8x7B: +90 GB of 288 GB) — skipped when less than 24 GiB of HBM
        would stay free for the KV cache, or with HIPSERVE_MOE_PACK=0 (the row-major
        expert GEMM runs instead)."""
        if (not self.cfg.num_experts or getattr(self.ops, "name", "") != "hip"
                or os.environ.get("HIPSERVE_MOE_PACK", "1") == "0"):
            return 0
        lws = [lw for lw in self.layers if isinstance(lw.w13, torch.Tensor) and self._moe_decode_ok(lw)]
        if not lws:
            return 0
        need = sum(2 * (lw.w13.numel() + lw.w2.numel()) for lw in lws)
        if drop_plain:  # the packed copy REPLACES the row-major experts (one layer at a time)
            if not all(lw.moe_packed is not None or self.cfg.hidden_act == "silu" for lw in lws):
                return 0
            need = 0
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            if need + (24 << 30) > free:
                log.warning("MoE decode weights not packed: %.1f GB needed, %.1f GB free", need / 2**30, free / 2**30)
                return 0
        freed = 0
        for lw in lws:
            if lw.moe_packed is None:
                lw.moe_packed = self._pack_experts(lw.w13, lw.w2)
            if drop_plain and self.moe_packed_prefill(lw, for_drop=True):
                freed += 2 * (lw.w13.numel() + lw.w2.numel())
                lw.w13 = lw.w2 = None
        return freed if drop_plain else need

    @staticmethod
    def _pack_experts(w13: torch.Tensor, w2: torch.Tensor) -> tuple:
        """(w13 gate/up-interleaved, w2) packed per expert, all experts in one launch each."""
        E, N13, K13 = w13.shape
        _, N2, K2 = w2.shape
        p13 = torch.empty(E, N13 * K13, dtype=w13.dtype, device=w13.device)
        p2 = torch.empty(E, -(-N2 // 128) * 128 * K2, dtype=w2.dtype, device=w2.device)
        torch.ops.hipserve.pack_decode_weight(p13, w13.contiguous(), True)
        torch.ops.hipserve.pack_decode_weight(p2, w2.contiguous(), False)
        return p13, p2

    def _route(self, x: torch.Tensor, lw, k: int):
        """(weights [T, k] fp32, expert ids [T, k] int32) of the top-k softmax over the
        router logits x @ router^T. When the start-up timing picked the decode GEMM for the
        router at this row count, its fp32 split-K partials go straight into the top-k
        kernel, which sums and rounds them as splitk_reduce would (bit-identical, one
        launch fewer per MoE layer)."""
        op = torch.ops.hipserve
        T, dev = x.shape[0], x.device
        w = torch.empty(T, k, dtype=torch.float32, device=dev)
        ids = torch.empty(T, k, dtype=torch.int32, device=dev)
        fc = (gemm.fused_choice(T, lw.router)
              if x.is_cuda and x.stride(1) == 1 and x.stride(0) % 8 == 0 else None)
        if fc is not None:
            ws, S = gemm.gemm_partial(x, lw.router, fc)
            op.moe_topk_softmax(w, ids, ws, k, self.cfg.norm_topk_prob, S)
        else:
            op.moe_topk_softmax(w, ids, gemm.linear(x, lw.router), k, self.cfg.norm_topk_prob)
        return w, ids

    def _route_align(self, x: torch.Tensor, lw, tile: int, ends: bool = False):
        """Routing (``_route``) and the expert-sorted slot table padded to whole ``tile``-row
        tiles (moe_align; ``ends``: with its per-expert end offsets output): (weights, slots,
        tile_expert, ntiles, pair_slot, cap), ``cap`` the slot count the buffers are sized to."""
        E, k = self.num_local_experts, self.cfg.num_experts_per_tok
        P, dev = x.shape[0] * k, x.device
        cap = -(-(P + E * (tile - 1)) // tile) * tile
        w, ids = self._route(x, lw, k)
        slots = torch.empty(cap, dtype=torch.int32, device=dev)
        tile_expert = torch.empty(cap // tile, dtype=torch.int32, device=dev)
        ntiles = torch.empty(1, dtype=torch.int32, device=dev)
        pair_slot = torch.empty(P, dtype=torch.int32, device=dev)
        extra = (torch.empty(E, dtype=torch.int32, device=dev),) if ends else ()
        # pairs of experts outside [expert_lo, expert_lo + E) (another rank's) take no slot
        torch.ops.hipserve.moe_align(ids, E, tile, slots, tile_expert, ntiles, pair_slot, *(extra or (None,)),
                                     self.expert_lo)
        return w, slots, tile_expert, ntiles, pair_slot, cap

    def _decode_tile(self, P: int) -> int:  # row tile of the streaming expert GEMMs for P (token, expert) pairs
        E = self.num_local_experts
        return 16 if P <= 8 * E else 32 if P <= 32 * E else 64

    def _combine(self, out: torch.Tensor, y: torch.Tensor, S: int, w, pair_slot, k: int, tail=None):
        """Weighted combine of a token's k expert rows (bf16 ``y`` [slots, H] when S == 0,
        fp32 split-K partials [S, slots, H] else) into ``out``. With ``tail`` = (norm
        output, residual, norm weight) the one-kernel combine + residual add + next-layer
        RMSNorm instead (bit-identical to combine then fused_add_rmsnorm): writes the norm
        output and the residual in place, returns None."""
        op = torch.ops.hipserve
        if tail is not None:
            # TP = 1 only: the fused tail reads every pair's row (no skipped pairs)
            assert self.num_local_experts == self.cfg.num_experts, "moe_combine_add_rmsnorm with expert sharding"
            xn, residual, nw = tail
            op.moe_combine_add_rmsnorm(xn, residual, y, S, w, pair_slot, k, nw, self.cfg.rms_norm_eps)
            return None
        if S > 0:
            op.moe_combine_partial(out, y, w, pair_slot, k)
        else:
            op.moe_combine(out, y, w, pair_slot, k)
        return out

    def moe(self, x: torch.Tensor, lw, tail=None) -> torch.Tensor | None:
        """Sparse MoE: softmax over the E router logits, top-k experts, weights
        renormalised over the k (Mixtral; Qwen3-MoE when ``norm_topk_prob``).

        On the GPU every batch runs one of the graph-capturable kernel paths:
        ``moe_hip`` (the weight-streaming expert decode GEMM; decode batches, and
        prefill batches below the start-up-timed crossover ``moe_packed_from_tokens``),
        ``moe_quant`` (decode batches on quantised experts) or ``moe_grouped`` (the
        packed-layout one-launch grouped GEMM); with ``tail`` they return None (see
        ``_combine``). The per-expert loop at the end is the CPU reference path only."""
        cfg = self.cfg
        k = cfg.num_experts_per_tok
        T = x.shape[0]
        P = T * k
        hip = self.ops.name == "hip"
        if lw.w13 is not None and not isinstance(lw.w13, torch.Tensor):  # quantised experts (ops/quant.py QuantMoE)
            if P <= MOE_KERNEL_MAX_PAIRS:
                return self.moe_quant(x, lw, tail)
            if (hip and self._moe_packed_shape_ok() and lw.w13.dense is None
                    and self.moe_prefill_choice(T) == "packed"):
                # experts dequantised straight into the packed layout, then the one-launch grouped GEMMs
                packed = (Q.moe_packed_scratch(lw.w13, 0, True), Q.moe_packed_scratch(lw.w2, 1, False))
                return self.moe_grouped(x, ExpertWeights(lw.router, moe_packed=packed), tail)
            lw = ExpertWeights(lw.router, Q.moe_dense(lw.w13, 0), Q.moe_dense(lw.w2, 1))
        if hip:
            kernel_ok = (cfg.num_experts <= 128 and cfg.hidden_size % 256 == 0 and self.inter % 256 == 0
                         and (lw.w13 is not None or lw.moe_packed is not None))
            grouped_ok = self.moe_packed_prefill(lw)
            if kernel_ok and (P <= MOE_KERNEL_MAX_PAIRS or not grouped_ok
                              or (P <= MOE_KERNEL_MAX_ROWS_PER_EXPERT * self.num_local_experts
                                  and self.moe_prefill_choice(T) == "hip")):
                return self.moe_hip(x, lw, tail)
            if grouped_ok:
                return self.moe_grouped(x, lw, tail)
            raise NotImplementedError(f"MoE shape (E={cfg.num_experts}, H={cfg.hidden_size}, I={self.inter}) "
                                      "has no gfx950 expert kernel")
        logits = F.linear(x, lw.router).float()
        w, idx = torch.topk(torch.softmax(logits, dim=-1), k, dim=-1)
        if cfg.norm_topk_prob:
            w = w / w.sum(-1, keepdim=True)
        out = torch.zeros(T, cfg.hidden_size, device=x.device, dtype=torch.float32)
        flat_idx = idx.reshape(-1)
        flat_tok = torch.arange(T, device=x.device).repeat_interleave(k)
        flat_w = w.reshape(-1)
        order = torch.argsort(flat_idx)
        counts = torch.bincount(flat_idx, minlength=cfg.num_experts).tolist()
        start = 0
        lo = self.expert_lo
        for e, n in enumerate(counts):
            sel = order[start:start + n]
            start += n
            if n == 0 or not lo <= e < lo + self.num_local_experts:  # expert sharding: this rank's experts only
                continue
            toks = flat_tok[sel]
            gu = F.linear(x[toks], lw.w13[e - lo])
            act = torch.empty(n, self.inter, device=x.device, dtype=x.dtype)
            self.ops.silu_and_mul(act, gu)
            y = F.linear(act, lw.w2[e - lo]).float() * flat_w[sel].unsqueeze(-1)
            out.index_add_(0, toks, y)
        return out.to(x.dtype)

    def _moe_decode_ok(self, lw) -> bool:
        """Shapes the expert decode GEMM (decode_gemm.hip kMoe) takes: K = H for w13
        (one K slice of 256 * one of DG_MOE_STEPS) and K = I/TP for w2 (split over K)."""
        H, I = self.cfg.hidden_size, self.inter
        return ((H // 256) in DG_MOE_STEPS and H % 256 == 0 and I % 256 == 0 and (2 * I) % 128 == 0
                and self._moe_w2_splits(I, 1, 1) > 0)

    @staticmethod
    def _moe_w2_splits(K: int, ntiles: int, active: int) -> int:
        """Split-K factor of the w2 expert GEMM: the fewest K slices (of 256 * one of
        DG_MOE_STEPS) that give >= 1024 workgroups over the active expert tiles."""
        ks = K // 256
        opts = sorted(ks // st for st in DG_MOE_STEPS if ks % st == 0)
        if not opts:
            return 0
        for S in opts:
            if ntiles * S * active >= 1024:
                return S
        return opts[-1]

    def moe_grouped(self, x: torch.Tensor, lw, tail=None) -> torch.Tensor | None:
        """Prefill-sized MoE: routing (top-k kernel), expert-sorted slots padded to the
        GEMM's row tile (moe_align), then the two expert GEMMs as ONE launch each on the
        packed expert layout (prefill_gemm_packed.hip kGroup: expert ids read on the
        device, no host round trip, graph-capturable; the token rows gathered through the
        slot table inside the first GEMM's X loads, SiLU-GLU in its epilogue), and the
        weighted combine (moe_combine). Row-major experts without a packed copy (tests)
        are packed into a scratch first."""
        op = torch.ops.hipserve
        k, H = self.cfg.num_experts_per_tok, self.cfg.hidden_size
        T, dev = x.shape[0], x.device
        p13, p2 = lw.moe_packed if lw.moe_packed is not None else self._pack_experts(lw.w13, lw.w2)
        w, slots, tile_expert, ntiles, pair_slot, cap = self._route_align(x, lw, 128 * gemm.PW_WM, ends=True)
        act = torch.empty(cap, self.inter, dtype=x.dtype, device=dev)
        # the first GEMM reads its token rows through the slot table (moe_gather fused)
        op.prefill_gemm_packed_grouped(act, x, p13, 2 * self.inter, 2, tile_expert, ntiles, gemm.PW_WM, gemm.PW_RW,
                                       slots, k)
        y = torch.empty(cap, H, dtype=x.dtype, device=dev)
        op.prefill_gemm_packed_grouped(y, act, p2, H, 0, tile_expert, ntiles, gemm.PW_WM, gemm.PW_RW)
        return self._combine(torch.empty(T, H, dtype=x.dtype, device=dev), y, 0, w, pair_slot, k, tail)

    # prefill-sized MoE batches: the packed one-launch grouped GEMM (``moe_grouped``) or the
    # weight-streaming expert kernel (``moe_hip``). ``auto``: by the start-up timing of the
    # layer's expert shape at several token counts (``tune_moe_prefill``): the grouped GEMM
    # from ``moe_packed_from_tokens`` tokens up, the streaming kernel below (its 128-row
    # tiles are mostly padding when 128 experts share a few hundred tokens). ``1`` / ``0``
    # force the grouped GEMM / the streaming kernel. hipBLASLt's grouped GEMM
    # (torch._grouped_mm) lost to the packed kernel on every shipped MoE config (Mixtral
    # 4.82 vs 5.10 ms, Qwen3-30B-A3B 1.52 vs 5.17 ms per layer at 16K tokens,
    # profiles/r5_bench_mixtral_gather_fused.json, r5_bench_q3int8_align_multiblock.json)
    # and read its group offsets on the host: removed
    MOE_PACKED_PREFILL = os.environ.get("HIPSERVE_MOE_PACKED_PREFILL", "auto")
    moe_prefill_path: str | None = None  # "hip" | "packed" at the timed budget, set by tune_moe_prefill
    moe_packed_from_tokens: int = 0     # "packed": the grouped GEMM from this many tokens up

    def moe_prefill_choice(self, T: int) -> str:
        """'packed' (grouped GEMM) or 'hip' (streaming expert kernel) for a T-token batch."""
        mode = self.MOE_PACKED_PREFILL
        if mode in ("0", "1"):
            return "packed" if mode == "1" else "hip"
        if self.moe_prefill_path == "packed" and T >= self.moe_packed_from_tokens:
            return "packed"
        if self.moe_prefill_path is None:  # untimed (tests, CPU): the grouped GEMM above the kernel row limit
            E, k = self.num_local_experts, self.cfg.num_experts_per_tok
            return "packed" if T * k > MOE_KERNEL_MAX_ROWS_PER_EXPERT * E else "hip"
        return "hip"

    def _moe_packed_shape_ok(self) -> bool:
        return (self.cfg.hidden_act == "silu" and self.cfg.hidden_size % 256 == 0 and self.inter % 256 == 0
                and (2 * self.inter) % 128 == 0 and hasattr(torch.ops.hipserve, "prefill_gemm_packed_grouped"))

    def moe_packed_prefill(self, lw, for_drop: bool = False) -> bool:
        """The packed-layout grouped GEMM can run this layer's prefill: SiLU-GLU experts,
        K of both GEMMs % 256, a packed copy (or row-major experts to pack from)."""
        if not self._moe_packed_shape_ok() or (lw.moe_packed is None and lw.w13 is None):
            return False
        if for_drop:
            return self.MOE_PACKED_PREFILL != "0" and lw.moe_packed is not None
        return True

    @torch.inference_mode()
    def tune_moe_prefill(self, T: int) -> dict | None:
        """Start-up timing of one MoE layer's prefill on random bf16 experts of the layer's
        shape through the model's own paths, the weight-streaming expert kernel
        (``moe_hip``, where its row limit allows) vs the packed one-launch grouped GEMM
        (``moe_grouped``), at ``T`` tokens and at halvings of it down to the decode
        kernels' pair limit. Sets ``moe_prefill_path`` (the winner at T) and
        ``moe_packed_from_tokens`` (the smallest timed count from which the grouped GEMM
        wins at every larger count). Cached per device and kernel build."""
        from ..ops import tune_cache as TC

        cfg = self.cfg
        lw = next((lw for lw in self.layers if lw.router is not None), None)
        if (lw is None or not self._moe_packed_shape_ok() or self.MOE_PACKED_PREFILL != "auto"
                or getattr(self.ops, "name", "") != "hip" or self.device.type != "cuda" or cfg.num_experts > 128):
            return None
        # E: the experts this rank holds (all of them unless expert-sharded); the router stays global
        E, k, H, I = self.num_local_experts, cfg.num_experts_per_tok, cfg.hidden_size, self.inter
        quant = lw.w13 is not None and not isinstance(lw.w13, torch.Tensor)
        if not quant and lw.moe_packed is None and lw.w13 is None:
            return None
        key = [E, k, H, I, T, quant, "v2"] + ([cfg.num_experts] if E != cfg.num_experts else [])
        hit = TC.get(self.device, "moe_prefill", key)
        if hit is not None:
            self.moe_prefill_path, self.moe_packed_from_tokens = hit["path"], hit["packed_from_tokens"]
            return dict(hit, cached=True)
        dev = self.device
        g = torch.Generator(device=dev).manual_seed(E * H + I)
        w13 = (torch.randn(E, 2 * I, H, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        w2 = (torch.randn(E, H, I, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        packed = self._pack_experts(w13, w2)
        # routed over all experts, so the local pair counts are those of a real step
        router = (torch.randn(cfg.num_experts, H, device=dev, generator=g) * 0.3).to(torch.bfloat16)
        syn = ExpertWeights(router, w13, w2, packed)
        counts = []
        t = T
        while t * k > MOE_KERNEL_MAX_PAIRS and len(counts) < 5:
            counts.append(t)
            t //= 2
        rows = []
        for t in counts:
            x = torch.randn(t, H, device=dev, generator=g).to(torch.bfloat16)
            # quantised experts dequantise once per step on either path: only the GEMMs are timed
            row = {"tokens": t, "packed_ms": round(pgemm._time(lambda i: self.moe_grouped(x, syn), reps=2), 3)}
            if not quant and t * k <= MOE_KERNEL_MAX_ROWS_PER_EXPERT * E and self._moe_decode_ok(syn):
                row["hip_ms"] = round(pgemm._time(lambda i: self.moe_hip(x, syn), reps=2), 3)
            rows.append(row)
        del w13, w2, packed, syn
        torch.cuda.empty_cache()
        wins = [r.get("hip_ms") is None or r["packed_ms"] < r["hip_ms"] for r in rows]
        best = "packed" if not rows or wins[0] else "hip"
        frm = T
        for r, w_ in zip(rows, wins):  # counts descend: the grouped GEMM's run of wins from the top
            if not w_:
                break
            frm = r["tokens"]
        if best == "packed" and len(rows) and all(wins):
            frm = 0  # wins down to the pair limit: every prefill-sized batch
        self.moe_prefill_path, self.moe_packed_from_tokens = best, frm
        r = {"E": E, "E_global": cfg.num_experts, "H": H, "I": I, "tokens": T, "quant": quant, "path": best,
             "packed_from_tokens": frm, "timing": rows}
        TC.put(self.device, "moe_prefill", key, r)
        TC.flush()
        log.info("MoE prefill expert GEMMs: %s", r)
        return r

    def moe_hip(self, x: torch.Tensor, lw, tail=None) -> torch.Tensor | None:
        """Graph-capturable MoE on the gfx950 kernels (decode-sized batches): top-k
        routing, expert-sorted 16/32/64-row tiles, two gathered MFMA GEMMs with the
        SiLU*up in between, weighted combine. No host synchronisation.

        The expert GEMMs are the decode GEMM in its MoE mode (weight-streaming:
        128 weight rows x one expert tile per workgroup, x tile staged in LDS):
        with packed weights (``pack_moe_weights``) the SiLU-GLU runs in the w13
        epilogue, and w2 writes split-K fp32 partials that the combine sums."""
        op = torch.ops.hipserve
        cfg = self.cfg
        E, k, H = self.num_local_experts, cfg.num_experts_per_tok, cfg.hidden_size
        T, dev = x.shape[0], x.device
        P = T * k
        tile = self._decode_tile(P)
        w, slots, tile_expert, _, pair_slot, cap = self._route_align(x, lw, tile)
        out = torch.empty(T, H, dtype=x.dtype, device=dev)
        if self._moe_decode_ok(lw):
            packed = lw.moe_packed is not None
            act = torch.empty(cap, self.inter, dtype=x.dtype, device=dev)
            if packed:
                op.moe_decode_gemm(act, x, lw.moe_packed[0], slots, tile_expert, tile, k, 2 * self.inter, 1,
                                   True, True)
            else:
                gu = torch.empty(cap, 2 * self.inter, dtype=x.dtype, device=dev)
                op.moe_decode_gemm(gu, x, lw.w13, slots, tile_expert, tile, k, 2 * self.inter, 1, False, False)
                self.ops.silu_and_mul(act, gu)
            active = min(E, cap // tile, P)
            S = self._moe_w2_splits(self.inter, -(-H // 128), active)
            w2 = lw.moe_packed[1] if packed else lw.w2
            if S == 1:  # one K slice: bf16 expert outputs, no fp32 partial slab
                y = torch.empty(cap, H, dtype=x.dtype, device=dev)
                op.moe_decode_gemm(y, act, w2, slots, tile_expert, tile, 0, H, 1, packed, False)
                return self._combine(out, y, 0, w, pair_slot, k, tail)
            ws = torch.empty(S, cap, H, dtype=torch.float32, device=dev)
            op.moe_decode_gemm(ws, act, w2, slots, tile_expert, tile, 0, H, S, packed, False)
            return self._combine(out, ws, S, w, pair_slot, k, tail)
        gu = torch.empty(cap, 2 * self.inter, dtype=x.dtype, device=dev)
        op.moe_gemm(gu, x, lw.w13, slots, tile_expert, tile, k)
        act = torch.empty(cap, self.inter, dtype=x.dtype, device=dev)
        self.ops.silu_and_mul(act, gu)
        y = torch.empty(cap, H, dtype=x.dtype, device=dev)
        op.moe_gemm(y, act, lw.w2, slots, tile_expert, tile, 0)
        return self._combine(out, y, 0, w, pair_slot, k, tail)

    def moe_quant(self, x: torch.Tensor, lw, tail=None) -> torch.Tensor | None:
        """Decode-sized MoE on quantised experts (``QuantMoE``: INT8 / FP8 checkpoints, or
        the GGUF blocks Q4_0 / Q4_1 / Q8_0 / Q4_K / Q5_K / Q6_K of a MoE GGUF file; w13 and
        w2 may differ in format, Q4_K_M puts down experts in Q6_K): routing and
        expert-sorted tiles as ``moe_hip``, then the dequant-MFMA expert GEMM in its
        MoE mode (gathered token rows, one expert's weight stream per workgroup) for
        w13, SiLU-GLU, and w2 (split over K into fp32 partials summed by the
        weighted combine). No host synchronisation (graph-capturable)."""
        op = torch.ops.hipserve
        cfg = self.cfg
        E, k, H = self.num_local_experts, cfg.num_experts_per_tok, cfg.hidden_size
        T, dev = x.shape[0], x.device
        P = T * k
        tile = self._decode_tile(P)
        w, slots, tile_expert, _, pair_slot, cap = self._route_align(x, lw, tile)
        w13, w2 = lw.w13, lw.w2
        f32 = torch.empty(0, dtype=torch.float32, device=dev)
        act = torch.empty(cap, w13.N // 2, dtype=x.dtype, device=dev)
        if tile <= 32 and (w13.N // 2) % 16 == 0:  # GLU in the w13 epilogue (bit-identical)
            glu = 2 if cfg.hidden_act == "gelu_tanh" else 1
            op.qmoe_gemm(act, f32, x, w13.q, w13.rs, w13.kqt, w13.N, w13.K, slots, tile_expert, tile, k, 1,
                         w13.kmajor, glu)
        else:
            gu = torch.empty(cap, w13.N, dtype=x.dtype, device=dev)
            op.qmoe_gemm(gu, f32, x, w13.q, w13.rs, w13.kqt, w13.N, w13.K, slots, tile_expert, tile, k, 1,
                         w13.kmajor)
            self.act_and_mul(act, gu)
        out = torch.empty(T, H, dtype=x.dtype, device=dev)
        active = min(E, cap // tile, P)
        S = self._moe_w2_splits(w2.K, -(-H // 128), active)
        if S <= 1:
            y = torch.empty(cap, H, dtype=x.dtype, device=dev)
            op.qmoe_gemm(y, f32, act, w2.q, w2.rs, w2.kqt, w2.N, w2.K, slots, tile_expert, tile, 0, 1, w2.kmajor)
            return self._combine(out, y, 0, w, pair_slot, k, tail)
        ws = torch.empty(S, cap, H, dtype=torch.float32, device=dev)
        S = op.qmoe_gemm(out, ws, act, w2.q, w2.rs, w2.kqt, w2.N, w2.K, slots, tile_expert, tile, 0, S, w2.kmajor)
        return self._combine(out, ws[:S], S, w, pair_slot, k, tail)
