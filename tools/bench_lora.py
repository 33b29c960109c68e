#!/usr/bin/env python3
"""Multi-LoRA kernels at Llama-3-8B projection shapes: the shrink + expand pair next to the
base projection's GEMM (torch.mm, bf16), timed with device events, the variants alternating
in one loop. A, B and W are rotated over 6 copies; the copies of A and B alone (tens of MB)
fit the 256 MB MALL, so how cold they are rests on the base GEMM's W traffic (190 MB to
1.4 GB over the copies) that runs between two LoRA pairs, not on the rotation.

    python tools/bench_lora.py [--iters 30]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipserve.ops import KernelOps  # noqa: E402

# projection -> (K, slice widths)
SHAPES = {"qkv": (4096, (4096, 1024, 1024)), "o": (4096, (4096,)), "gate|up": (4096, (14336, 14336)),
          "down": (14336, (4096,))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args(argv)
    ops, dev = KernelOps(), torch.device("cuda", 0)
    slots, copies = 8, 6
    print("proj M rank adapters | lora pair us | base GEMM us | A+B bytes touched | GB/s over the pair")
    for proj, (K, widths) in SHAPES.items():
        N = sum(widths)
        W = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) for _ in range(copies)]
        for r in (16, 64):
            R = r * len(widths)
            A = [torch.randn(slots, R, K, device=dev, dtype=torch.bfloat16) for _ in range(copies)]
            B = [torch.randn(slots, N, r, device=dev, dtype=torch.bfloat16) for _ in range(copies)]
            scale = torch.ones(slots, device=dev)
            slices = [(sum(widths[:j]), j * r) for j in range(len(widths))]
            ws = torch.empty(ops.LORA_WS_ROWS * R, device=dev)
            for M, nad in ((1, 1), (16, 1), (16, 8), (64, 1), (64, 8), (8192, 8)):
                x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
                out = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
                t = torch.empty(M, R, device=dev, dtype=torch.bfloat16)
                # 8,192 rows: 8 sequences of 1,024 rows, one adapter each; decode: rows dealt round-robin
                idx = ((torch.arange(M, device=dev) * nad // M) if M > 64 else torch.arange(M, device=dev) % nad).int()
                ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.iters)]
                for i in range(a.iters + 3):
                    e = ev[max(i - 3, 0)]
                    c = i % copies
                    e[0].record()
                    ops.lora_shrink(t, x, A[c], idx, ws)
                    ops.lora_expand(out, t, B[c], scale, idx, slices)
                    e[1].record()
                    torch.mm(x, W[c].t(), out=out)
                    e[2].record()
                torch.cuda.synchronize()
                lora = sorted(e[0].elapsed_time(e[1]) for e in ev)[a.iters // 2] * 1e3
                base = sorted(e[1].elapsed_time(e[2]) for e in ev)[a.iters // 2] * 1e3
                touched = min(nad, M) * (R * K + N * r) * 2
                print(f"{proj} {M} {r} {min(nad, M)} | {lora:.1f} | {base:.1f} | {touched} | {touched / lora / 1e3:.1f}",
                      flush=True)


if __name__ == "__main__":
    main()
