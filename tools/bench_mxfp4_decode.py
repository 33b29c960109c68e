#!/usr/bin/env python3
"""MXFP4 W4A8 GEMM (mxfp4.hip) against its two comparison points at decode row counts, on
COLD weights, Llama-3-8B projection shapes: the FP8 W8A8 GEMM (fp8_decode.hip: the same
structure at twice the bytes) and the INT4 body of the quantised decode GEMM (gguf_mfma.hip:
the same bytes, dequantised in VALU into f16 MFMAs). Each kernel at its best K split, fp32
partials, timed in hipGraphs whose launches rotate over copies of the weight totalling
>= 768 MiB (beyond the 256 MiB MALL), as ops/quant.py tune_splits does. One JSON line per
(proj, M, kernel): microseconds and TB/s of weight bytes.
usage: python tools/bench_mxfp4_decode.py [--m 1 16 64 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hipserve.ops import load_library, pgemm, quant as Q

SHAPES = {"qkv": ([4096, 1024, 1024], 4096), "o": ([4096], 4096), "gate_up": ([14336, 14336], 4096),
          "down": ([4096], 14336)}


def _weights(kind, rows, K, dev, g):
    parts = []
    for n in rows:
        if kind == "mxfp4":
            parts.append(Q.QuantPart.from_mxfp4(
                torch.randint(0, 256, (n, K // 2), device=dev, generator=g, dtype=torch.uint8),
                torch.randint(119, 122, (n, K // 32), device=dev, generator=g, dtype=torch.uint8), dev))
        elif kind == "fp8":
            w = (torch.rand(n, K, device=dev, generator=g) * 2 - 1) * 0.05
            s = w.abs().amax(1, keepdim=True) / 448.0
            parts.append(Q.QuantPart.from_fp8((w / s).to(torch.float8_e4m3fn), s, dev))
        else:
            u = torch.randint(0, 16, (n, K), device=dev, generator=g, dtype=torch.uint8)
            parts.append(Q.QuantPart.from_int4(u, torch.full((n, K // 128), 0.00375, device=dev), None, dev))
    return Q.QuantWeight(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16, 64, 256])
    a = ap.parse_args()
    load_library()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    empty = torch.empty(0, dtype=torch.bfloat16, device=dev)
    for name, (rows, K) in SHAPES.items():
        nsb = K // 256
        for kind in ("mxfp4", "fp8", "int4"):
            w = _weights(kind, rows, K, dev, g)
            nbytes = sum(p.q.numel() for p in w.parts)
            ncopy = max(1, -(-Q.COLD_BYTES // nbytes))
            copies = [[p.q for p in w.parts]] + [[p.q.clone() for p in w.parts] for _ in range(ncopy - 1)]
            for M in a.m:
                if kind == "int4" and M > Q.MAX_FUSED_M:
                    continue  # the dequant-MFMA decode body serves up to 64 rows
                x = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
                xq, xs = pgemm.act_quant(x)
                if kind == "int4":
                    cands = sorted({Q._actual_splits(nsb, s) for s in (1, 2, 4, 8, 16, 32) if s <= nsb})
                else:
                    cands = [S for S in Q._f8_valid_splits(w)]
                best = None
                for S in cands:
                    ws = torch.empty(S * M * w.N, dtype=torch.float32, device=dev)
                    if kind == "mxfp4":
                        fn = lambda qs: torch.ops.hipserve.mxfp4_gemm(ws, xq, xs, qs, [p.N for p in w.parts], S)  # noqa: E731
                    elif kind == "fp8":
                        fn = lambda qs: torch.ops.hipserve.fp8_decode_gemm(ws, xq, xs, qs, [p.rs for p in w.parts], S)  # noqa: E731
                    else:
                        fn = lambda qs: Q._launch_v2(empty, ws, x, w, S, None, qs)  # noqa: E731
                    t = Q._graph_time_us(lambda: [fn(qs) for qs in copies], reps=max(1, 10 // ncopy)) / ncopy
                    if best is None or t < best[1]:
                        best = (S, t)
                    del ws
                print(json.dumps({"proj": name, "M": M, "kernel": kind, "splits": best[0], "us": round(best[1], 2),
                                  "weight_MB": round(nbytes / 1e6, 2), "TBps": round(nbytes / 1e6 / best[1], 3)}),
                      flush=True)
            del w, copies
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
