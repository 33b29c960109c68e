"""Perplexity of a token stream under a served model, in the manner of llama.cpp's
``llama-perplexity``: the stream is cut into non-overlapping windows of ``--ctx`` tokens,
each window is scored as one prompt (``LLMEngine.score``: the log-prob of every token but
the window's first, given the tokens before it in the window), and the mean negative
log-likelihood over all scored tokens and its exponential are reported. A last window
shorter than ``--ctx`` is scored too when it holds at least two tokens.

    python tools/perplexity.py --model llama-3-8b --load-format dummy --tokens ids.npy
    python tools/perplexity.py --model /models/m.gguf --text wiki.test.raw --ctx 512 --json ppl.json

The engine flags are the server's (``python -m hipserve.server --help``). Without a GPU the
tool stops unless ``--device cpu`` asks for the fp32 reference engine. Single process:
``--tensor-parallel-size`` above 1 is refused.
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH = 64  # windows handed to the engine at once


def windows(ids, ctx: int) -> list[list[int]]:
    return [w for w in (list(map(int, ids[i:i + ctx])) for i in range(0, len(ids), ctx)) if len(w) >= 2]


def perplexity(engine, ids, ctx: int | None = None) -> dict:
    """{"nll", "ppl", "tokens", "windows", "ctx"} of the token stream ``ids``."""
    limit = engine.max_model_len - 1  # the longest prompt that leaves room for the one sampled token
    ctx = limit if ctx is None else ctx
    if not 2 <= ctx <= limit:
        raise ValueError(f"--ctx must be in [2, {limit}] (max_model_len - 1)")
    ws = windows(ids, ctx)
    if not ws:
        raise ValueError("the stream holds fewer than two tokens")
    total, count = 0.0, 0
    for i in range(0, len(ws), BATCH):
        for lp in engine.score(ws[i:i + BATCH]):
            total -= float(np.sum(lp, dtype=np.float64))
            count += len(lp)
    nll = total / count
    return {"nll": nll, "ppl": math.exp(nll), "tokens": count, "windows": len(ws), "ctx": ctx}


def main(argv=None) -> int:
    import torch

    from hipserve.server.cli import build_parser, config_from_args

    ap = build_parser("perplexity")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--tokens", help=".npy file of token ids")
    src.add_argument("--text", help="text file, tokenised with the model's tokenizer")
    ap.add_argument("--ctx", type=int, default=None, help="window length in tokens (default: max_model_len - 1)")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args(argv)
    if a.device != "cpu" and not torch.cuda.is_available():
        print("perplexity: no GPU is visible; pass --device cpu for the fp32 reference engine", file=sys.stderr)
        return 2
    if a.tensor_parallel_size != 1:
        print("perplexity: single process only (--tensor-parallel-size 1)", file=sys.stderr)
        return 2
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    cfg = config_from_args(a)
    if cfg.device == "cpu" and cfg.dtype in ("bfloat16", "bf16"):
        cfg = cfg.replace(dtype="float32")
    engine = LLMEngine(cfg, tp=TPGroup() if cfg.device == "cpu" else None)
    try:
        if a.tokens:
            ids = np.load(a.tokens, allow_pickle=False).reshape(-1)
        else:
            with open(a.text, encoding="utf-8") as f:
                ids = engine.tokenizer.encode(f.read())
        res = {"model": cfg.model_name, **perplexity(engine, ids, a.ctx)}
    except ValueError as e:
        print(f"perplexity: {e}", file=sys.stderr)
        return 2
    finally:
        engine.shutdown()
    print(f"tokens {res['tokens']}  windows {res['windows']} x {res['ctx']}  "
          f"mean NLL {res['nll']:.6f}  perplexity {res['ppl']:.4f}")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
