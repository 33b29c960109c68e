#!/usr/bin/env python3
"""Micro-benchmarks of individual hipserve kernels on the GPU (HIP-event timing,
median of N launches). Prints one JSON line per case.

    python tools/bench_ops.py [sample|decode|prefill|gemm|norm|rope|all]
    python tools/bench_ops.py prompt_logprobs        # the prompt-scoring kernel vs top_logprobs vs a copy
    python tools/bench_ops.py prompt_logprobs_step   # cost of prompt_logprobs=1 to an 8 x 1,024 prefill step
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hipserve.ops import KernelOps, reference  # noqa: E402

DEV = "cuda"


def timeit(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1000 for a, b in evs)
    return ts[len(ts) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def graph_time(fn, n=20, reps=5):
    """Device time per call with the calls captured in one hipGraph (how the
    engine's decode step runs them: no host launch cost)."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        ts.append((a, b))
    torch.cuda.synchronize()
    v = sorted(x.elapsed_time(y) for x, y in ts)
    return v[len(v) // 2] * 1000.0 / n


def bench_sample(ops):
    timer = graph_time if os.environ.get("BENCH_GRAPH", "1") == "1" else timeit
    for V, B in [(128256, 64), (128256, 256), (32000, 64), (128256, 1)]:
        logits = (torch.randn(B, V, device=DEV) * 3).to(torch.bfloat16)
        tok = torch.empty(B, dtype=torch.long, device=DEV)
        lp = torch.empty(B, device=DEV)
        for name, t, k, p in [("greedy", 0.0, 0, 1.0), ("temp", 0.8, 0, 1.0), ("top_p", 0.8, 0, 0.95),
                              ("top_k_p", 0.8, 50, 0.95)]:
            temp = torch.full((B,), t, device=DEV)
            tk = torch.full((B,), k, dtype=torch.int32, device=DEV)
            tp = torch.full((B,), p, device=DEV)
            seeds = torch.arange(B, device=DEV)
            steps = torch.zeros(B, dtype=torch.long, device=DEV)
            us = timer(lambda: ops.sample(tok, lp, logits, temp, tk, tp, seeds, steps))
            emit(op="sample", mode=name, V=V, B=B, us=round(us, 1), graph=timer is graph_time)
        # temperature sampling with a min_p cut on every row
        temp = torch.full((B,), 0.8, device=DEV)
        tk = torch.zeros(B, dtype=torch.int32, device=DEV)
        tp = torch.ones(B, device=DEV)
        mp = torch.full((B,), 0.05, device=DEV)
        us = timer(lambda: ops.sample(tok, lp, logits, temp, tk, tp, seeds, steps, min_p=mp))
        emit(op="sample", mode="min_p", V=V, B=B, us=round(us, 1), graph=timer is graph_time)
    # logit_bias_apply: 64 rows, every row with a full 300-entry slot
    V, B, E = 128256, 64, 300
    logits = (torch.randn(B, V, device=DEV) * 3).to(torch.bfloat16)
    ids = torch.stack([torch.randperm(V, device=DEV)[:E] for _ in range(B)]).int()
    vals = torch.rand(B, E, device=DEV) * 2 - 1
    n = torch.full((B,), E, dtype=torch.int32, device=DEV)
    slot = torch.arange(B, dtype=torch.int32, device=DEV)
    us = timer(lambda: ops.logit_bias_apply(logits, slot, ids, vals, n))
    emit(op="logit_bias_apply", V=V, B=B, entries=E, us=round(us, 1), graph=timer is graph_time)


def softcaps():
    """BENCH_SOFTCAP="0,50": the attention benches time every shape once per value, in the same
    run on the same tensors (0 = the uncapped kernel, > 0 = Gemma-2 score soft-capping)."""
    return [float(x) for x in os.environ.get("BENCH_SOFTCAP", "0").split(",")]


def bench_decode(ops):
    D = int(os.environ.get("BENCH_D", "128"))  # head_dim: 64 / 96 / 128 / 256
    parts = [int(x) for x in os.environ.get("DECODE_PARTS", "512").split(",")]
    bss = [int(x) for x in os.environ.get("DECODE_BS", "16").split(",")]  # KV block sizes
    shapes = [(64, 1152, 32, 8), (64, 1280, 32, 8), (256, 1152, 32, 8), (1, 4096, 32, 8), (64, 4096, 64, 8)]
    if os.environ.get("DECODE_SHAPES"):  # "BxCTXxNQxNKV,..." e.g. 64x1152x32x4 (Qwen3-30B-A3B)
        shapes = [tuple(int(v) for v in sh.split("x")) for sh in os.environ["DECODE_SHAPES"].split(",")]
    for (B, ctx, nq, nkv), part, bs in [(c, p, b) for c in shapes for p in parts for b in bss]:
        mb = math.ceil(ctx / bs) + 1
        nblocks = B * mb
        # DECODE_COLD=1: rotate over enough KV copies (> 2x the 256 MB MALL) that every
        # call streams cold K / V, as in the engine (one step touches every layer's KV)
        # DECODE_KV=fp8: e4m3 cache (--kv-cache-dtype fp8), half the bytes
        f8 = os.environ.get("DECODE_KV") == "fp8"
        kvt = torch.float8_e4m3fn if f8 else torch.bfloat16
        byts = 2 * B * ctx * nkv * D * (1 if f8 else 2)
        ncopy = max(1, min(8, -(-(768 << 20) // byts))) if os.environ.get("DECODE_COLD") == "1" else 1
        kcs = [torch.randn(nblocks, nkv, bs, D, device=DEV).to(kvt) for _ in range(ncopy)]
        vcs = [torch.randn(nblocks, nkv, D, bs, device=DEV).to(kvt) for _ in range(ncopy)]
        bt = torch.randperm(nblocks, device=DEV).int().view(B, mb)
        cl = torch.full((B,), ctx, device=DEV, dtype=torch.int32)
        q = torch.randn(B, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
        mp = math.ceil(mb * bs / part)
        to = torch.empty(B, nq, mp, D, device=DEV)
        tm = torch.empty(B, nq, mp, 2, device=DEV)
        out = torch.empty(B, nq * D, device=DEV, dtype=torch.bfloat16)
        it = [0]
        for cap in softcaps():
            def call():
                i = it[0] % ncopy
                it[0] += 1
                ops.paged_decode(out, q, kcs[i], vcs[i], bt, cl, to, tm, nq, nkv, part, 1 / math.sqrt(D), 0, None, cap)

            us = timeit(call)
            emit(op="paged_decode", D=D, kv="fp8" if f8 else "bf16", B=B, ctx=ctx, nq=nq, nkv=nkv, part=part, bs=bs,
                 cold=ncopy > 1, nt=os.environ.get("HIPSERVE_DECODE_NT", "1"), softcap=cap, us=round(us, 1),
                 TBps=round(byts / us / 1e6, 2))
        del kcs, vcs


def bench_prefill(ops):
    D, bs = int(os.environ.get("BENCH_D", "128")), 16  # head_dim 256 runs v1 whatever the version asked for
    shapes = [(1024, 8, 32, 8), (4096, 2, 32, 8), (8192, 1, 32, 8), (1024, 8, 8, 1)]
    if os.environ.get("BENCH_PREFILL_LONG"):
        shapes = [(1024, 8, 32, 8), (8192, 1, 32, 8), (32768, 1, 32, 8)]
    if os.environ.get("PREFILL_SHAPES"):  # "SxNSEQxNQxNKV,..." e.g. 1024x8x16x4
        shapes = [tuple(int(v) for v in sh.split("x")) for sh in os.environ["PREFILL_SHAPES"].split(",")]
    vers = os.environ.get("BENCH_PREFILL_VERS", "v2w4,v2w8,v1").split(",")
    for S, nseq, nq, nkv in shapes:
        mb = S // bs
        kvt = torch.float8_e4m3fn if os.environ.get("DECODE_KV") == "fp8" else torch.bfloat16
        kc = torch.randn(nseq * mb, nkv, bs, D, device=DEV).to(kvt)
        vc = torch.randn(nseq * mb, nkv, D, bs, device=DEV).to(kvt)
        bt = torch.arange(nseq * mb, device=DEV).int().view(nseq, mb)
        cu = torch.arange(0, (nseq + 1) * S, S, device=DEV, dtype=torch.int32)
        ctx = torch.full((nseq,), S, device=DEV, dtype=torch.int32)
        tiles = torch.tensor(sorted(((s, r) for s in range(nseq) for r in range(0, S, 128)), key=lambda t: -t[1]),
                             device=DEV, dtype=torch.int32)
        q = torch.randn(nseq * S, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
        out = torch.empty(nseq * S, nq * D, device=DEV, dtype=torch.bfloat16)
        flops = 4 * nseq * (S * S / 2) * D * nq
        for ver in vers:  # v1: per-wave L2 K/V reads (HIPSERVE_PREFILL_ATTN_V1=1)
            os.environ["HIPSERVE_PREFILL_ATTN_V1"] = "1" if ver == "v1" else "0"
            os.environ["HIPSERVE_PREFILL_ATTN_WAVES"] = "8" if ver == "v2w8" else "4"
            for cap in softcaps():
                us = timeit(lambda: ops.prefill_attention(out, q, kc, vc, bt, cu, ctx, tiles, nq, nkv,
                                                          1 / math.sqrt(D), 0, cap), n=10)
                emit(op="prefill_attention", D=D, ver=ver, kv="fp8" if kvt == torch.float8_e4m3fn else "bf16", S=S,
                     nseq=nseq, nq=nq, nkv=nkv, softcap=cap, us=round(us, 1), TFLOPs=round(flops / us / 1e6, 1))
            # BENCH_LIMITS=1: the per-row key limit kernels too (Gemma-3 image blocks), on the same
            # tensors: one 256-token block per sequence at rows [S/2, S/2 + 256), and limits equal
            # to every row's own position ("own": the limit kernel doing the causal kernel's work)
            if os.environ.get("BENCH_LIMITS") == "1" and D in (128, 256) and ver != "v2w4":
                own = torch.arange(S, device=DEV, dtype=torch.int32).repeat(nseq)
                blk = own.clone().view(nseq, S)
                blk[:, S // 2:S // 2 + 256] = S // 2 + 255
                for name, lim in (("own", own), ("block256", blk.view(-1))):
                    us = timeit(lambda: ops.prefill_attention(out, q, kc, vc, bt, cu, ctx, tiles, nq, nkv,
                                                              1 / math.sqrt(D), 0, 0.0, lim), n=10)
                    emit(op="prefill_attention", D=D, ver=ver, kv="fp8" if kvt == torch.float8_e4m3fn else "bf16",
                         S=S, nseq=nseq, nq=nq, nkv=nkv, limits=name, us=round(us, 1),
                         TFLOPs=round(flops / us / 1e6, 1))
        os.environ.pop("HIPSERVE_PREFILL_ATTN_V1", None)


def bench_prefill_chunked(ops):
    """Chunked prefill attention: ``chunk`` new query rows at the end of a ``ctx``-token
    context per sequence (the shape of every step of a long prompt under an 8K token
    budget), TFLOP/s over the causal work of the chunk."""
    D, bs, nq, nkv = 128, 16, 32, 8
    for ctx_len, chunk, nseq in [(32768, 2048, 4), (32768, 8192, 1), (16384, 2048, 4), (8192, 2048, 4)]:
        mb = ctx_len // bs
        kc = torch.randn(nseq * mb, nkv, bs, D, device=DEV, dtype=torch.bfloat16)
        vc = torch.randn(nseq * mb, nkv, D, bs, device=DEV, dtype=torch.bfloat16)
        bt = torch.arange(nseq * mb, device=DEV).int().view(nseq, mb)
        cu = torch.arange(0, (nseq + 1) * chunk, chunk, device=DEV, dtype=torch.int32)
        ctx = torch.full((nseq,), ctx_len, device=DEV, dtype=torch.int32)
        tiles = torch.tensor(sorted(((s, r) for s in range(nseq) for r in range(0, chunk, 128)), key=lambda t: -t[1]),
                             device=DEV, dtype=torch.int32)
        q = torch.randn(nseq * chunk, (nq + 2 * nkv) * D, device=DEV, dtype=torch.bfloat16)
        out = torch.empty(nseq * chunk, nq * D, device=DEV, dtype=torch.bfloat16)
        flops = 4 * nseq * chunk * (ctx_len - chunk / 2) * D * nq
        us = timeit(lambda: ops.prefill_attention(out, q, kc, vc, bt, cu, ctx, tiles, nq, nkv, 1 / math.sqrt(D)), n=10)
        emit(op="prefill_attention_chunked", ctx=ctx_len, chunk=chunk, nseq=nseq, us=round(us, 1),
             TFLOPs=round(flops / us / 1e6, 1))
        del kc, vc, q, out


def bench_gemm(ops):
    for M in (1, 16, 64, 128, 256):
        for N, K, name in [(6144, 4096, "qkv"), (4096, 4096, "o"), (28672, 4096, "gate_up"),
                           (4096, 14336, "down"), (128256, 4096, "lm_head")]:
            x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16)
            us = timeit(lambda: torch.nn.functional.linear(x, w))
            emit(op="hipblaslt_linear", name=name, M=M, N=N, K=K, us=round(us, 1),
                 TBps=round(N * K * 2 / us / 1e6, 2))


def bench_norm(ops):
    for T, H in [(64, 4096), (8192, 4096)]:
        x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
        r = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
        w = torch.randn(H, device=DEV, dtype=torch.bfloat16)
        out = torch.empty_like(x)
        us = timeit(lambda: ops.fused_add_rmsnorm(out, x, r, w, 1e-5))
        emit(op="fused_add_rmsnorm", T=T, H=H, us=round(us, 1), TBps=round(4 * T * H * 2 / us / 1e6, 2))
    # the decode step's other row-norm kernels, at a 64-row batch, inside a graph
    hs = torch.ops.hipserve
    M, S = 64, 4
    for N in (4096, 5376):
        ws = torch.randn(S * M * N, device=DEV) * 0.5
        r = torch.randn(M, N, device=DEV, dtype=torch.bfloat16)
        w = (torch.rand(N, device=DEV) + 0.5).to(torch.bfloat16)
        w2 = (torch.rand(N, device=DEV) + 0.5).to(torch.bfloat16)
        out = torch.empty_like(r)
        table = torch.randn(32000, N, device=DEV, dtype=torch.bfloat16)
        ids = torch.randint(0, 32000, (M,), device=DEV)
        for name, fn in [
            ("splitk_add_rmsnorm", lambda: hs.splitk_add_rmsnorm(out, r, ws, S, w, 1e-5)),
            ("splitk_post_add_rmsnorm", lambda: hs.splitk_post_add_rmsnorm(out, r, ws, S, w, w2, 1e-5)),
            ("embed_rmsnorm", lambda: hs.embed_rmsnorm(out, r, table, ids, None, None, w, 1e-5, 1.0)),
        ]:
            emit(op=name, M=M, N=N, S=S, us=round(graph_time(fn), 2))
    T, k, H = 64, 8, 2048
    cap = T * k + 64
    slot = torch.randperm(cap, device=DEV)[: T * k].int()
    tw = torch.rand(T, k, device=DEV)
    r = torch.randn(T, H, device=DEV, dtype=torch.bfloat16)
    nw = (torch.rand(H, device=DEV) + 0.5).to(torch.bfloat16)
    out = torch.empty_like(r)
    for S in (0, 4):  # bf16 expert rows, fp32 split-K partials
        y = torch.randn(S, cap, H, device=DEV) if S else torch.randn(cap, H, device=DEV).to(torch.bfloat16)
        us = graph_time(lambda: hs.moe_combine_add_rmsnorm(out, r, y, S, tw, slot, k, nw, 1e-6))
        emit(op="moe_combine_add_rmsnorm", T=T, k=k, H=H, S=S, us=round(us, 2))


def bench_rope(ops):
    """The RoPE + KV-write family at the Llama-3-8B shapes, inside a graph: rope_cache (per-token
    kernel at T = 64, tile kernel at T = 8192), the split-K epilogue and the fused decode attention."""
    hs = torch.ops.hipserve
    nq, nkv, D, bs, S = 32, 8, 128, 16, 4
    N = (nq + 2 * nkv) * D
    cs = reference.rope_cos_sin(D, 8192, 500000.0).to(DEV)
    for T in (64, 8192):
        nblk = T // bs + 2
        qkv = torch.randn(T, N, device=DEV, dtype=torch.bfloat16)
        pos = torch.arange(T, device=DEV)
        slots = torch.arange(T, device=DEV) + bs
        kc = torch.zeros(nblk, nkv, bs, D, device=DEV, dtype=torch.bfloat16)
        vc = torch.zeros(nblk, nkv, D, bs, device=DEV, dtype=torch.bfloat16)
        us = graph_time(lambda: ops.rope_cache(qkv, pos, slots, cs, kc, vc, nq, nkv, D, 0))
        emit(op="rope_cache", T=T, us=round(us, 2))
    B, ctx, part = 64, 1152, 512
    nblk = ctx // bs
    ws = torch.randn(S, B, N, device=DEV) * 0.5
    qkv = torch.empty(B, N, device=DEV, dtype=torch.bfloat16)
    kc = torch.randn(B * nblk, nkv, bs, D, device=DEV).to(torch.bfloat16)
    vc = torch.randn(B * nblk, nkv, D, bs, device=DEV).to(torch.bfloat16)
    bt = torch.randperm(B * nblk, device=DEV).int().view(B, nblk)
    cl = torch.full((B,), ctx, device=DEV, dtype=torch.int32)
    pos = (cl - 1).long()
    slots = bt[:, -1].long() * bs + (ctx - 1) % bs
    us = graph_time(lambda: hs.splitk_rope_cache(qkv, ws, S, pos, slots, cs, kc, vc, nq, nkv, D, 0))
    emit(op="splitk_rope_cache", T=B, S=S, us=round(us, 2))
    parts = math.ceil(ctx / part)
    out = torch.empty(B, nq * D, device=DEV, dtype=torch.bfloat16)
    tmp = torch.empty(B, nq, parts, D, device=DEV)
    ml = torch.empty(B, nq, parts, 2, device=DEV)
    us = graph_time(lambda: hs.paged_decode_qkv(out, ws, S, pos, slots, cs, kc, vc, bt, cl, tmp, ml, nq, nkv, part,
                                                D ** -0.5, 0, 0, None, None, None, 1e-6))
    emit(op="paged_decode_qkv", B=B, ctx=ctx, S=S, us=round(us, 2))


def bench_prompt_logprobs(ops):
    """One full lm_head chunk (1,046 x 128,256 bf16, 268 MB: not cache resident): the
    one-pass kernel at nreq 0 / 1 / 5 / 20 on all rows, the top_logprobs kernel on the same
    buffer at n = 1 / 5 and a plain device copy, taken in alternation (one launch of each
    per round, median over the rounds). TB/s is of the logits bytes (x2 for the copy)."""
    R, V, K, rounds = 1046, 128256, 20, 12
    logits = torch.empty(R, V, device=DEV, dtype=torch.bfloat16)
    for a in range(0, R, 128):  # in slices: no fp32 copy of the whole buffer
        logits[a:a + 128] = (torch.randn(min(128, R - a), V, device=DEV) * 3).to(torch.bfloat16)
    dst = torch.empty_like(logits)
    tg = torch.randint(0, V, (R,), device=DEV, dtype=torch.int32)
    lp, rank = torch.empty(R, device=DEV), torch.empty(R, dtype=torch.int32, device=DEV)
    ids, top = torch.empty(R, K, dtype=torch.int32, device=DEV), torch.empty(R, K, device=DEV)
    nr = {n: torch.full((R,), n, dtype=torch.int32, device=DEV) for n in (0, 1, 5, 20)}
    cases = [(f"prompt_logprobs n={n}", lambda n=n: ops.prompt_logprobs(logits, tg, nr[n], lp, rank, ids, top))
             for n in (0, 1, 5, 20)]
    cases += [(f"top_logprobs n={n}", lambda n=n: ops.top_logprobs(logits, nr[n], ids, top)) for n in (1, 5)]
    cases += [("copy", lambda: dst.copy_(logits))]
    for _, fn in cases:
        fn()
    torch.cuda.synchronize()
    evs = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[name].append((a, b))
    torch.cuda.synchronize()
    nbytes = R * V * 2
    for name, _ in cases:
        ts = sorted(a.elapsed_time(b) * 1000 for a, b in evs[name])
        us = ts[len(ts) // 2]
        moved = nbytes * (2 if name == "copy" else 1)
        emit(op=name, R=R, V=V, us=round(us, 1), min_us=round(ts[0], 1), max_us=round(ts[-1], 1),
             logits_MB=round(nbytes / 1e6, 1), TBps=round(moved / us / 1e6, 3))


def bench_prompt_logprobs_step(ops):
    """Cost to a request: one prefill step of 8 x 1,024 tokens (llama-3-8b, dummy weights)
    with and without prompt_logprobs=1, in alternation, and the lm_head + kernel part on its
    own (the 8 x 1,023 scored rows through ModelRunner._prompt_logprobs)."""
    import time

    import numpy as np

    from hipserve.config import EngineConfig
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.engine.model_runner import StepInputs
    from hipserve.engine.request import SamplingParams

    eng = LLMEngine(EngineConfig(model="llama-3-8b", load_format="dummy", max_num_seqs=64, max_num_batched_tokens=8192,
                                 max_model_len=2048, num_kv_blocks=4096, enable_prefix_caching=False,
                                 enforce_eager=True))
    rng = np.random.default_rng(0)

    def step(plp):
        prompts = [rng.integers(10, 100000, 1024).tolist() for _ in range(8)]
        for p in prompts:
            eng.add_request(None, p, SamplingParams(temperature=0.0, max_tokens=1, ignore_eos=True, prompt_logprobs=plp))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(outs) == 8 and not eng.has_unfinished()
        return dt * 1e3

    step(None), step(1)
    ts = {None: [], 1: []}
    for _ in range(5):
        for plp in (None, 1):
            ts[plp].append(step(plp))
    base, scored = sorted(ts[None])[2], sorted(ts[1])[2]
    r = eng.runner
    m = 8 * 1023
    hidden = torch.randn(8192, r.mcfg.hidden_size, device=DEV).to(torch.bfloat16)
    inp = StepInputs(*([None] * 17))
    inp.plp_rows = np.array([i for i in range(8192) if i % 1024 != 1023], np.int64)
    inp.plp_targets = rng.integers(0, r.mcfg.vocab_size, m).astype(np.int32)
    inp.plp_n = np.ones(m, np.int32)
    part = timeit(lambda: r._prompt_logprobs(hidden, inp), n=5, warm=1) / 1e3
    emit(op="prefill_step_8x1024", model="llama-3-8b", step_ms=round(base, 2), step_ms_prompt_logprobs_1=round(scored, 2),
         step_ms_all=[round(t, 2) for t in ts[None]], step_ms_prompt_logprobs_1_all=[round(t, 2) for t in ts[1]],
         diff_ms=round(scored - base, 2), lm_head_plus_kernel_ms=round(part, 2), scored_rows=m,
         share_of_diff=round(part / max(scored - base, 1e-9), 3))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ops = KernelOps()
    for name, fn in [("sample", bench_sample), ("decode", bench_decode), ("prefill", bench_prefill),
                     ("prefill_chunked", bench_prefill_chunked),
                     ("gemm", bench_gemm), ("norm", bench_norm), ("rope", bench_rope)]:
        if which in ("all", name):
            fn(ops)
    # by name only: a 268 MB buffer, and an 8B engine
    for name, fn in [("prompt_logprobs", bench_prompt_logprobs), ("prompt_logprobs_step", bench_prompt_logprobs_step)]:
        if which == name:
            fn(ops)




def bench_tune():
    from hipserve.ops import gemm
    shapes = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336), (128256, 4096)]
    import time
    t0 = time.time()
    ms = [int(m) for m in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 16, 32, 64]
    for r in gemm.TUNER.tune(shapes, torch.device("cuda"), ms):
        emit(op="gemm_tune", **r)
    emit(op="gemm_tune_total_s", seconds=round(time.time() - t0, 1))


def bench_gemm_sweep():
    """Every decode-GEMM candidate vs hipBLASLt, cold weights (tuner timing)."""
    import torch.nn.functional as F
    from hipserve.ops import gemm
    T = gemm.GemmTuner
    shapes = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]
    ms = [int(m) for m in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64]
    for N, K in shapes:
        ncopy = max(1, min(16, -(-gemm.COLD_BYTES // (N * K * 2))))
        ws_ = [torch.randn(N, K, device="cuda", dtype=torch.bfloat16) for _ in range(ncopy)]
        wp_ = [gemm.pack(w) for w in ws_]
        n = max(16, ncopy)
        for M in ms:
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            res = {"blas": T._time(lambda i: F.linear(x, ws_[i % ncopy]), n=n)}
            for cfg in T.candidates(M, N, K, packed=True):
                res[str(cfg)] = T._time(lambda i: gemm.run_choice(cfg, out, x, ws_[i % ncopy], wp_[i % ncopy]), n=n)
            emit(op="gemm_sweep", M=M, N=N, K=K, **{k: round(v, 1) for k, v in sorted(res.items(), key=lambda kv: kv[1])[:10]})
        del ws_, wp_


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "sweep":
    KernelOps()
    bench_gemm_sweep()
    sys.exit(0)


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "tune":
    KernelOps()
    bench_tune()
    sys.exit(0)


if __name__ == "__main__":
    main()
