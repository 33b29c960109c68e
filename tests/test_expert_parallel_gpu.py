"""Expert-parallel MoE under TP on the GPU: ``moe_align`` over an expert range (pairs of
other ranks' experts take no slot), the combine kernels skipping those pairs, one MoE layer
summed over the ranks against an fp32 oracle (bf16 unpacked / packed and INT8 experts,
decode- and prefill-sized, captured in a hipGraph), the automatic choice of expert sharding
where the width slice has no expert kernel (Qwen3-30B-A3B's 768-wide experts at TP=2), and
a TP=2 engine (two ranks sharing cuda:0) against TP=1."""
import multiprocessing as mp
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from hipserve.ops import load_library

    load_library()


# ------------------------------------------------------------------ 1. moe_align with a range
def _ids(T, k, Eg, lo, E, seed):
    """[T, k] distinct expert ids per token: token 0 has no expert in [lo, lo + E) and the
    local expert lo + 1 has no pair at all."""
    g = torch.Generator().manual_seed(seed)
    dead = lo + 1
    allowed = torch.tensor([e for e in range(Eg) if e != dead])
    ids = torch.stack([allowed[torch.randperm(len(allowed), generator=g)[:k]] for _ in range(T)])
    outside = torch.tensor([e for e in range(Eg) if not lo <= e < lo + E])
    assert len(outside) >= k
    ids[0] = outside[torch.randperm(len(outside), generator=g)[:k]]
    return ids.int()


def _align(ids, E, tile, lo, ends):
    P = ids.numel()
    cap = -(-(P + E * (tile - 1)) // tile) * tile
    slots = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    te = torch.full((cap // tile,), -7, dtype=torch.int32, device=DEV)
    nt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ps = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    ge = torch.full((E,), -7, dtype=torch.int32, device=DEV) if ends else None
    torch.ops.hipserve.moe_align(ids.to(DEV), E, tile, slots, te, nt, ps, ge, lo)
    torch.cuda.synchronize()
    return slots.cpu().long(), te.cpu().long(), int(nt.item()), ps.cpu().long(), None if ge is None else ge.cpu().long()


def _check_align(ids, E, tile, lo, ends):
    slots, te, nt, ps, ge = _align(ids, E, tile, lo, ends)
    flat = ids.reshape(-1).long()
    P = flat.numel()
    local = (flat >= lo) & (flat < lo + E)
    assert torch.equal(ps < 0, ~local) and bool((ps[~local] == -1).all())
    lp = local.nonzero().squeeze(1)
    assert bool((ps[lp] < slots.numel()).all())
    assert torch.equal(slots[ps[lp]], lp)                      # slots[pair_slot[p]] == p
    assert torch.equal(te[ps[lp] // tile], flat[lp] - lo)      # the tile's expert is the local id
    used = torch.zeros(slots.numel(), dtype=torch.bool)
    used[ps[lp]] = True
    assert int(used.sum()) == lp.numel()                       # one slot per local pair
    assert bool((slots[~used] == -1).all())                    # every other slot is padding
    cnt = torch.bincount(flat[lp] - lo, minlength=E)
    tiles = (cnt + tile - 1) // tile
    assert nt == int(tiles.sum())
    assert torch.equal(te[:nt], torch.repeat_interleave(torch.arange(E), tiles))
    assert bool((te[nt:] == -1).all())
    if ends:
        assert torch.equal(ge, torch.cumsum(tiles * tile, 0))
    return local, cnt


@pytest.mark.parametrize("Eg,k,T,tile,lo,E,ends", [(16, 4, 5, 16, 8, 8, False), (128, 8, 40, 64, 96, 32, False),
                                                    (128, 8, 2064, 128, 64, 64, True)])
def test_moe_align_expert_range(Eg, k, T, tile, lo, E, ends):
    """(128, 8, 2064): 16,512 pairs, the multi-workgroup count / place kernels."""
    ids = _ids(T, k, Eg, lo, E, seed=Eg + T)
    local, cnt = _check_align(ids, E, tile, lo, ends)
    assert not bool(local[:k].any()) and int(cnt[1]) == 0 and 0 < int(local.sum()) < local.numel()
    # all experts from 0: the same invariants, and every pair has a slot
    local, _ = _check_align(ids, Eg, tile, 0, ends)
    assert bool(local.all())


# ------------------------------------------------------------------ 2. combine skip, bit-exact
@pytest.mark.parametrize("T,k,H", [(7, 4, 512), (33, 8, 2048)])
@pytest.mark.parametrize("partial", [False, True])
def test_combine_skips_negative_slots(T, k, H, partial):
    """A pair with pair_slot -1 contributes exactly what a zero-weight pair would: nothing."""
    op = torch.ops.hipserve
    g = torch.Generator(device=DEV).manual_seed(T * k + H)
    P = T * k
    S = 3
    y = (torch.randn(S, P, H, device=DEV, generator=g) if partial
         else torch.randn(P, H, device=DEV, generator=g).to(torch.bfloat16))
    w = torch.rand(T, k, device=DEV, generator=g) + 0.1
    ps = torch.randperm(P, device=DEV, generator=g).int()
    skip = torch.rand(P, device=DEV, generator=g) < 0.4
    skip[k:2 * k] = True   # token 1: no local expert at all -> a zero row
    skip[0] = False
    ps_skip = torch.where(skip, torch.full_like(ps, -1), ps)
    ps_zero = torch.where(skip, torch.zeros_like(ps), ps)
    w_zero = torch.where(skip.view(T, k), torch.zeros_like(w), w)
    run = op.moe_combine_partial if partial else op.moe_combine
    got = torch.full((T, H), 7.0, device=DEV, dtype=torch.bfloat16)
    want = torch.full((T, H), 9.0, device=DEV, dtype=torch.bfloat16)
    run(got, y, w, ps_skip, k)
    run(want, y, w_zero, ps_zero, k)
    assert torch.equal(got, want)
    assert bool((got[1] == 0).all()) and bool(got[0].float().abs().max() > 0)


# ------------------------------------------------------------------ 3. MoE layer, sum over ranks vs fp32
H_, I_, E_, K_ = 512, 768, 16, 4


def _cfg():
    from hipserve.config import PRESETS

    return PRESETS["tiny-mixtral"].replace(name="ep-layer-test", hidden_size=H_, intermediate_size=I_,
                                           num_experts=E_, num_experts_per_tok=K_, num_layers=1)


def _rank_model(r, tp, flag=True):
    from hipserve.models.llama import LlamaModel
    from hipserve.ops import KernelOps
    from hipserve.parallel.comm import TPGroup

    return LlamaModel(_cfg(), TPGroup(r, tp, None, torch.device(DEV)), DEV, torch.bfloat16, KernelOps(),
                      **({"enable_expert_parallel": True} if flag else {}))


_EXPERTS = {}


def _experts(kind):
    """One set of experts per kind, made once: (router, w13 source, w2 source, fp32 w13, fp32 w2)."""
    if kind not in _EXPERTS:
        g = torch.Generator(device=DEV).manual_seed(17)
        router = (torch.randn(E_, H_, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
        w13 = torch.randn(E_, 2 * I_, H_, device=DEV, generator=g) * 0.05
        w2 = torch.randn(E_, H_, I_, device=DEV, generator=g) * 0.05
        if kind == "int8":
            from tests.test_quant_moe_gpu import _qmoe

            # per-output-channel scales: a rank's slice of the experts quantises as the whole set
            d13, d2 = _qmoe(w13, "int8", kmajor=True)[1], _qmoe(w2, "int8")[1]
        else:
            w13, w2 = w13.to(torch.bfloat16), w2.to(torch.bfloat16)
            d13, d2 = w13.float(), w2.float()
        _EXPERTS[kind] = (router, w13, w2, d13, d2)
    return _EXPERTS[kind]


def _layer(m, kind):
    """The LayerWeights of model ``m``'s own expert range."""
    from hipserve.models.llama import LayerWeights

    router, w13, w2, _, _ = _experts("int8" if kind == "int8" else "bf16")
    sl = slice(m.expert_lo, m.expert_lo + m.num_local_experts)
    lw = LayerWeights(ln1=None, wqkv=None, wo=None, ln2=None, router=router)
    if kind == "int8":
        from tests.test_quant_moe_gpu import _qmoe

        lw.w13, lw.w2 = _qmoe(w13[sl], "int8", kmajor=True)[0], _qmoe(w2[sl], "int8")[0]
    else:
        lw.w13, lw.w2 = w13[sl].contiguous(), w2[sl].contiguous()
        if kind == "packed":
            lw.moe_packed = m._pack_experts(lw.w13, lw.w2)
    return lw


def _oracle(x, wts, ids, d13, d2):
    """fp32 over ALL experts with the routing the kernel made (no near-tie flips)."""
    want = torch.zeros(x.shape[0], H_, device=DEV)
    xf = x.float()
    for e in range(E_):
        rows, slot = (ids == e).nonzero(as_tuple=True)
        if rows.numel():
            gu = xf[rows] @ d13[e].T
            act = torch.nn.functional.silu(gu[:, :I_]) * gu[:, I_:]
            want.index_add_(0, rows, (act @ d2[e].T) * wts[rows, slot].unsqueeze(-1))
    return want


def _sum_over_ranks(kind, T, tp, grouped=False):
    from hipserve.models.moe import ExpertWeights
    from hipserve.ops import quant as Q

    x = torch.randn(T, H_, device=DEV, generator=torch.Generator(device=DEV).manual_seed(T)).to(torch.bfloat16)
    got = torch.zeros(T, H_, device=DEV)
    seen = []
    for r in range(tp):
        m = _rank_model(r, tp)
        assert m.moe_shard == ("expert", r * E_ // tp, E_ // tp) and m.inter == I_
        lw = _layer(m, kind)
        if not grouped:
            y = m.moe(x, lw)
        elif kind == "int8":  # as moe() does for a prefill-sized batch on quantised experts
            packed = (Q.moe_packed_scratch(lw.w13, 0, True), Q.moe_packed_scratch(lw.w2, 1, False))
            y = m.moe_grouped(x, ExpertWeights(lw.router, moe_packed=packed))
        else:
            y = m.moe_grouped(x, lw)
        got += y.float()
        seen.append((m, lw, y))
    wts, ids = seen[0][0]._route(x, seen[0][1], K_)
    _, _, _, d13, d2 = _experts("int8" if kind == "int8" else "bf16")
    want = _oracle(x, wts, ids.long(), d13, d2)
    err = (got - want).abs().max().item()
    bound = 3e-2 * want.abs().max().item() + 1e-3
    print(f"{kind} T={T} tp={tp} grouped={grouped}: max err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)   # every element
    return x, seen


@pytest.mark.parametrize("kind", ["bf16", "packed", "int8"])
@pytest.mark.parametrize("T", [3, 40])
def test_expert_parallel_layer_tp2_vs_fp32(kind, T):
    x, seen = _sum_over_ranks(kind, T, 2)
    if T != 3:
        return
    # the decode-sized call is device-only: capture it in a hipGraph and replay
    m, lw, eager = seen[1]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.moe(x, lw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = m.moe(x, lw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, eager)


def test_expert_parallel_layer_tp4_vs_fp32():
    _sum_over_ranks("packed", 40, 4)


@pytest.mark.parametrize("kind", ["bf16", "int8"])
def test_expert_parallel_grouped_prefill_tp2_vs_fp32(kind):
    _sum_over_ranks(kind, 300, 2, grouped=True)


# ------------------------------------------------------------------ 4. the crash this replaces
def test_width_768_at_tp2_runs_without_the_flag():
    """Experts of width 768 at TP=2 are 384 per rank, which no expert GEMM takes: the model
    used to raise NotImplementedError on its first forward. It now holds whole experts."""
    x = torch.randn(6, H_, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(torch.bfloat16)
    outs = []
    for r in range(2):
        m = _rank_model(r, 2, flag=False)
        m.allocate_random(seed=1, std=0.05)
        y = m.moe(x, m.layers[0])  # without expert sharding: NotImplementedError, no kernel for I = 384
        assert y.shape == (6, H_) and bool(torch.isfinite(y.float()).all())
        assert m.moe_shard == ("expert", r * E_ // 2, E_ // 2)
        assert (m.expert_lo, m.num_local_experts, m.inter) == (r * E_ // 2, E_ // 2, I_)
        assert m.layers[0].w13.shape == (E_ // 2, 2 * I_, H_) and m.layers[0].w2.shape == (E_ // 2, H_, I_)
        outs.append(y.float())
    # the two ranks hold the two halves of the TP=1 dummy model's experts
    one = _rank_model(0, 1, flag=False)
    one.allocate_random(seed=1, std=0.05)
    want = one.moe(x, one.layers[0]).float()
    err = (outs[0] + outs[1] - want).abs().max().item()
    assert want.abs().max().item() > 0 and err <= 3e-2 * want.abs().max().item() + 1e-3, err


# ------------------------------------------------------------------ 5. TP=2 engine, two ranks on cuda:0
N_TOK = 33


def _e2e_model_cfg():
    from hipserve.config import PRESETS

    # tests/test_tp_gpu.py's qwen3moe shape with Qwen3-30B-A3B's expert width: 384 per rank at TP=2
    return PRESETS["qwen3-30b-a3b"].replace(name="qwen3moe-ep-test", num_layers=2, hidden_size=1024,
                                            num_heads=8, num_kv_heads=2, moe_intermediate_size=768,
                                            num_experts=16, num_experts_per_tok=4, vocab_size=32000,
                                            max_position_embeddings=1024, eos_token_id=(2,))


def _e2e_engine_cfg(tp, exact, quant):
    from hipserve.config import EngineConfig

    extra = {"tp_exact_reduce": exact}
    if quant:
        extra["quantization"] = quant
    return EngineConfig(model=_e2e_model_cfg().name, load_format="dummy", device="cuda", max_num_seqs=8,
                        max_num_batched_tokens=256, max_model_len=640, num_kv_blocks=512,
                        tensor_parallel_size=tp, extra=extra)


def _e2e_worker(rank, world, port, quant, q, timeout):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK="0",
                      WORLD_SIZE=str(world), HIPSERVE_CAR_TIMEOUT_S="60")
    import faulthandler

    # a rank stuck in a collective, the shm ring or a capture prints its stack before the parent gives up
    faulthandler.dump_traceback_later(max(timeout - 15, 30), exit=False)
    import torch
    import torch.distributed as dist

    from hipserve.engine.llm_engine import LLMEngine, worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.parallel.comm import TPGroup, init_tp
    from tests.test_tp_gpu import PROMPTS, _generate, _logit_bound

    out = None
    try:
        tp = init_tp(world, backend="gloo", device_type="cuda")
        cfg, mcfg = _e2e_engine_cfg(world, True, quant), _e2e_model_cfg()
        if rank == 0:
            eng = LLMEngine(cfg, tp=tp, model_cfg=mcfg)
            m = eng.runner.model
            info = {"graphs": len(eng.runner.graphs), "custom_ar": tp.custom_ar is not None,
                    "shard": m.moe_shard, "experts": type(m.layers[0].w13 if m.layers[0].w13 is not None
                                                          else m.layers[0].moe_packed).__name__}
            ref = LLMEngine(_e2e_engine_cfg(1, False, quant), tp=TPGroup(0, 1, None, torch.device("cuda", 0)),
                            model_cfg=mcfg)
            want, top2 = _generate(ref, PROMPTS, N_TOK, top2=True)
            got, _ = _generate(eng, PROMPTS, N_TOK)
            info["exact_prefix"] = [next((j for j, (a, b) in enumerate(zip(g, w)) if a != b), len(g))
                                    for g, w in zip(got, want)]
            info["logit"] = _logit_bound(eng, ref.runner.model, PROMPTS, want, top2, N_TOK)
            info["car_failed"] = tp.custom_ar.failed() if tp.custom_ar else None
            info["graph_steps"] = eng.runner.stats["graph_steps"]
            eng.shutdown()
            out = ("ok", None, info)
        else:
            worker_loop(ModelRunner(cfg, mcfg, tp), tp)
    except BaseException:
        import traceback
        out = ("error", f"rank {rank}:\n" + traceback.format_exc(), None)
        # report BEFORE touching the device again (see tests/test_tp_gpu.py)
        q.put(out)
        q.close()
        q.join_thread()
        os._exit(1)
    if rank == 0:
        q.put(out)
    q.close()
    q.join_thread()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    os._exit(0)


def _run_e2e(quant, timeout):
    """Runs the two ranks and returns rank 0's report; fails within ~2 s of a rank reporting
    an exception or dying without a report (as tests/test_tp_gpu.py's _run_tp)."""
    import queue
    import time

    from tests.test_tp_gpu import _port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_e2e_worker, args=(r, 2, port, quant, q, timeout)) for r in range(2)]
    for p in ps:
        p.start()
    t_end = time.time() + timeout
    res = None
    try:
        while res is None:
            try:
                res = q.get(timeout=1.0)
                break
            except queue.Empty:
                pass
            dead = [(r, p.exitcode) for r, p in enumerate(ps) if p.exitcode not in (None, 0)]
            if dead:
                try:  # a report may still be in flight from the dying rank
                    res = q.get(timeout=2.0)
                except queue.Empty:
                    res = ("error", f"rank(s) died without a report (rank, exit code): {dead}", None)
            elif time.time() > t_end:
                alive = [r for r, p in enumerate(ps) if p.is_alive()]
                res = ("error", f"timeout after {timeout} s; ranks still running: {alive}", None)
    finally:
        for p in ps:
            p.join(20 if res and res[0] == "ok" else 2)
            if p.is_alive():
                p.kill()
    status, err, info = res
    assert status == "ok", err
    return info


# the existing MoE TP=2 cases (256 tokens per prompt, the same two engines) take 6-10 s each in
# the suite's logs and carry a 300 s limit; this one generates 33 tokens per prompt (4-17 s
# measured, the first case timing the decode GEMMs for an empty tuning cache)
@pytest.mark.timeout(90)
@pytest.mark.parametrize("quant", [None, "int8"], ids=["bf16", "int8"])
def test_tp2_expert_parallel_engine_matches_tp1(quant):
    """Qwen3-MoE with 768-wide experts at TP=2 (the reference's Qwen3-VL-30B-A3B default,
    gpuRequestCount 2): no flag, expert sharding chosen at construction, hipGraph decode and
    the in-house all-reduce summing the ranks' expert outputs; exact (fp32) exchange, and the
    teacher-forced logit bound derived from TP=1's own distance to fp32."""
    from tests.test_tp_gpu import _check_bound

    info = _run_e2e(quant, timeout=75)
    assert info["shard"] == ("expert", 0, 8), info
    assert info["experts"] == ("QuantMoE" if quant else "Tensor"), info
    assert info["graphs"] and info["graph_steps"] > 0 and info["custom_ar"], info
    assert info["car_failed"] is False
    print("greedy divergences (not asserted): exact prefixes", info["exact_prefix"], "of", N_TOK)
    _check_bound(info["logit"], True)
