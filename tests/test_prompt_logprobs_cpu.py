"""Prompt log-probs on the CPU engine: the reference op against the float64 oracle, the
engine against log_softmax of the dense forward (chunked prefill, several lm_head chunks a
step), the prefix-cache rule, preemption, TP = 2, LLMEngine.score and tools/perplexity.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import hipserve.engine.model_runner as model_runner
from hipserve.config import EngineConfig
from hipserve.engine.request import MAX_LOGPROBS, RequestOutput, SamplingParams
from hipserve.ops import ReferenceOps

from .prompt_logprobs_cases import CASES, K, case, check
from .test_engine_cpu import dense_logits, make_engine
from .test_tp_cpu import _port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4  # fp32 reduction-order noise, as assert_greedy's


@pytest.mark.parametrize("R,V,dtype,layout", CASES)
def test_reference_op_matches_fp64_oracle(R, V, dtype, layout):
    x, tg, nreq = case(R, V, dtype)
    lp, rank = torch.empty(R), torch.empty(R, dtype=torch.int32)
    ids, top = torch.empty(R, K, dtype=torch.int32), torch.empty(R, K)
    ReferenceOps().prompt_logprobs(x.to(getattr(torch, dtype)), tg, nreq, lp, rank, ids, top)
    check(f"reference {R}x{V} {dtype}", (lp, rank, ids, top), R, V, dtype)


def _dense_logprobs(model, prompt):
    """log_softmax of the dense forward at every position: [len - 1, V] float64."""
    return torch.stack([torch.log_softmax(dense_logits(model, prompt[:p]).double(), 0)
                        for p in range(1, len(prompt))])


def _run(eng, prompts, sp):
    ids = [eng.add_request(None, p, sp).request_id for p in prompts]
    toks, plp = {r: [] for r in ids}, {}
    while eng.has_unfinished():
        for o in eng.step():
            toks[o.request_id] += o.new_token_ids
            if o.prompt_logprobs is not None:
                assert o.request_id not in plp and o.num_output_tokens == 1  # once, with the first token
                plp[o.request_id] = o.prompt_logprobs
    return [toks[r] for r in ids], [plp.get(r) for r in ids]


def _assert_matches_dense(model, prompt, plp, n):
    want = _dense_logprobs(model, prompt)
    assert len(plp) == len(prompt) and plp[0] is None
    for p in range(1, len(prompt)):
        lp, rank, top = plp[p]
        row, t = want[p - 1], prompt[p]
        assert abs(lp - row[t].item()) < TOL, (p, lp, row[t].item())
        # the rank may differ only through logits within the noise of the target's
        lo = 1 + int((row > row[t] + TOL).sum())
        hi = 1 + int((row >= row[t] - TOL).sum()) - 1
        assert lo <= rank <= max(hi, lo), (p, rank, lo, hi)
        assert len(top) == n
        vals = torch.tensor([v for _, v in top], dtype=torch.float64)
        assert (vals - torch.sort(row, descending=True).values[:n]).abs().max() < TOL if n else True
        for i, v in top:
            assert abs(v - row[i].item()) < TOL
        if rank <= n:
            assert top[rank - 1][0] == t


def test_engine_matches_dense_logprobs(monkeypatch):
    """A 71-token prompt in chunks of 24 (three prefill steps) with the row-chunk constant
    patched down to its floor of 16 rows, so one step takes two lm_head chunks; a second,
    short prompt in the same batch."""
    monkeypatch.setattr(model_runner, "PROMPT_LOGPROBS_CHUNK_BYTES", 1)
    eng = make_engine(max_num_batched_tokens=24)
    calls = []
    real = eng.runner.ops.prompt_logprobs
    monkeypatch.setattr(eng.runner.ops, "prompt_logprobs", lambda lg, *a: (calls.append(lg.shape[0]), real(lg, *a)),
                        raising=False)
    prompts = [[1] + list(range(5, 75)), [1, 9, 4]]
    sp = SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True, prompt_logprobs=3)
    toks, plps = _run(eng, prompts, sp)
    assert max(calls) == 16 and sum(calls) == 70 + 2 and len(calls) >= 6
    for p, plp in zip(prompts, plps):
        _assert_matches_dense(eng.runner.model, p, plp, 3)
    # the field changes nothing about the generated tokens; without it nothing is attached
    eng2 = make_engine(max_num_batched_tokens=24)
    toks2, none = _run(eng2, prompts, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    assert toks2 == toks and none == [None, None]
    # n = 0: the token's own log-prob and rank, no alternatives
    _, (zero,) = _run(make_engine(), [prompts[0]], SamplingParams(temperature=0.0, max_tokens=1, prompt_logprobs=0))
    assert [e[0] for e in zero[1:]] == pytest.approx([e[0] for e in plps[0][1:]], abs=TOL)
    assert all(e[2] == [] and e[1] >= 1 for e in zero[1:])
    # a one-token prompt: nothing to score
    _, (one,) = _run(make_engine(), [[7]], SamplingParams(temperature=0.0, max_tokens=1, prompt_logprobs=2))
    assert one == [None]


def test_prefix_cache_rule():
    """A request that scores its prompt takes no prefix hit (cached positions have no hidden
    states); its blocks are registered all the same, and a request without the field hits."""
    eng = make_engine()
    prompt = [1] + list(range(20, 120))
    sp = SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True, prompt_logprobs=2)
    seqs = []
    res = []
    for params in (sp, sp, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True)):
        seq = eng.add_request(None, prompt, params)
        seqs.append(seq)
        plp = None
        while eng.has_unfinished():
            for o in eng.step():
                if o.prompt_logprobs is not None:
                    plp = o.prompt_logprobs
        res.append(plp)
    assert res[0] is not None and res[0] == res[1] and res[2] is None
    assert seqs[0].num_cached_prefix == 0 and seqs[1].num_cached_prefix == 0
    assert seqs[2].num_cached_prefix > 0
    _assert_matches_dense(eng.runner.model, prompt, res[0], 2)


def test_preemption_scores_each_position_once(monkeypatch):
    """A pool small enough to preempt (test_preemption_recompute_is_exact): the recompute starts
    at 0 again, positions already scored are not scored twice, the lists are complete."""
    eng = make_engine(num_kv_blocks=24, block_size=16, max_num_batched_tokens=64, enable_prefix_caching=False)
    rows = []
    real = eng.runner.ops.prompt_logprobs
    monkeypatch.setattr(eng.runner.ops, "prompt_logprobs", lambda lg, *a: (rows.append(lg.shape[0]), real(lg, *a)),
                        raising=False)
    prompts = [list(range(5 + i, 85 + i)) for i in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=40, ignore_eos=True, prompt_logprobs=1)
    toks, plps = _run(eng, prompts, sp)
    assert eng.scheduler.num_preemptions > 0
    assert sum(rows) == sum(len(p) - 1 for p in prompts)  # no position scored twice
    for p, t, plp in zip(prompts, toks, plps):
        assert len(t) == 40
        _assert_matches_dense(eng.runner.model, p, plp, 1)


def test_preempted_mid_prompt_keeps_its_scores():
    """A sequence preempted after its first chunk was scored: the recompute skips the scored
    positions, takes no prefix hit while the list is incomplete, and ends with one entry per
    position."""
    eng = make_engine(max_num_batched_tokens=32)
    prompt = [1] + list(range(30, 120))
    seq = eng.add_request(None, prompt, SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True,
                                                       prompt_logprobs=2))
    eng.step()
    assert len(seq.prompt_logprobs) == 32 and seq.wants_prompt_logprobs
    first = list(seq.prompt_logprobs)
    from hipserve.engine.scheduler import SchedulerOutput

    eng.scheduler._preempt(seq, SchedulerOutput())
    eng.runner.release(seq)
    plp = None
    while eng.has_unfinished():
        for o in eng.step():
            if o.prompt_logprobs is not None:
                plp = o.prompt_logprobs
    assert seq.num_cached_prefix == 0
    assert plp[1:33] == first and len(plp) == len(prompt)
    _assert_matches_dense(eng.runner.model, prompt, plp, 2)


def test_score_equals_the_lists():
    eng = make_engine(max_num_batched_tokens=24)
    prompts = [[1] + list(range(40, 90)), [3, 4], [9] * 30]
    _, plps = _run(eng, prompts, SamplingParams(temperature=0.0, max_tokens=1, prompt_logprobs=0))
    got = make_engine(max_num_batched_tokens=24).score(prompts)
    for p, g, plp in zip(prompts, got, plps):
        assert g.dtype == np.float32 and g.shape == (len(p) - 1,)
        assert g.tolist() == pytest.approx([e[0] for e in plp[1:]], abs=1e-6)
    want = _dense_logprobs(eng.runner.model, prompts[0])
    assert np.abs(got[0] - want[torch.arange(50), torch.tensor(prompts[0][1:])].numpy()).max() < TOL


def test_perplexity_tool(tmp_path):
    rng = np.random.default_rng(11)
    ids = rng.integers(3, 500, 150)
    np.save(tmp_path / "ids.npy", ids)
    out = tmp_path / "ppl.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "perplexity.py"), "--model", "tiny-llama",
                        "--device", "cpu", "--load-format", "dummy", "--max-model-len", "128", "--num-kv-blocks", "64",
                        "--max-num-batched-tokens", "48", "--tokens", str(tmp_path / "ids.npy"), "--ctx", "64",
                        "--json", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(r.stdout.strip().splitlines()[-1]) == res
    # windows of 64, 64 and 22 tokens, each scored from its second token on
    model = make_engine().runner.model
    nll = []
    for a in range(0, 150, 64):
        w = ids[a:a + 64].tolist()
        lp = _dense_logprobs(model, w)
        nll += (-lp[torch.arange(len(w) - 1), torch.tensor(w[1:])]).tolist()
    assert res["tokens"] == len(nll) == 147 and res["windows"] == 3 and res["ctx"] == 64
    assert res["nll"] == pytest.approx(sum(nll) / len(nll), abs=TOL)
    assert res["ppl"] == pytest.approx(math.exp(sum(nll) / len(nll)), rel=2 * TOL)


def test_bad_values_and_images_are_refused():
    assert SamplingParams().prompt_logprobs is None
    assert SamplingParams(prompt_logprobs="3").prompt_logprobs == 3
    assert SamplingParams(prompt_logprobs=0).prompt_logprobs == 0
    for bad in (-1, MAX_LOGPROBS + 1, 1.5, "x", True, [1]):
        with pytest.raises(ValueError, match="prompt_logprobs"):
            SamplingParams(prompt_logprobs=bad)
    # RequestOutput: a new last field with a default; positional construction is unchanged
    assert RequestOutput("r", [1], "a", False).prompt_logprobs is None
    from hipserve.multimodal import MultiModalPrompt

    eng = make_engine()
    with pytest.raises(ValueError, match="prompt_logprobs is not supported for prompts with images"):
        eng.add_request(None, MultiModalPrompt([1, 2, 3], [object()]), SamplingParams(prompt_logprobs=1))
    assert not eng.has_unfinished()


# ---------------------------------------------------------------- TP = 2 on gloo
TP_PROMPTS = [[1, 5, 9, 33, 70], list(range(3, 60)), [7] * 20]


def _tp_cfg(world):
    return EngineConfig(model="tiny-llama", load_format="dummy", device="cpu", dtype="float32",
                        tensor_parallel_size=world, num_kv_blocks=128, max_model_len=256,
                        max_num_batched_tokens=32, max_num_seqs=4)


def _tp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from hipserve.config import resolve_model_config
    from hipserve.engine.llm_engine import LLMEngine, worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.parallel.comm import init_tp

    model_runner.PROMPT_LOGPROBS_CHUNK_BYTES = 1  # several lm_head chunks (and all-gathers) a step
    tp = init_tp(world, backend="gloo", device_type="cpu")
    try:
        if rank == 0:
            eng = LLMEngine(_tp_cfg(world), tp=tp)
            res = _run(eng, TP_PROMPTS, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True,
                                                       prompt_logprobs=3))
            eng.shutdown()
            q.put(res)
        else:
            worker_loop(ModelRunner(_tp_cfg(world), resolve_model_config("tiny-llama"), tp), tp)
    finally:
        dist.destroy_process_group()
    q.close()
    q.join_thread()
    os._exit(0)  # as tests/test_tp_cpu.py: no interpreter teardown under gloo helper threads


def test_tp2_matches_tp1():
    """TP workers run the same lm_head chunks (the all-gather is inside compute_logits). The
    log-probs equal TP = 1 to fp32 reduction-order noise; ids and ranks are pinned by the
    kernel tests (near-ties may flip under a different reduction order)."""
    from hipserve.engine.llm_engine import LLMEngine
    from hipserve.parallel.comm import TPGroup

    toks1, plps1 = _run(LLMEngine(_tp_cfg(1), tp=TPGroup()), TP_PROMPTS,
                        SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True, prompt_logprobs=3))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    toks2, plps2 = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert toks2 == toks1
    for p, a, b in zip(TP_PROMPTS, plps1, plps2):
        assert len(a) == len(b) == len(p) and a[0] is None and b[0] is None
        for t, (lp1, _, top1), (lp2, rank2, top2) in zip(p[1:], a[1:], b[1:]):
            assert abs(lp1 - lp2) < TOL
            assert [v for _, v in top2] == pytest.approx([v for _, v in top1], abs=TOL)
            assert rank2 >= 1 and (rank2 == 1) == (top2[0][0] == t)
