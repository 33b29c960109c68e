"""prompt_logprobs on the GPU: the one-pass kernel against a float64 oracle of the exact
input values (tests/prompt_logprobs_cases.py), and the engine's prompt log-probs against the
fp32 CPU engine on the same weights."""
import pytest
import torch

from hipserve.engine.request import SamplingParams

from .prompt_logprobs_cases import CASES, K, case, check
from .test_engine_gpu import _engine

pytestmark = pytest.mark.gpu


def _device_logits(x, dtype, layout, dev):
    dt = getattr(torch, dtype)
    R, V = x.shape
    if layout == "view":  # what compute_logits returns after the TP all-gather
        buf = torch.zeros(R, V + 64, dtype=dt, device=dev)
        buf[:, :V] = x.to(dt)
        buf[:, V:] = 100.0  # larger than every logit: read past V and the results change
        return buf[:, :V]
    return x.to(dt).to(dev)


def _outputs(R, dev, width=K):
    return (torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
            torch.empty(R, width, dtype=torch.int32, device=dev), torch.empty(R, width, dtype=torch.float32, device=dev))


@pytest.mark.parametrize("R,V,dtype,layout", CASES)
def test_kernel_matches_fp64_oracle(R, V, dtype, layout):
    from hipserve.ops import load_library

    x, tg, nreq = case(R, V, dtype)  # builds the case and checks the <= 64-per-bin condition on the CPU
    load_library()
    op = torch.ops.hipserve
    dev = torch.device("cuda", 0)
    lg = _device_logits(x, dtype, layout, dev)
    if layout == "odd":
        assert lg.stride(0) % 8 != 0
    lp, rank, ids, top = _outputs(R, dev)
    op.prompt_logprobs(lg, tg.to(dev), nreq.to(dev), lp, rank, ids, top)
    check(f"prompt_logprobs {R}x{V} {dtype}", (lp.cpu(), rank.cpu(), ids.cpu(), top.cpu()), R, V, dtype)
    # rows with n >= 1: the ids top_logprobs gives on the same logits
    oi = torch.empty(R, K, dtype=torch.int32, device=dev)
    ol = torch.empty(R, K, dtype=torch.float32, device=dev)
    op.top_logprobs(lg, nreq.to(dev), oi, ol)
    sel = nreq > 0
    assert torch.equal(ids.cpu()[sel], oi.cpu()[sel])


def test_bad_arguments_raise():
    from hipserve.ops import load_library

    load_library()
    op = torch.ops.hipserve
    dev = torch.device("cuda", 0)
    R, V = 4, 64
    lg = torch.zeros(R, V, dtype=torch.bfloat16, device=dev)
    tg = torch.zeros(R, dtype=torch.int32, device=dev)
    nr = torch.zeros(R, dtype=torch.int32, device=dev)
    op.prompt_logprobs(lg, tg, nr, *_outputs(R, dev))
    with pytest.raises(RuntimeError, match="targets must be int32"):
        op.prompt_logprobs(lg, tg.long(), nr, *_outputs(R, dev))
    with pytest.raises(RuntimeError, match="at most 20"):
        op.prompt_logprobs(lg, tg, nr, *_outputs(R, dev, width=21))
    with pytest.raises(RuntimeError, match="nreq must have"):
        op.prompt_logprobs(lg, tg, nr[:R - 1], *_outputs(R, dev))
    with pytest.raises(RuntimeError, match="out_lp must have"):
        out = list(_outputs(R, dev))
        out[0] = out[0][:R - 1]
        op.prompt_logprobs(lg, tg, nr, *out)
    with pytest.raises(RuntimeError, match="targets must be a tensor on"):
        op.prompt_logprobs(lg, tg.cpu(), nr, *_outputs(R, dev))


# 4, 41, 290 and 599 tokens: the last two span prefill chunks of 256
PROMPTS = [[1, 7, 8, 9], [1] + [42] * 40, [1] + list(range(10, 299)), list(range(3, 602))]


def _run(eng, sp):
    ids = [eng.add_request(None, p, sp).request_id for p in PROMPTS]
    toks, plp = {r: [] for r in ids}, {}
    while eng.has_unfinished():
        for o in eng.step():
            toks[o.request_id] += o.new_token_ids
            if o.prompt_logprobs is not None:
                assert o.request_id not in plp and o.num_output_tokens == 1  # once, with the first token
                plp[o.request_id] = o.prompt_logprobs
    return [toks[r] for r in ids], [plp.get(r) for r in ids]


def test_engine_prompt_logprobs_match_cpu_engine():
    """small-llama, chunked prefill (256 tokens a step), prompt_logprobs=5: every prompt
    log-prob within 0.1 of the fp32 CPU engine's on the same weights (twice the 0.05 logit
    bound of test_engine_gpu: the target logit and the log-sum-exp)."""
    assert [len(p) for p in PROMPTS] == [4, 41, 290, 599]
    g = _engine(True)
    c = _engine(True, device="cpu", dtype="float32")
    gm, cm = g.runner.model, c.runner.model
    cm.embed = gm.embed.float().cpu()
    cm.lm_head = gm.lm_head.float().cpu()
    cm.norm = gm.norm.float().cpu()
    for lg, lc in zip(gm.layers, cm.layers):
        for f in ("ln1", "wqkv", "wo", "ln2", "wgu", "wd"):
            setattr(lc, f, getattr(lg, f).float().cpu())
    # first without the field, on the empty prefix cache: requests that score their prompt take
    # no prefix hit, so both runs prefill the same chunks
    plain, none = _run(g, SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True))
    assert none == [None] * len(PROMPTS)
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True, prompt_logprobs=5)
    tg, pg = _run(g, sp)
    _, pc = _run(c, sp)
    worst = 0.0
    for p, a, b in zip(PROMPTS, pg, pc):
        assert len(a) == len(p) == len(b) and a[0] is None and b[0] is None
        for t, (lp, rank, top), (lpc, _, _) in zip(p[1:], a[1:], b[1:]):
            worst = max(worst, abs(lp - lpc))
            assert rank >= 1 and len(top) == 5
            assert (rank == 1) == (top[0][0] == t)
            vals = [v for _, v in top]
            assert all(x >= y for x, y in zip(vals, vals[1:]))
            if rank <= 5:
                assert top[rank - 1] == (t, lp)
    print(f"max |GPU - CPU| prompt log-prob: {worst:.4f}")
    assert worst < 0.1
    # the field changes nothing about the generated tokens
    assert tg == plain
