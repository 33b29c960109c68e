"""min_p and logit_bias end to end on the GPU: requests that use them keep the whole
batch on the hipGraph + lookahead decode path and match the eager engine."""
import pytest

from hipserve.engine.request import SamplingParams

from .test_engine_gpu import PROMPTS, _engine

pytestmark = pytest.mark.gpu


def _run(eng, prompts, sps):
    rids = [eng.add_request(None, p, sp).request_id for p, sp in zip(prompts, sps)]
    toks, lps = {r: [] for r in rids}, {r: [] for r in rids}
    while eng.has_unfinished():
        for o in eng.step():
            toks[o.request_id] += o.new_token_ids
            if o.logprobs and len(o.logprobs) > 1:
                lps[o.request_id].append(o.logprobs[1])
    return [toks[r] for r in rids], [lps[r] for r in rids]


def test_min_p_and_logit_bias_stay_on_graph():
    """Request 1 bans (-100) the token its plain run emits most, request 2 samples with
    min_p, request 3 has both plus a penalty and logprobs, in a batch of 8: graph engine
    and eager engine agree token for token, decode stays on the graph path, the banned
    token never appears, and every bias and penalty slot is free again at the end."""
    prompts = PROMPTS * 2
    n = 20
    plain = [SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True) for _ in prompts]
    g, e = _engine(False, max_num_seqs=8), _engine(True, max_num_seqs=8)   # 8 rows: a graph bucket, 8 slots
    assert g.lookahead
    base, _ = _run(g, prompts, plain)
    _run(e, prompts, plain)   # both engines enter the compared run with the same prefix-cache state
    ban1 = max(set(base[1]), key=base[1].count)
    ban3 = max(set(base[3]), key=base[3].count)
    sps = list(plain)
    sps[1] = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True, logit_bias={str(ban1): -100})
    sps[2] = SamplingParams(temperature=0.8, seed=1234, min_p=0.2, max_tokens=n, ignore_eos=True)
    sps[3] = SamplingParams(temperature=0.8, seed=99, min_p=0.1, max_tokens=n, ignore_eos=True,
                            logit_bias={ban3: -100, 11: 3.0, 12: -2.5}, frequency_penalty=0.7,
                            repetition_penalty=1.2, logprobs=5)
    before = g.runner.stats["graph_steps"]
    tg, lg = _run(g, prompts, sps)
    te, le = _run(e, prompts, sps)
    assert tg == te
    assert all(len(t) == n for t in tg)
    assert g.runner.stats["graph_steps"] - before >= 18, g.runner.stats   # decode stayed on the graph path
    assert e.runner.stats["graph_steps"] == 0
    # the ban acted: never the banned token, and not the output of the unbiased twin (same prompt)
    assert ban1 not in tg[1] and tg[1] != tg[5]
    assert ban3 not in tg[3]
    # top-n logprobs stay those of the raw distribution on both paths
    assert len(lg[3]) == len(le[3]) == n
    for a, b in zip(lg[3], le[3]):
        assert [i for i, _ in a] == [i for i, _ in b]
        assert all(abs(x - y) < 1e-3 for (_, x), (_, y) in zip(a, b))
    # a plain batch after it: the staged bias slots and min_p are back at their defaults
    assert _run(g, prompts, plain)[0] == _run(e, prompts, plain)[0]
    for r in (g.runner, e.runner):
        assert len(r._free_bias) == r.bias_n.shape[0] and len(set(r._free_bias)) == r.bias_n.shape[0]
        assert len(r._free_pen) == r.pen_counts.shape[0]
