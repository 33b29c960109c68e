"""min_p in the sampler kernels and the logit_bias kernel against the PyTorch reference.

Vocabulary sizes: 4099 takes the one-workgroup sampler (V < 8192) with a ragged last
8-element group; 16390 the multi-CU path with two chunks, the second of 6 elements;
128256 is the 8-chunk production shape."""
import functools
import math

import pytest
import torch

from hipserve.ops import KernelOps
from hipserve.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 12
TEMP = [0.0, 1.0, 0.7, 1.0, 1.3, 0.9, 1.0, 0.5, 1.0, 2.0, 0.0, 1.5]
MIN_P = [0.3, 0.05, 0.1, 1.0, 0.02, 0.2, 0.01, 0.5, 0.3, 0.1, 0.0, 0.0]   # alone: rows 1, 3, 6
TOP_K = [0, 0, 50, 0, 0, 20, 0, 0, 1000, 5, 0, 7]                         # with top-k: 2, 9
TOP_P = [1.0, 1.0, 1.0, 1.0, 0.9, 0.5, 1.0, 0.95, 0.8, 1.0, 1.0, 0.3]     # top-p: 4, 7; both: 5, 8
BAND = 0.02   # the device __logf and the host log differ in the last bits: no logit may sit
              # this close to a row's cut z = ln(min_p)
CASES = [(4099, torch.float32), (4099, torch.bfloat16), (16390, torch.bfloat16), (128256, torch.bfloat16)]


@pytest.fixture(scope="module")
def ops():
    return KernelOps()


def _z_dist(x, r):
    """|z - ln(min_p)| of row r's entries, the row maximum (first argmax) at +inf."""
    z = (x[r] - x[r].max()) / TEMP[r]
    d = (z - math.log(MIN_P[r])).abs()
    d[int(x[r].argmax())] = float("inf")
    return d


@functools.lru_cache(maxsize=None)
def _case(V):
    """Logits (bf16-exact fp32 values: what the kernels and the reference see for either
    input dtype), the per-row parameters, and the reference's keep sets / draw, computed
    once per vocabulary size and shared by the tests below (never modified)."""
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16).float()
    for r in range(B):
        if TEMP[r] > 1e-5 and MIN_P[r] > 0:
            near = _z_dist(x, r) < BAND
            x[r, near] = x[r].max() + TEMP[r] * (math.log(MIN_P[r]) - 0.25)
    x = x.to(torch.bfloat16).float()
    for r in range(B):
        if TEMP[r] > 1e-5 and MIN_P[r] > 0:
            assert not (_z_dist(x, r) < BAND).any(), r   # the band is empty
    temp, minp = torch.tensor(TEMP), torch.tensor(MIN_P)
    tk, tp = torch.tensor(TOP_K, dtype=torch.int32), torch.tensor(TOP_P)
    seeds = torch.arange(B, dtype=torch.long) * 7919 + 1
    steps = torch.arange(B, dtype=torch.long) + 2
    keep = torch.zeros(B, V, dtype=torch.bool)
    for r in range(B):
        if TEMP[r] > 1e-5:
            keep[r] = ref.sample_keep(x[r], TEMP[r], TOP_K[r], TOP_P[r], MIN_P[r])
        else:
            keep[r, int(x[r].argmax())] = True
    kept = keep.sum(1)
    assert (kept >= 1).all() and kept[3] == 1          # min_p = 1: the argmax alone
    rt, rlp = ref.sample(x, temp, tk, tp, seeds, steps, min_p=minp)
    return x, (temp, tk, tp, seeds, steps), minp, keep, rt, rlp


def _run(ops, x, dtype, args, **kw):
    logits = x.to(dtype).to(DEV)
    tok = torch.empty(B, device=DEV, dtype=torch.long)
    lp = torch.empty(B, device=DEV, dtype=torch.float32)
    ops.sample(tok, lp, logits, *[a.to(DEV) for a in args], **kw)
    return tok.cpu(), lp.cpu()


@pytest.mark.parametrize("V,dtype", CASES)
def test_min_p_draws_stay_in_the_keep_set(ops, V, dtype):
    """Hard, no allowance: every sampled token is in the reference's keep set (top-k,
    top-p and min_p survivors); greedy rows and min_p = 1 rows return the argmax."""
    x, args, minp, keep, _, _ = _case(V)
    tok, _ = _run(ops, x, dtype, args, min_p=minp.to(DEV))
    inside = keep[torch.arange(B), tok]
    print("kept per row", keep.sum(1).tolist(), "tokens", tok.tolist(), "inside", inside.tolist())
    assert ((tok >= 0) & (tok < V)).all()
    assert inside.all(), (tok, inside)
    for r in (0, 3, 10):
        assert tok[r] == int(x[r].argmax())


@pytest.mark.parametrize("V,dtype", CASES)
def test_min_p_matches_reference_draw(ops, V, dtype):
    """Token equality with ref.sample under test_sample's allowance (at most one row of
    the batch may differ: near-ties in the threshold masses); logprobs of agreeing rows
    within its atol. The logprob stays the log-softmax of the logits given."""
    x, args, minp, _, rt, rlp = _case(V)
    tok, lp = _run(ops, x, dtype, args, min_p=minp.to(DEV))
    ok = tok == rt
    print("mismatching rows", (~ok).nonzero().flatten().tolist(), "max |dlp|",
          float((lp[ok] - rlp[ok]).abs().max()))
    assert (~ok).sum().item() <= 1, (tok, rt)
    assert torch.allclose(lp[ok], rlp[ok], atol=1e-3)


@pytest.mark.parametrize("V,dtype", CASES)
def test_min_p_off_changes_nothing(ops, V, dtype):
    """Without min_p, with min_p=None and with an all-zero min_p tensor: the same tokens
    and logprobs, bit for bit."""
    x, args, _, _, _, _ = _case(V)
    t0, l0 = _run(ops, x, dtype, args)
    t1, l1 = _run(ops, x, dtype, args, min_p=None)
    t2, l2 = _run(ops, x, dtype, args, min_p=torch.zeros(B, device=DEV))
    assert torch.equal(t0, t1) and torch.equal(t0, t2)
    assert torch.equal(l0, l1) and torch.equal(l0, l2)


def test_min_p_distribution(ops):
    """Frequencies follow softmax(x) restricted to the min_p survivors: linspace(-2, 2, 16)
    at T = 1 with min_p = 0.25 cuts at 2 + ln 0.25 = 0.614, so ids 10..15 survive (the
    nearest entries are 0.400 and 0.667). N and the bound are test_sample_distribution's."""
    V, N = 16, 4096
    base = torch.linspace(-2, 2, V)
    logits = base.repeat(N, 1).to(DEV)
    tok = torch.empty(N, device=DEV, dtype=torch.long)
    lp = torch.empty(N, device=DEV)
    ops.sample(tok, lp, logits, torch.full((N,), 1.0, device=DEV), torch.zeros(N, device=DEV, dtype=torch.int32),
               torch.ones(N, device=DEV), torch.arange(N, device=DEV, dtype=torch.long),
               torch.zeros(N, device=DEV, dtype=torch.long), min_p=torch.full((N,), 0.25, device=DEV))
    cnt = torch.bincount(tok.cpu(), minlength=V).float() / N
    p = torch.softmax(base[10:], 0)
    print("freq", cnt.tolist())
    assert cnt[:10].sum() == 0
    assert (cnt[10:] - p).abs().max() < 0.03


def test_min_p_graph_capture(ops):
    """Capture + replay of the multi-CU path with min_p gives the eager draw."""
    x, args, minp, _, _, _ = _case(16390)
    logits = x.to(torch.bfloat16).to(DEV)
    dargs = [a.to(DEV) for a in args]
    mp = minp.to(DEV)
    tok = torch.empty(B, device=DEV, dtype=torch.long)
    lp = torch.empty(B, device=DEV)
    ops.sample(tok, lp, logits, *dargs, min_p=mp)
    tok2, lp2 = torch.empty_like(tok), torch.empty_like(lp)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sample(tok2, lp2, logits, *dargs, min_p=mp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sample(tok2, lp2, logits, *dargs, min_p=mp)
    tok2.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(tok2, tok) and torch.equal(lp2, lp)


# ------------------------------------------------------------------ logit_bias
ROWS, SLOTS, WIDTH = 6, 4, 300
COUNTS = [0, 1, 300, 37]
ROW_SLOT = [2, -1, 0, 3, 1, -1]   # row 2 has the empty slot; rows 1 and 5 have none


def _bias_tables(V):
    g = torch.Generator().manual_seed(V)
    ids = torch.zeros(SLOTS, WIDTH, dtype=torch.int32)
    vals = torch.zeros(SLOTS, WIDTH)
    for s, c in enumerate(COUNTS):
        if c:
            perm = torch.randperm(V - 2, generator=g)[:c] + 1   # unique ids in [1, V - 2]
            ids[s, :c] = perm.int()
            vals[s, :c] = (torch.rand(c, generator=g) * 200 - 100)
    ids[2, 0], ids[2, 299] = 0, V - 1    # the first and the last token, the last entry of a full slot
    ids[3, 5] = V - 1
    ids[1, 0], vals[1, 0] = 0, -7.5
    # entries past a slot's count are garbage the kernel must not read as biases
    ids[3, 37:] = 3
    vals[3, 37:] = 50.0
    return ids, vals, torch.tensor(COUNTS, dtype=torch.int32)


@pytest.mark.parametrize("V,dtype", CASES)
def test_logit_bias_apply(ops, V, dtype):
    """Against the reference: the penalty test's tolerance (1e-5 relative for fp32, one
    bf16 ulp 2**-7 for bf16, + 1e-5); rows without a slot or with an empty one keep
    their bits."""
    g = torch.Generator().manual_seed(V + 1)
    logits = (torch.randn(ROWS, V, generator=g) * 3).to(dtype)
    ids, vals, n = _bias_tables(V)
    slot = torch.tensor(ROW_SLOT, dtype=torch.int32)
    want = ref.logit_bias_apply(logits.clone(), slot, ids, vals, n)
    got = logits.clone().to(DEV)
    ops.logit_bias_apply(got, slot.to(DEV), ids.to(DEV), vals.to(DEV), n.to(DEV))
    got = got.cpu()
    biased = torch.zeros(ROWS, V, dtype=torch.bool)
    for r, s in enumerate(ROW_SLOT):
        if s >= 0:
            biased[r, ids[s, :COUNTS[s]].long()] = True
    assert biased.sum(1).tolist() == [300, 0, 0, 37, 1, 0]
    assert torch.equal(got[~biased], logits[~biased])   # every other entry keeps its bits
    assert (want != logits)[biased].float().mean() > 0.9    # the reference did move them
    rtol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
    err = (got.float() - want.float()).abs()
    print("max err", float(err.max()))
    assert (err <= rtol * want.float().abs() + 1e-5).all()


@pytest.mark.parametrize("V,dtype", CASES)
def test_logit_bias_steers_greedy_sample(ops, V, dtype):
    """+100 on one id makes a greedy sample return it; -100 on the argmax makes it return
    the runner-up."""
    g = torch.Generator().manual_seed(V + 2)
    logits = (torch.randn(2, V, generator=g) * 3).to(dtype)
    logits[1, 17], logits[1, V - 5] = 20.0, 19.0   # a clear argmax and runner-up
    order = logits[1].float().argsort(descending=True, stable=True)
    assert logits[1, order[0]] > logits[1, order[1]] > logits[1, order[2]]
    pick = V - 1
    ids = torch.zeros(2, WIDTH, dtype=torch.int32)
    vals = torch.zeros(2, WIDTH)
    ids[0, 0], vals[0, 0] = pick, 100.0
    ids[1, 0], vals[1, 0] = int(order[0]), -100.0
    n = torch.tensor([1, 1], dtype=torch.int32)
    d = logits.to(DEV)
    ops.logit_bias_apply(d, torch.tensor([0, 1], dtype=torch.int32, device=DEV), ids.to(DEV), vals.to(DEV), n.to(DEV))
    tok = torch.empty(2, device=DEV, dtype=torch.long)
    lp = torch.empty(2, device=DEV)
    z = torch.zeros(2, device=DEV)
    ops.sample(tok, lp, d, z, torch.zeros(2, device=DEV, dtype=torch.int32), torch.ones(2, device=DEV),
               torch.zeros(2, device=DEV, dtype=torch.long), torch.zeros(2, device=DEV, dtype=torch.long))
    assert tok.tolist() == [pick, int(order[1])]
