"""Inputs and the float64 oracle shared by the prompt_logprobs kernel test (GPU) and the
reference-op test (CPU): built once per case, never modified.

A case is (logits fp32 [R, V] holding bf16-exact values, targets int32 [R], nreq int32 [R]).
The rows hold between them: nreq 0 / 1 / 2 / 5 / 20, the target at the argmax, the target
inside a run of equal values (its rank goes by id), targets -1 and >= V, rows with -inf
entries (target finite, and target -inf), an all-equal row, and a run of equal values that
crosses the n-th place with fewer than 64 members.
"""
import functools

import torch

K = 20
NEG = float("-inf")
# (R, V, dtype name, layout): "odd" = row stride V (odd: most rows not 16-byte aligned, ragged
# tail), "view" = a [:, :V] view of a buffer 64 columns wider, "small" = V < threads * 8
CASES = [(37, 4099, "float32", "odd"), (37, 4099, "bfloat16", "odd"),
         (5, 128256, "bfloat16", "view"), (3, 300, "float32", "small")]


@functools.lru_cache(maxsize=None)
def case(R, V, dtype):
    g = torch.Generator().manual_seed(R * 1000003 + V)
    x = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16).float()
    tg = torch.randint(0, V, (R,), generator=g).int()
    nreq = torch.tensor([(0, 1, 2, 5, 20)[r % 5] for r in range(R)], dtype=torch.int32)
    exact_ties = set()  # rows whose n-th place lies in a run of EXACTLY equal values longer than 64
    top = lambda r: float(x[r][torch.isfinite(x[r])].max())
    if R == 37:
        tg[0] = int(x[0].argmax())                      # n = 0, target at the argmax
        tg[1] = int(x[1].argmax())                      # n = 1, target is the top-1
        x[2, 100:110] = top(2) + 1                      # n = 2: run of 10 at the top, target inside it
        tg[2] = 105
        tg[3] = -1                                      # n = 5, no target
        tg[4] = V                                       # n = 20, target past the vocabulary
        tg[5] = V + 1000                                # n = 0 and no target: nothing to do
        hole = torch.randperm(V, generator=g)[:500]
        x[6, hole] = NEG                                # n = 1, -inf entries, finite target
        tg[6] = int(torch.isfinite(x[6]).nonzero()[17])
        x[7, hole] = NEG                                # n = 2, the target is -inf
        tg[7] = int(hole[3])
        x[8] = 1.5                                      # n = 5, all equal: rank = id + 1
        tg[8] = 7
        exact_ties.add(8)
        # n = 20: 15 distinct values on top, then a run of 40 equal ones across the 20th place
        run = torch.arange(40) * 97 + 11
        x[9, 4000:4015] = top(9) + 2 + torch.arange(15) * 0.25
        x[9, run] = top(9) - 15 * 0.25 - 1
        tg[9] = int(run[5])                             # the first of the run left out: rank 21
        x[11, [50, 60, 70]] = top(11) + 1               # n = 1: the target ties with the argmax
        tg[11] = 60
        x[12, hole] = NEG                               # n = 2 ... and n = 0 below: -inf targets
        tg[12] = int(hole[9])
        x[15, hole] = NEG
        tg[15] = int(hole[0])
        x[16, :3] = NEG                                 # n = 1: a -inf head (the scalar head elements)
        tg[16] = 1
        if dtype == "float32":
            # fp32 only: ten values inside ONE bf16 bin, increasing with id: the exact-value
            # order is the reverse of the id order (row 5 of test_penalty_and_top_logprobs_kernels)
            x[13, 300:310] = top(13) + 1 + torch.arange(10) * 1e-4   # n = 5
            tg[13] = 304
    elif R == 5:
        tg[1] = int(x[1].argmax())
        x[2, 70000:70006] = top(2) + 1                  # n = 2: run of 6, target its 4th
        tg[2] = 70003
        x[3, torch.randperm(V, generator=g)[:3000]] = NEG   # n = 5
        tg[3] = int(torch.isfinite(x[3]).nonzero()[123])
        tg[4] = V                                       # n = 20
    else:
        nreq = torch.tensor([1, 5, 20], dtype=torch.int32)
        tg[1] = -1
    if dtype == "bfloat16":
        assert torch.equal(x.to(torch.bfloat16).float(), x)
    # the kernels' one bound: at most 64 logits in the bf16 bin of the n-th largest
    for r in range(R):
        n = int(nreq[r])
        if n == 0 or r in exact_ties:
            continue
        b = x[r].to(torch.bfloat16).float()
        kth = torch.sort(b, descending=True).values[n - 1]
        assert int((b == kth).sum()) <= 64, (r, int((b == kth).sum()))
    return x, tg, nreq


@functools.lru_cache(maxsize=None)
def oracle(R, V, dtype):
    """(lp [R], rank [R], ids [R, K], top [R, K]) in float64 on the exact input values."""
    x, tg, nreq = case(R, V, dtype)
    lp = torch.full((R,), NEG, dtype=torch.float64)
    rank = torch.zeros(R, dtype=torch.int32)
    ids = torch.full((R, K), -1, dtype=torch.int32)
    topv = torch.full((R, K), NEG, dtype=torch.float64)
    for r in range(R):
        l = x[r].double()
        lse = torch.logsumexp(l, 0)
        t, n = int(tg[r]), int(nreq[r])
        if 0 <= t < V:
            if l[t] != NEG:
                lp[r] = l[t] - lse
            rank[r] = 1 + int((l > l[t]).sum()) + int((l[:t] == l[t]).sum())
        if n:
            order = torch.argsort(-l, stable=True)[:n]  # value desc, id asc
            ids[r, :n] = order.int()
            topv[r, :n] = torch.where(l[order] == NEG, l[order], l[order] - lse)
    return lp, rank, ids, topv


def check(name, got, R, V, dtype, tol=1e-3):
    """got = (lp, rank, ids, top) CPU tensors against the oracle: ranks, ids and the
    finite / non-finite pattern exact, finite values within tol, no NaN."""
    x, tg, nreq = case(R, V, dtype)
    lp, rank, ids, topv = oracle(R, V, dtype)
    glp, grank, gids, gtop = got
    assert not torch.isnan(glp).any() and not torch.isnan(gtop).any(), name
    assert torch.equal(grank.int(), rank), (name, (grank.int() != rank).nonzero().flatten().tolist())
    assert torch.equal(gids.int(), ids), (name, (gids.int() != ids).any(1).nonzero().flatten().tolist())
    for g, w in ((glp, lp), (gtop, topv)):
        fin = torch.isfinite(w)
        assert torch.equal(torch.isfinite(g), fin), name
        assert torch.equal(g[~fin].double(), w[~fin]), name  # -inf, not +inf
        err = (g[fin].double() - w[fin]).abs().max().item() if fin.any() else 0.0
        print(f"{name}: max |err| {err:.3e}")
        assert err < tol, (name, err)
    # rank <= n exactly when the target stands in the top-n at index rank - 1
    for r in range(R):
        k, n, t = int(grank[r]), int(nreq[r]), int(tg[r])
        if k:
            assert (k <= n) == (t in gids[r, :n].tolist()), (name, r)
            if k <= n:
                assert int(gids[r, k - 1]) == t, (name, r)
