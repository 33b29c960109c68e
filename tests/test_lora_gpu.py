"""Multi-LoRA kernels (csrc/kernels/lora.hip) against an fp64 reference built from the same
bf16 inputs, with the kernel's single bf16 rounding of t."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SLOTS = 17  # enough for a different adapter on each of a tile's 16 rows
# (slice widths, per-module padded rank r): wo / wd, wqkv under GQA, gate | up
SHAPES = {"one": ((48,), 16), "qkv": ((64, 16, 16), 64), "gu": ((80, 80), 32)}


def _idx(pattern, M):
    i = torch.arange(M)
    if pattern == "one":
        return torch.full((M,), 3)
    if pattern == "none":
        return torch.full((M,), -1)
    if pattern == "mixed":  # -1 and 3 adapters inside every tile
        return torch.tensor([-1, 0, 5, 5, 16, -1, 0, 16])[i % 8]
    return i % SLOTS  # "each": no two rows of a tile share an adapter


ROWS = 1040  # 65 tiles: 3 K slices of 4160, a wave owns 384 columns (the 256-column loop and a ragged end)
# the issue's shapes, then gate | up at r 64 / r 16 (R = 128 / 32: the 8- and 2-tile shrink instantiations)
SHAPES.update({"gu64": ((80, 80), 64), "gu16": ((80, 80), 16)})


@functools.lru_cache(maxsize=None)
def _weights(K, shape):
    widths, r = SHAPES[shape]
    g = torch.Generator().manual_seed(K + r)
    R, N = r * len(widths), sum(widths)
    A = (torch.randn(SLOTS, R, K, generator=g) / K ** 0.5).bfloat16().cuda()
    B = torch.randn(SLOTS, N, r, generator=g).bfloat16().cuda()
    scale = (0.5 + torch.rand(SLOTS, generator=g)).cuda()
    x = torch.randn(ROWS, K, generator=g).bfloat16().cuda()
    out0 = torch.randn(ROWS + 3, N + 8, generator=g).cuda()
    return A, B, scale, x, out0


def _check(M, pattern, K, shape, f32):
    from hipserve.ops import KernelOps

    ops = KernelOps()
    widths, r = SHAPES[shape]
    N, R = sum(widths), r * len(widths)
    begins = [sum(widths[:j]) for j in range(len(widths))]
    slices = [(n0, j * r) for j, n0 in enumerate(begins)]
    A, B, scale, x, out0 = _weights(K, shape)
    x = x[:M]
    idx = _idx(pattern, M).int().cuda()
    buf = out0.clone() if f32 else out0.bfloat16()
    before = buf.clone()
    out = buf[:M, :N]  # row stride N + 8, rows below

    t = torch.empty(M, R, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ops.LORA_WS_ROWS * R, dtype=torch.float32, device="cuda")
    ops.lora_shrink(t, x, A, idx, ws)
    ops.lora_expand(out, t, B, scale, idx, slices)
    torch.cuda.synchronize()

    assert torch.equal(buf[M:], before[M:]) and torch.equal(buf[:, N:], before[:, N:])
    none = idx < 0
    assert torch.equal(buf[:M][none], before[:M][none])  # bit-identical, in both modes

    worst = 0.0
    for a in idx[~none].unique().tolist():
        rows = (idx == a).nonzero().flatten()
        x64, A64, B64, sc = x[rows].double(), A[a].double(), B[a].double(), scale[a].double()
        t64 = (x64 @ A64.t()).bfloat16().double()  # the one rounding of t
        tmag = x64.abs() @ A64.abs().t()
        ref, tol = before[:M, :N][rows].double(), torch.zeros(rows.numel(), N, dtype=torch.float64, device="cuda")
        for (n0, off), w in zip(slices, widths):
            Bs = B64[n0:n0 + w]
            ref[:, n0:n0 + w] += sc * (t64[:, off:off + r] @ Bs.t())
            tol[:, n0:n0 + w] = sc * (2.0 ** -9 * (t64[:, off:off + r].abs() @ Bs.abs().t())
                                      + K * 2.0 ** -24 * (tmag[:, off:off + r] @ Bs.abs().t()))
        if not f32:
            tol = tol + 2.0 ** -9 * ref.abs()
        worst = max(worst, ((out[rows].double() - ref).abs() / (2 * tol)).max().item())
    print(f"max err / tol = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", ["one", "qkv", "gu"])
@pytest.mark.parametrize("K", [64, 4096 + 64])
@pytest.mark.parametrize("pattern", ["one", "none", "mixed", "each"])
@pytest.mark.parametrize("M", [1, 16, 17, 69])
def test_shrink_expand(M, pattern, K, shape, f32):
    _check(M, pattern, K, shape, f32)


@pytest.mark.parametrize("shape", ["qkv", "gu64", "gu16"])
@pytest.mark.parametrize("M,K", [(ROWS, 4096 + 64), (ROWS - 7, 3072), (69, 4096 + 64)])
def test_shrink_wide_slices(M, K, shape):
    """Prefill-sized M: few K slices, so a wave owns 256 columns or more (the shrink's main
    loop); K 3072 in 3 slices is exactly one 256-column chunk a wave. 69 rows: the decode
    split on the 2- and 8-tile instantiations."""
    _check(M, "mixed", K, shape, False)


def test_engine_mixed_batch(tmp_path):
    """One batch mixing base, ad1 and ad2 requests on the tiny Llama of lora_cases.py. With
    seed 4 (chosen on the CPU among 1..12) both adapters change the base model's first token
    on all 4 prompts, and the smallest fp32 top-1 / top-2 log-prob gap over the 12 cases is
    0.043."""
    from hipserve.engine.request import SamplingParams

    from . import lora_cases as LC

    paths = LC.write_all(str(tmp_path))
    lora = {n: paths[n] for n in LC.ADAPTERS}
    prompts = LC.PROMPTS * 3
    names = [None] * 4 + ["ad1"] * 4 + ["ad2"] * 4
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    res = {}
    for key, dev, eager in (("graph", "cuda", False), ("eager", "cuda", True), ("cpu", "cpu", True)):
        eng = LC.engine(paths["base"], dev, lora, eager)
        res[key] = [r[0] for r in eng.generate(prompts, sp, lora=names)]
        if key == "graph":
            st = eng.runner.stats  # the adapter rows decode inside the LoRA variant of the graphs
            assert eng.runner.use_graphs and any("lora" in k for k in eng.runner.graphs) and st["graph_steps"] >= 5
            alone = [r[0] for r in eng.generate(prompts[:4], sp)]  # base-only: the unchanged graphs
        eng.shutdown()
    for a, b in zip(res["graph"], res["eager"]):
        assert len(a) == 6 and a[:2] == b[:2], res
    assert sum(a[0] != b[0] for a, b in zip(res["graph"], res["cpu"])) <= 1, res
    assert sum(a[0] != b[0] for a, b in zip(res["cpu"][4:], res["cpu"][:4] * 2)) >= 7  # the adapters bite
    assert res["graph"][:4] == alone
