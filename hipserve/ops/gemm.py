"""bf16 linear layers: hipBLASLt (``F.linear``) or a hand-written MFMA GEMM for
decode batches — the split-K LDS-shared ``decode_gemm`` (csrc/kernels/decode_gemm.hip)
or the skinny weight-streaming GEMM (csrc/kernels/skinny_gemm.hip).

The choice is made per (M, N, K) by timing the candidates on the device once,
before the decode hipGraphs are captured (``GemmTuner.tune``); the captured graphs
then bake in the winner. Nothing is dispatched per call at run time except a dict
lookup. Timing is cold-cache: every timed call reads a different copy of the
weight, cycling through >= 1 GiB so the 256 MiB MALL cannot serve a weight that a
real decode step streams from HBM once per layer.
"""
from __future__ import annotations

import logging
import os
import weakref

import torch
import torch.nn.functional as F

log = logging.getLogger("hipserve.gemm")

SKINNY_CONFIGS = [(1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (2, 1), (2, 2), (2, 4), (2, 8)]
# split-K MFMA GEMM with an LDS-staged x chunk shared by 64 rows (gguf.hip, qtype 6 = bf16)
SPLITK_CONFIGS = [1, 2, 4, 8]
DG_RT = [1, 2, 3]  # 3: 64-row workgroups (4 waves x 1 row group), 33-64 rows, no GLU epilogue
DG_STEPS = [1, 2, 4, 7, 8, 12, 16, 21]  # 256-k steps per workgroup (compile-time in decode_gemm.hip)
# decode weights pre-shuffled for the packed decode GEMM, keyed by the plain
# weight's data_ptr (the plain [N, K] copy stays for prefill / hipBLASLt)
PACKED: dict[int, tuple] = {}  # data_ptr -> (weakref to the plain weight, packed copy)
# merged gate|up weights packed gate/up-interleaved for the GLU-fused decode GEMM
PACKED_GLU: dict[int, tuple] = {}
COLD_BYTES = 1 << 30
COLD_COPIES_MAX = 1024
TC_KIND = "decode_gemm_cold2"  # tuning-cache kind: bumped when the timing method changes
# Fused decode shapes are tuned as whole units — the GEMM plus the op its output
# feeds (RMSNorm / RoPE+KV write / SiLU-GLU): hipBLASLt pays a separate epilogue
# launch, the decode GEMMs pay for reading their split-K partials in the fused
# epilogue, and only timing both units picks the split count that is really best.
_EMPTY = {}
TUNE_MS = [1, 2, 4, 8, 16, 24, 32, 48, 64]
# the wide decode GEMM (csrc/kernels/decode_gemm_wide.hip, choice ("dgw", nw, mh, S)): decode
# buckets of 65-256 rows are tuned at these row counts, a bucket M using the smallest entry >= M
WIDE_MS = (128, 256)
WIDE_STEPS = [1, 2, 4, 7, 8, 14, 16, 28, 32]  # 128-k half-steps per workgroup (compile-time there)
WIDE = os.environ.get("HIPSERVE_WIDE_GEMM", "1") != "0"  # 0: hipBLASLt above 64 rows, as before (A/B)


class GemmTuner:
    def __init__(self):
        self.table: dict[tuple, object] = {}
        # best packed-layout decode GEMM per (M, N, K), whatever won overall: the choice
        # for weights kept only in the packed layout (PackedLinear)
        self.best_packed: dict[tuple, tuple] = {}
        self.report: list[dict] = []
        self.wide_fused = True  # rows above 64 are tuned as GEMM + epilogue units (the engine: TP = 1 only)

    def packed_shapes(self) -> set:
        """(N, K) whose tuned choice uses the packed layout at some M."""
        return {(N, K) for (M, N, K), c in self.table.items() if isinstance(c, tuple) and c[0] in ("dgp", "dgw")}

    def choose(self, M: int, N: int, K: int):
        if M > 64:  # the wide table: empty (hipBLASLt) unless tune() was given wide row counts
            for m in WIDE_MS if WIDE else ():
                if m >= M:
                    return self.table.get((m, N, K), "blas")
            return "blas"
        for m in TUNE_MS:
            if m >= M:
                return self.table.get((m, N, K), "blas")
        return "blas"

    def choose_packed(self, M: int, N: int, K: int) -> tuple:
        """The decode GEMM config for a packed-only weight at M <= 64: the overall winner
        when it is a packed config, else the fastest packed config timed for that M
        bucket (a split-K default when the shape was never tuned)."""
        for m in TUNE_MS:
            if m >= M:
                c = self.table.get((m, N, K))
                if isinstance(c, tuple) and c[0] == "dgp":
                    return c
                bp = self.best_packed.get((m, N, K))
                if bp is not None:
                    return bp[0]
                break
        ks = K // 256
        S = next((s for s in (8, 4, 2, 1) if ks % s == 0 and (ks // s) in DG_STEPS and -(-N // 128) * s >= 64), 1)
        return ("dgp", 1, S)

    @staticmethod
    def _time(fn, n=16, reps=5):
        """Device time per call inside a hipGraph (how decode runs), so host
        launch cost — which differs between hipBLASLt and our ops — is excluded.
        ``fn(i)`` is called with the call index (to rotate weight copies)."""
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(0)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(n):
                fn(i)
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
        del g
        return v[len(v) // 2] * 1000.0 / n

    @torch.inference_mode()
    def tune(self, shapes, device, ms=None, fused=None):
        """fused: {(N, K): spec} for projections whose output feeds a fused
        epilogue in the decode layer — ("norm",), ("rope", nq, nkv, D, mode), ("attn", nq,
        nkv, D, mode) (the fused decode attention reads the partials: GEMM alone) or
        ("glu",); those are timed as GEMM + epilogue units. Row counts in WIDE_MS time the
        wide decode GEMM's candidates the same way (``self.wide_fused`` False: as plain
        GEMMs — TP > 1, whose cross-rank epilogues stop at 64 rows)."""
        # inference mode like the engine's graph capture: the generator state tensors a
        # capture registers must not switch between inference and normal tensors
        from . import tune_cache as TC

        fused = fused or {}
        ms = [m for m in (ms or TUNE_MS) if m <= 64 or (WIDE and m in WIDE_MS)]
        for (N, K) in sorted(set(shapes)):
            spec0 = fused.get((N, K))
            specs = {M: spec0 if M <= 64 or self.wide_fused else None for M in ms}
            glu = spec0 is not None and spec0[0] == "glu"
            # a GLU-interleaved copy has no plain x W^T: a wide row of a gate|up shape that may
            # not run its GLU unit (TP > 1) is neither timed nor cached and stays on hipBLASLt
            tms = [M for M in ms if not (glu and specs[M] is None)]
            # a previous start on this device and kernel build timed this shape: reuse it
            hits = [TC.get(device, TC_KIND, [M, N, K, specs[M]]) for M in tms]
            if all(h is not None for h in hits):
                for M, h in zip(tms, hits):
                    self.table[(M, N, K)] = TC.tup(h["best"])
                    if h["bp"] is not None:
                        self.best_packed[(M, N, K)] = (TC.tup(h["bp"][0]), h["bp"][1])
                    self.report.append(dict(h["row"], cached=True))
                continue
            # enough copies that the rotation outgrows the 256 MiB MALL: 16 copies of a
            # 0.5 MB MoE router stayed cache-resident, so the timing (5.8 us for hipBLASLt)
            # missed what the engine sees between two uses of a layer (10.7 us, cold)
            ncopy = max(1, min(COLD_COPIES_MAX, -(-COLD_BYTES // (N * K * 2))))
            ws_ = [torch.randn(N, K, device=device, dtype=torch.bfloat16) for _ in range(ncopy)]
            wp_ = [pack(w, glu=glu) for w in ws_] if packable(N, K) and (not glu or N % 128 == 0) else None
            n = max(16, ncopy)
            for M in tms:
                spec = specs[M]
                x = torch.randn(M, K, device=device, dtype=torch.bfloat16)
                out = torch.empty(M, N, device=device, dtype=torch.bfloat16)
                unit = _Unit(spec, M, N, device) if spec else None
                blas_fn = (lambda i: unit.blas(F.linear(x, ws_[i % ncopy]))) if unit else \
                    (lambda i: F.linear(x, ws_[i % ncopy]))
                best, best_t = "blas", self._time(blas_fn, n=n)
                t_blas = best_t
                timed = []
                cands = self.candidates(M, N, K, packed=wp_ is not None, glu=glu) if M <= 64 else \
                    self.wide_candidates(M, N, K, glu=glu) if wp_ is not None else []
                for cfg in cands:
                    if unit is not None:
                        if cfg[0] == "sk":
                            continue
                        fn = (lambda i, cfg=cfg: unit.fused(cfg, x, ws_[i % ncopy], wp_[i % ncopy] if wp_ else None))
                    else:
                        fn = (lambda i, cfg=cfg: run_choice(cfg, out, x, ws_[i % ncopy],
                                                            wp_[i % ncopy] if wp_ else None))
                    timed.append((self._time(fn, n=n), cfg, fn))
                # confirmation round: the three fastest re-timed in interleaved rounds (median),
                # so one noisy first-round sample cannot pick a config that runs ~20 % slower in
                # the engine (a box once kept the 128-row o_proj body at 12 us over the 64-row
                # one at 9.7 us on a 2 % first-round difference)
                finalists = sorted(timed, key=lambda e: e[0])[:3]
                rounds = {id(e): [e[0]] for e in finalists}
                for _ in range(2):
                    for e in finalists:
                        rounds[id(e)].append(self._time(e[2], n=n))
                for e in finalists:
                    v = sorted(rounds[id(e)])
                    t, cfg = v[len(v) // 2], e[1]
                    if cfg[0] == "dgp":
                        bp = self.best_packed.get((M, N, K))
                        if bp is None or t < bp[1]:
                            self.best_packed[(M, N, K)] = (cfg, t)
                    if t < best_t * (0.97 if best == "blas" else 1.0):
                        best, best_t = cfg, t
                if (M, N, K) not in self.best_packed:  # no packed finalist: the fastest packed config
                    dg = [(t, cfg) for t, cfg, _ in timed if cfg[0] == "dgp"]
                    if dg:
                        t, cfg = min(dg)
                        self.best_packed[(M, N, K)] = (cfg, t)
                self.table[(M, N, K)] = best
                row = {"M": M, "N": N, "K": K, "unit": spec[0] if spec else "gemm",
                       "blas_us": round(t_blas, 1), "best": str(best), "best_us": round(best_t, 1),
                       "best_TBps": round(N * K * 2 / best_t / 1e6, 2)}
                self.report.append(row)
                bp = self.best_packed.get((M, N, K))
                TC.put(device, TC_KIND, [M, N, K, spec],
                       {"best": best, "bp": [bp[0], bp[1]] if bp else None, "row": row})
            del ws_, wp_
        TC.flush()
        return self.report

    @staticmethod
    def candidates(M, N, K, packed=False, glu=False):
        out = []
        for rt in DG_RT:
            if rt == 3 and (glu or not 32 < M <= 64):
                continue
            tiles = -(-N // (64 if rt == 3 else 128))
            for ns in DG_STEPS:
                if K % (256 * ns):
                    continue
                sp = K // (256 * ns)
                # under 64 workgroups only for small weights (an MoE router [E, H]: 0.5 MB,
                # where hipBLASLt took 11 us at 64 rows); larger ones must fill the chip
                if (sp > 1 and N % 8) or tiles * sp > 4096 or (tiles * sp < 64 and N * K > (1 << 21)):
                    continue
                out.append(("dg", rt, sp))
                if packed:
                    out.append(("dgp", rt, sp))
        for rt, kw in SKINNY_CONFIGS:
            if K % (256 * kw) == 0:
                out.append(("sk", rt, kw))
        return out

    @staticmethod
    def wide_candidates(M, N, K, glu=False):
        """("dgw", nw, mh, S) for a row count in WIDE_MS: every (nw, mh) the kernel runs at M,
        each with the split that first fills the 256 CUs and its two neighbours. A split whose
        fp32 partials (S M N 4 bytes) outweigh the weight (N K 2) is pruned: small-N
        projections fill the chip with M-halves and 128-row workgroups before split-K."""
        out = []
        if K % 256 or N % (128 if glu else 8):
            return out
        for nw, mh in ([(128, 1), (256, 1)] if M <= 128 else [(128, 2), (256, 2), (256, 1)]):
            tiles = -(-N // nw)
            ss = [S for S in range(1, K // 128 + 1)
                  if K % (128 * S) == 0 and K // (128 * S) in WIDE_STEPS and (S == 1 or S * M * 4 <= K * 2)]
            if not ss:
                continue
            fill = next((i for i, S in enumerate(ss) if tiles * S * mh >= 256), len(ss) - 1)
            out += [("dgw", nw, mh, S) for S in ss[max(0, fill - 1):fill + 2]]
        return out[:10]


class _Unit:
    """A decode GEMM together with the op its output feeds, for tuning: the
    hipBLASLt path runs the unfused epilogue kernel, a decode-GEMM config runs
    the split-K partial GEMM + the fused epilogue it enables (or, for a plain
    dg config on a GLU shape, the GEMM + silu_and_mul)."""

    def __init__(self, spec, M, N, device):
        op = torch.ops.hipserve
        self.op, self.spec, self.M, self.N = op, spec, M, N
        bf = dict(device=device, dtype=torch.bfloat16)
        self.kind = spec[0]
        if self.kind == "norm":
            self.res = torch.randn(M, N, **bf)
            self.w = torch.ones(N, **bf)
            self.y = torch.empty(M, N, **bf)
        elif self.kind in ("rope", "attn"):
            _, self.nq, self.nkv, self.D, self.mode = spec
            nb = -(-M // 16) + 1
            self.kc = torch.zeros(nb, self.nkv, 16, self.D, **bf)
            self.vc = torch.zeros(nb, self.nkv, self.D, 16, **bf)
            self.pos = torch.arange(M, device=device, dtype=torch.long)
            self.slots = torch.arange(M, device=device, dtype=torch.long)
            self.cs = torch.rand(4096, self.D, device=device, dtype=torch.float32)
            self.qkv = torch.empty(M, N, **bf)
        elif self.kind == "glu":
            self.act = torch.empty(M, N // 2, **bf)

    def blas(self, y):
        op = self.op
        if self.kind == "norm":
            op.fused_add_rmsnorm(self.y, y, self.res, self.w, 1e-5)
        elif self.kind in ("rope", "attn"):  # hipBLASLt: qkv rows, then the RoPE + KV write kernel
            op.rope_cache(y, self.pos, self.slots, self.cs, self.kc, self.vc, self.nq, self.nkv, self.D, self.mode)
        else:
            op.silu_and_mul(self.act, y)

    def fused(self, cfg, x, w, wp):
        op, M, N = self.op, self.M, self.N
        if cfg[0] == "dgw":  # the wide GEMM: GLU form, or partials into the same epilogues
            _, nw, mh, S = cfg
            if self.kind == "glu":
                ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device) if S > 1 else \
                    _empty(x.device)[1]
                return op.decode_gemm_wide_glu(self.act, x, wp, ws, N, nw, mh, S)
            ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device)
            op.decode_gemm_wide_partial(ws, x, wp, N, nw, mh, S)
            return self.epilogue(ws, S)
        kind, rt, S = cfg
        packed = kind == "dgp" and wp is not None
        if self.kind == "glu":
            if packed:  # GLU in the GEMM epilogue (S = 1) or the GLU reduce (S > 1)
                ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device) if S > 1 else \
                    _empty(x.device)[1]
                op.decode_gemm_glu(self.act, x, wp, ws, N, rt, S)
            else:
                y = torch.empty(M, N, dtype=x.dtype, device=x.device)
                decode_gemm(y, x, w, rt, S)
                op.silu_and_mul(self.act, y)
            return
        ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device)
        op.decode_gemm_partial(ws, x, wp if packed else w, N, rt, S, packed)
        self.epilogue(ws, S)

    def epilogue(self, ws, S):
        op = self.op
        if self.kind == "norm":
            op.splitk_add_rmsnorm(self.y, self.res, ws, S, self.w, 1e-5)
        elif self.kind == "attn":
            pass  # the fused decode attention sums the partials (RoPE + KV write inside)
        else:
            op.splitk_rope_cache(self.qkv, ws, S, self.pos, self.slots, self.cs, self.kc, self.vc,
                                 self.nq, self.nkv, self.D, self.mode)


TUNER = GemmTuner()


def _empty(device):
    e = _EMPTY.get(device)
    if e is None:
        e = _EMPTY[device] = (torch.empty(0, dtype=torch.int16, device=device),
                              torch.empty(0, dtype=torch.float32, device=device))
    return e


def splitk_gemm(out, x, w, splits):
    M, K = x.shape
    N = w.shape[0]
    e16, e32 = _empty(x.device)
    ws = torch.empty(splits, M, N, dtype=torch.float32, device=x.device) if splits > 1 else e32
    torch.ops.hipserve.gguf_gemm(out, x, w.view(torch.uint8), e16, e16, 6, 2 * K, N, K, ws, splits)
    return out


def decode_gemm(out, x, w, rt, splits):
    M, N = x.shape[0], w.shape[0]
    ws = (torch.empty(splits * M * N, dtype=torch.float32, device=x.device) if splits > 1
          else _empty(x.device)[1])
    torch.ops.hipserve.decode_gemm(out, x, w, ws, rt, splits)
    return out


def packable(N: int, K: int) -> bool:
    return K % 256 == 0 and N % 8 == 0


def pack(w: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """Pre-shuffle a [N, K] bf16 weight for ``decode_gemm_packed`` (flat, N padded
    to 128). glu: [gate; up] weight, tiles interleave 64 gate + 64 up rows."""
    N, K = w.shape
    out = torch.empty(-(-N // 128) * 128 * K, dtype=w.dtype, device=w.device)
    torch.ops.hipserve.pack_decode_weight(out, w.contiguous(), glu)
    return out


class PackedLinear:
    """A dense bf16 projection kept ONLY in the packed layout of ``pack_decode_weight``
    (one weight layout for prefill and decode, no second resident copy).
    The decode GEMMs (``decode_gemm_packed`` / ``decode_gemm_glu`` / the split-K partial
    kernels) and the packed prefill GEMM (csrc/kernels/prefill_gemm_packed.hip) read it
    directly. ``glu``: a merged [gate; up] weight packed gate/up-interleaved per 128-row
    tile (the GLU epilogues pair gate and up in registers). ``unpack()`` rebuilds the
    row-major [N, K] matrix (tests, fp32 oracles, rare fallbacks) — never on a hot path."""

    def __init__(self, wp: torch.Tensor, N: int, K: int, glu: bool = False):
        self.wp, self.N, self.K, self.glu = wp, N, K, glu
        self.shape = (N, K)
        self.dtype, self.device = wp.dtype, wp.device
        self.is_cuda = wp.is_cuda

    def dim(self) -> int:
        return 2

    def numel(self) -> int:
        return self.N * self.K

    def element_size(self) -> int:
        return self.wp.element_size()

    def data_ptr(self) -> int:
        return self.wp.data_ptr()

    def unpack(self) -> torch.Tensor:
        """Row-major [N, K] (the inverse of pack_decode_weight's permutation)."""
        T, KS = -(-self.N // 128), self.K // 256
        # packed [t][ks][rg][s][lane = g*16 + c][e] holds W[128 t + 16 rg + c][256 ks + 32 s + 8 g + e]
        v = self.wp.view(T, KS, 8, 8, 4, 16, 8).permute(0, 2, 5, 1, 3, 4, 6).reshape(T, 128, self.K)
        if self.glu:  # tile t: 64 gate rows [64t, 64t + 64), then the matching up rows
            v = v.view(T, 2, 64, self.K)
            return torch.cat([v[:, 0].reshape(-1, self.K), v[:, 1].reshape(-1, self.K)])[:self.N]
        return v.reshape(T * 128, self.K)[:self.N]

    def float(self) -> torch.Tensor:
        return self.unpack().float()

    def to(self, *a, **k) -> torch.Tensor:
        return self.unpack().to(*a, **k)

    def t(self) -> torch.Tensor:
        return self.unpack().t()


def _lookup(reg, w):
    e = reg.get(w.data_ptr())
    if e is None:
        return None
    ref, wp = e
    if ref() is not w:  # a freed weight's address reused by another tensor
        reg.pop(w.data_ptr(), None)
        return None
    return wp


def packed_of(w):
    """The packed copy of ``w`` — only if registered for this very tensor (or ``w``'s
    own layout when it is a ``PackedLinear`` without GLU interleaving)."""
    if isinstance(w, PackedLinear):
        return None if w.glu else w.wp
    return _lookup(PACKED, w)


def glu_of(w):
    if isinstance(w, PackedLinear):
        return w.wp if w.glu else None
    return _lookup(PACKED_GLU, w)


def register_packed(w: torch.Tensor, glu: bool = False) -> torch.Tensor:
    reg = PACKED_GLU if glu else PACKED
    wp = _lookup(reg, w)
    if wp is None:
        wp = pack(w, glu)
        reg[w.data_ptr()] = (weakref.ref(w), wp)
    return wp


def decode_gemm_packed(out, x, wp, N, rt, splits):
    M = x.shape[0]
    ws = (torch.empty(splits * M * N, dtype=torch.float32, device=x.device) if splits > 1
          else _empty(x.device)[1])
    torch.ops.hipserve.decode_gemm_packed(out, x, wp, ws, N, rt, splits)
    return out


def decode_gemm_wide(out, x, wp, N, nw, mh, splits):
    M = x.shape[0]
    ws = (torch.empty(splits * M * N, dtype=torch.float32, device=x.device) if splits > 1
          else _empty(x.device)[1])
    torch.ops.hipserve.decode_gemm_wide(out, x, wp, ws, N, nw, mh, splits)
    return out


def wide_choice(M: int, w, glu: bool = False):
    """(("dgw", nw, mh, S), packed weight) when the tuner picked the wide decode GEMM for
    ``w`` at 64 < M <= 256 and its (GLU-)packed copy exists; None: hipBLASLt / packed prefill."""
    if not 64 < M <= 256 or not TUNER.table:
        return None
    c = TUNER.choose(M, w.shape[0], w.shape[1])
    if not isinstance(c, tuple) or c[0] != "dgw":
        return None
    wp = glu_of(w) if glu else packed_of(w)
    return None if wp is None else (c, wp)


def fused_choice(M: int, w):
    """(choice, packed weight or None) when the tuned decode GEMM for ``w`` at M can
    write split-K partials for a fused epilogue; None for hipBLASLt / skinny."""
    if M > 64:
        return wide_choice(M, w) if isinstance(w, (torch.Tensor, PackedLinear)) else None
    if isinstance(w, PackedLinear):
        if w.glu:
            return None
        return TUNER.choose_packed(M, w.N, w.K), w.wp
    if not isinstance(w, torch.Tensor) or not TUNER.table:
        return None
    c = TUNER.choose(M, w.shape[0], w.shape[1])
    if not isinstance(c, tuple) or c[0] not in ("dg", "dgp"):
        return None
    wp = packed_of(w) if c[0] == "dgp" else None
    return c, wp


def gemm_partial(x, w, fc):
    """Run fused_choice ``fc`` on x writing fp32 partials; returns (ws, S)."""
    M, N = x.shape[0], w.shape[0]
    if fc[0][0] == "dgw":
        (_, nw, mh, S), wp = fc
        ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device)
        torch.ops.hipserve.decode_gemm_wide_partial(ws, x, wp, N, nw, mh, S)
        return ws, S
    (kind, rt, S), wp = fc
    ws = torch.empty(S * M * N, dtype=torch.float32, device=x.device)
    packed = wp is not None
    torch.ops.hipserve.decode_gemm_partial(ws, x, wp if packed else w, N, rt, S, packed)
    return ws, S


def glu_choice(M: int, w):
    """(rt, S, glu-packed weight) when the tuned decode GEMM for the merged gate|up
    weight ``w`` at M is the packed kernel and a GLU-interleaved copy exists; above 64
    rows (nw, mh, S, glu-packed weight) of the wide kernel."""
    if M > 64:
        wc = wide_choice(M, w, glu=True) if isinstance(w, (torch.Tensor, PackedLinear)) else None
        return None if wc is None else (*wc[0][1:], wc[1])
    if isinstance(w, PackedLinear):
        if not w.glu:
            return None
        c = TUNER.choose_packed(M, w.N, w.K)
        return c[1], c[2], w.wp
    if not isinstance(w, torch.Tensor) or not TUNER.table:
        return None
    c = TUNER.choose(M, w.shape[0], w.shape[1])
    wp = glu_of(w)
    if not isinstance(c, tuple) or c[0] != "dgp" or wp is None:
        return None
    return c[1], c[2], wp


def gemm_glu(x, w, gc):
    """act[M, N/2] = silu(x Wg^T) * (x Wu^T) in one decode GEMM (+ GLU reduce if S > 1)."""
    *cfg, S, wp = gc  # cfg: (rt,), or (nw, mh) of the wide kernel
    M, N = x.shape[0], w.shape[0]
    act = torch.empty(M, N // 2, dtype=x.dtype, device=x.device)
    ws = (torch.empty(S * M * N, dtype=torch.float32, device=x.device) if S > 1 else _empty(x.device)[1])
    if len(cfg) == 2:
        torch.ops.hipserve.decode_gemm_wide_glu(act, x, wp, ws, N, cfg[0], cfg[1], S)
    else:
        torch.ops.hipserve.decode_gemm_glu(act, x, wp, ws, N, cfg[0], S)
    return act


def run_choice(c, out, x, w, wp=None):
    if c[0] == "dgw":  # packed layout only: linear() takes hipBLASLt for a weight without the copy
        return decode_gemm_wide(out, x, wp if wp is not None else packed_of(w), out.shape[1], c[1], c[2], c[3])
    if c[0] == "dgp":
        if wp is None:
            wp = packed_of(w)
        if wp is None:  # weight was not packed (e.g. memory): same kernel, plain layout
            return decode_gemm(out, x, w, c[1], c[2])
        return decode_gemm_packed(out, x, wp, w.shape[0], c[1], c[2])
    if c[0] == "dg":
        return decode_gemm(out, x, w, c[1], c[2])
    if c[0] == "sk":
        torch.ops.hipserve.skinny_gemm(out, x, w, c[1], c[2])
        return out
    if c[0] == "splitk":
        return splitk_gemm(out, x, w, c[1])
    raise ValueError(c)


# packed prefill GEMM (prefill_gemm_packed.hip) workgroup shape: 1 = 128 x 512, 2 = 256 x 256
PW_WM = int(__import__("os").environ.get("HIPSERVE_PW_WM", "1"))
# weight register sets in flight (2 or 4 32-deep slots ahead of the MFMAs)
PW_RW = int(__import__("os").environ.get("HIPSERVE_PW_RW", "4"))
# workgroups: 0 = persistent (one per CU walking the tiles), large = one tile each. One tile
# per workgroup measured 2-5 % faster at 8192 rows (profiles/r4_pw_scaling_v3.log)
PW_GRID = int(__import__("os").environ.get("HIPSERVE_PW_GRID", str(1 << 30)))


def packed_prefill(x: torch.Tensor, w: PackedLinear, epi: int = 0, out: torch.Tensor | None = None,
                   bias: torch.Tensor | None = None) -> torch.Tensor:
    """Prefill-sized GEMM on the packed layout: epi 0 out = x W^T (+ bias), 1 out (the
    residual) += x W^T, 2 / 3 (glu weights) out = silu / gelu_tanh(gate) * up."""
    M = x.shape[0]
    if out is None:
        out = torch.empty(M, w.N // 2 if epi in (2, 3) else w.N, device=x.device, dtype=x.dtype)
    torch.ops.hipserve.prefill_gemm_packed(out, x, w.wp, w.N, epi, bias, PW_WM, PW_GRID, PW_RW)
    return out


def packed_linear(x: torch.Tensor, w: PackedLinear) -> torch.Tensor:
    """out = x W^T for a packed-only (non-GLU) weight: the packed decode GEMM up to 64
    rows, the wide one up to 256 where the tuner picked it, the packed prefill GEMM else."""
    assert not w.glu, "a GLU-interleaved weight has no plain x W^T (use packed_glu)"
    M = x.shape[0]
    if x.stride(1) != 1 or x.stride(0) % 8:
        x = x.contiguous()
    if M <= 64:
        c = TUNER.choose_packed(M, w.N, w.K)
        out = torch.empty(M, w.N, device=x.device, dtype=x.dtype)
        return decode_gemm_packed(out, x, w.wp, w.N, c[1], c[2])
    wc = wide_choice(M, w)
    if wc is not None:
        out = torch.empty(M, w.N, device=x.device, dtype=x.dtype)
        return run_choice(wc[0], out, x, w, wc[1])
    return packed_prefill(x, w)


def packed_glu(x: torch.Tensor, w: PackedLinear, gelu: bool = False) -> torch.Tensor:
    """act = silu / gelu_tanh(x Wg^T) * (x Wu^T) for a GLU-packed merged gate|up weight."""
    assert w.glu
    M = x.shape[0]
    if x.stride(1) != 1 or x.stride(0) % 8:
        x = x.contiguous()
    if M <= 64 and not gelu:
        c = TUNER.choose_packed(M, w.N, w.K)
        return gemm_glu(x, w, (c[1], c[2], w.wp))
    gc = None if gelu else glu_choice(M, w)
    if gc is not None:
        return gemm_glu(x, w, gc)
    return packed_prefill(x, w, 3 if gelu else 2)


def linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if isinstance(w, PackedLinear):
        return packed_linear(x, w)
    M = x.shape[0]
    if M <= 256 and x.is_cuda and TUNER.table:
        c = TUNER.choose(M, w.shape[0], w.shape[1])
        if c != "blas" and x.stride(1) == 1 and x.stride(0) % 8 == 0 and (c[0] != "dgw" or packed_of(w) is not None):
            out = torch.empty(M, w.shape[0], device=x.device, dtype=x.dtype)
            return run_choice(c, out, x, w)
    return F.linear(x, w)
