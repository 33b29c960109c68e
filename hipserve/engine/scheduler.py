"""Continuous-batching scheduler with chunked prefill, prefix caching and
recompute preemption (SURVEY §3.C engine core, §7.4 hard part 4).

Each step builds one batch under a token budget (``max_num_batched_tokens``):
running sequences first (1 token per decoding sequence, the next chunk for a
sequence still in prefill), then newly admitted ones (their prompt minus any
prefix-cache hit, chunked to the remaining budget). When the KV pool runs dry
the most recently admitted running sequence is preempted (blocks freed, state
reset to recompute) — FCFS fairness, no swap space needed with 288 GB HBM.

Image blocks (Gemma-3: the tokens of one image attend to each other in both
directions, ``Sequence.mm.blocks``): a prefill chunk never ends inside one, because
the block's earlier rows need the later rows' keys. A chunk that would is trimmed
back to the block's start; a chunk that starts at (or, after a prefix-cache hit,
inside) a block takes the whole rest of it, and where the sequences ahead left less
than that, the sequence waits one step with that much of the next step's budget
held for it.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field

from .block_manager import BlockManager
from .request import Sequence, Status


@dataclass
class ScheduledSeq:
    seq: Sequence
    start: int            # first token index computed this step
    end: int              # one past the last token index computed this step

    @property
    def num_tokens(self) -> int:
        return self.end - self.start

    @property
    def samples(self) -> bool:
        """The step's last row is the sequence's last known token -> sample."""
        return self.end == self.seq.num_tokens


@dataclass
class SchedulerOutput:
    prefill: list[ScheduledSeq] = field(default_factory=list)
    decode: list[ScheduledSeq] = field(default_factory=list)
    preempted: list[Sequence] = field(default_factory=list)

    @property
    def num_tokens(self) -> int:
        return sum(s.num_tokens for s in self.prefill) + len(self.decode)

    @property
    def empty(self) -> bool:
        return not self.prefill and not self.decode


class Scheduler:
    def __init__(self, blocks: BlockManager, max_num_seqs: int, max_num_batched_tokens: int,
                 max_model_len: int):
        self.blocks = blocks
        self.max_num_seqs = max_num_seqs
        self.max_tokens = max_num_batched_tokens
        self.max_model_len = max_model_len
        self.waiting: deque[Sequence] = deque()
        self.running: list[Sequence] = []
        self.num_preemptions = 0
        self._held: Sequence | None = None  # waits for a whole image block (module docstring)

    @staticmethod
    def _chunk(seq: Sequence, n: int) -> int:
        """Tokens of ``seq``'s next prefill chunk given room for ``n``: ``n``, less where
        the chunk would end inside an image block (0: the block it starts in needs more)."""
        mm = seq.mm
        if mm is None or not mm.blocks or n <= 0:
            return max(n, 0)
        start = seq.num_computed_tokens
        a = mm.block_start(start + n)
        return n if a == start + n else max(a - start, 0) if a > start else 0

    @staticmethod
    def _block_need(seq: Sequence) -> int:
        """Tokens up to the end of the image block that ``seq``'s next chunk starts in."""
        mm, start = seq.mm, seq.num_computed_tokens
        if mm is None:
            return 0
        return max((b - start for a, b in mm.blocks if a <= start < b), default=0)

    def add(self, seq: Sequence):
        seq.status = Status.WAITING
        self.waiting.append(seq)

    def abort(self, request_id: str) -> Sequence | None:
        for q in (self.running, self.waiting):
            for s in list(q):
                if s.request_id == request_id:
                    q.remove(s)
                    self.blocks.free(s)
                    s.status = Status.FINISHED
                    s.finish_reason = "abort"
                    return s
        return None

    def has_unfinished(self) -> bool:
        return bool(self.waiting or self.running)

    @property
    def num_running(self):
        return len(self.running)

    @property
    def num_waiting(self):
        return len(self.waiting)

    def _preempt(self, seq: Sequence, out: SchedulerOutput):
        self.running.remove(seq)
        self.blocks.free(seq)
        seq.num_computed_tokens = 0
        seq.status = Status.PREEMPTED
        self.waiting.appendleft(seq)
        out.preempted.append(seq)
        self.num_preemptions += 1

    def schedule(self) -> SchedulerOutput:
        out = SchedulerOutput()
        budget = self.max_tokens
        scheduled_ids = set()
        # the sequence that found no room for its image block last step: the others leave it that room
        held, self._held, reserve = self._held, None, 0
        if held is not None and (held in self.running or (
                self.waiting and self.waiting[0] is held and len(self.running) < self.max_num_seqs)):
            reserve = min(self._block_need(held), budget)
        # ---- 1. running sequences (FCFS order; victims taken from the tail)
        i = 0
        while i < len(self.running) and budget > 0:
            seq = self.running[i]
            room = budget if seq is held else budget - reserve
            n = self._chunk(seq, min(seq.num_uncomputed, room)) if seq.is_prefill else min(1, room)
            if n <= 0:  # this step has no room for it (the held room, or an image block that needs more)
                if seq.is_prefill and room > 0 and self._held is None:
                    self._held = seq
                i += 1
                continue
            if seq is held:
                reserve = 0
            target = seq.num_computed_tokens + n
            while not self.blocks.can_grow(seq, target):
                victim = self.running[-1]
                if victim is seq:
                    break
                self._preempt(victim, out)
            if not self.blocks.can_grow(seq, target):
                self._preempt(seq, out)
                continue
            self.blocks.grow(seq, target)
            ss = ScheduledSeq(seq, seq.num_computed_tokens, target)
            (out.prefill if seq.is_prefill else out.decode).append(ss)
            scheduled_ids.add(id(seq))
            budget -= n
            i += 1
        # ---- 2. admit waiting sequences (no admission in a step that preempted)
        if not out.preempted:
            while self.waiting and budget > 0 and len(self.running) < self.max_num_seqs:
                seq = self.waiting[0]
                # cached positions have no hidden states to score: no hit while prompt log-probs are incomplete
                if seq.num_computed_tokens == 0 and not seq.block_ids and not seq.wants_prompt_logprobs:
                    self.blocks.match_prefix(seq)
                room = budget if seq is held else budget - reserve
                n = self._chunk(seq, min(seq.num_uncomputed, room))
                if n <= 0:  # no room this step: it stays first in line (its prefix hit kept)
                    if room > 0 and self._held is None:
                        self._held = seq
                    break
                if seq is held:
                    reserve = 0
                target = seq.num_computed_tokens + n
                # the watermark protects RUNNING sequences' growth: with nothing running
                # (and nothing admitted yet this step) it would only block admission
                # forever for a chunk that fits the free pool exactly
                idle = not self.running and not out.prefill
                if not self.blocks.can_grow(seq, target, watermark=not idle):
                    if not self.running and not out.prefill:
                        # nothing else can free memory: the request can never fit
                        if not self.blocks.can_grow(seq, target):
                            self.waiting.popleft()
                            self.blocks.free(seq)
                            seq.status = Status.FINISHED
                            seq.finish_reason = "length"
                            out.preempted.append(seq)
                            continue
                    self.blocks.free(seq)  # undo prefix hit, retry next step
                    seq.num_computed_tokens = 0
                    break
                self.waiting.popleft()
                self.blocks.grow(seq, target)
                seq.status = Status.RUNNING
                self.running.append(seq)
                out.prefill.append(ScheduledSeq(seq, seq.num_computed_tokens, target))
                budget -= n
        return out

    def finish(self, seq: Sequence, reason: str):
        seq.status = Status.FINISHED
        seq.finish_reason = reason
        if seq in self.running:
            self.running.remove(seq)
        self.blocks.free(seq)
