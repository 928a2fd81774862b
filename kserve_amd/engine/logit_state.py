"""Per-request device state of the in-graph logit processors.

Decode windows replay a captured graph with no host work per token, so what
the processors need per request lives on the device: a token histogram
(`counts`, exact int32) for the presence / frequency / repetition penalties
and the request's `logit_bias` list. A request that sets any processor field
takes a slot for its lifetime; the graph reads the slot of each row from a
static buffer (-1: no processors, the row is skipped).

The four buffers are zero-filled, allocated once and only written in place:
their pointers are baked into captured graphs (the rule of the LoRA stacks).
Memory is `slots x vocab x 4 B` for the counts (64 slots at V = 128256:
33 MB) plus `slots x MAX_BIAS x 8 B`.

Invariant: `counts[slot]` is the histogram of the first `synced` entries of
the request's `output_token_ids`. Single steps (prefill sampling, k == 1,
fallback) sample on the host and only leave `synced` behind; `catch_up`
adds the missing tokens before a window, the window's graph adds its own,
and the engine calls `mark_synced` afterwards. Nothing in the engine rewrites
`output_token_ids` (recompute preemption keeps them, see
`Scheduler._preempt`), so a slot is never rebuilt, only released.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import torch

from kserve_amd import ops
from kserve_amd.engine.request import Request
from kserve_amd.engine.sampling_params import SamplingParams

# bias entries per slot; a request with more stays on the host path
MAX_BIAS = 512


def wants_processors(sp: SamplingParams) -> bool:
    """True when the request sets one of the five logit-processor fields."""
    return bool(
        sp.presence_penalty != 0.0
        or sp.frequency_penalty != 0.0
        or sp.repetition_penalty != 1.0
        or sp.logit_bias
        or sp.min_p != 0.0
    )


class LogitProcessorState:
    def __init__(self, slots: int, vocab: int, device):
        if slots < 1:
            raise ValueError("LogitProcessorState needs at least one slot")
        self.slots = slots
        self.vocab = vocab
        self.device = torch.device(device)
        dev = self.device
        self.counts = torch.zeros((slots, vocab), dtype=torch.int32, device=dev)
        self.bias_ids = torch.zeros((slots, MAX_BIAS), dtype=torch.int32, device=dev)
        self.bias_vals = torch.zeros(
            (slots, MAX_BIAS), dtype=torch.float32, device=dev
        )
        self.bias_len = torch.zeros(slots, dtype=torch.int32, device=dev)
        self._free: List[int] = list(range(slots - 1, -1, -1))  # pop() -> 0 first
        self._slot: Dict[str, int] = {}
        self._synced: Dict[str, int] = {}

    # -- queries --------------------------------------------------------------
    @staticmethod
    def eligible(sp: SamplingParams) -> bool:
        return not sp.logit_bias or len(sp.logit_bias) <= MAX_BIAS

    def slot_of(self, request_id: str) -> int:
        """The request's slot, -1 if it holds none."""
        return self._slot.get(request_id, -1)

    def synced(self, request_id: str) -> int:
        return self._synced[request_id]

    @property
    def num_free(self) -> int:
        return len(self._free)

    # -- life cycle -----------------------------------------------------------
    def acquire(self, req: Request) -> Optional[int]:
        """The request's slot, taking a free one if it holds none: counts row
        zeroed, bias list written, nothing synced. None when no slot is free."""
        slot = self._slot.get(req.request_id)
        if slot is not None:
            return slot
        if not self.eligible(req.sampling_params):
            raise ValueError(f"more than {MAX_BIAS} logit_bias entries")
        if not self._free:
            return None
        slot = self._free.pop()
        self.counts[slot].zero_()
        # the host path's filter; dict keys, so unique (the kernel needs that)
        items = [
            (int(t), float(v))
            for t, v in (req.sampling_params.logit_bias or {}).items()
            if 0 <= int(t) < self.vocab
        ]
        n = len(items)
        if n:
            self.bias_ids[slot, :n] = torch.tensor(
                [t for t, _ in items], dtype=torch.int32
            )
            self.bias_vals[slot, :n] = torch.tensor(
                [v for _, v in items], dtype=torch.float32
            )
        self.bias_len[slot] = n
        self._slot[req.request_id] = slot
        self._synced[req.request_id] = 0
        return slot

    def release(self, request_id: str) -> None:
        slot = self._slot.pop(request_id, None)
        if slot is None:
            return
        self._synced.pop(request_id, None)
        self._free.append(slot)

    def catch_up(self, reqs: List[Request]) -> int:
        """Add every output token the counts have not seen yet, for all the
        given requests that hold a slot, in ONE launch. Normally 0 or 1 token
        per request (the one sampled from the prefill logits). Returns the
        number of pairs applied."""
        slots: List[int] = []
        toks: List[int] = []
        for r in reqs:
            slot = self._slot.get(r.request_id)
            if slot is None:
                continue
            done = self._synced[r.request_id]
            new = r.output_token_ids[done:]
            if new:
                slots.extend([slot] * len(new))
                toks.extend(new)
                self._synced[r.request_id] = done + len(new)
        if toks:
            dev = self.device
            ops.token_count_add(
                self.counts,
                torch.tensor(slots, dtype=torch.int32).to(dev),
                torch.tensor(toks, dtype=torch.int64).to(dev),
            )
        return len(toks)

    def mark_synced(self, req: Request) -> None:
        """After a processed window: the graph counted every token the
        request took (a request that stopped early is finished and about to
        be released)."""
        if req.request_id in self._slot:
            self._synced[req.request_id] = len(req.output_token_ids)
