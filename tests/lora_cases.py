"""Cases for the batched multi-LoRA decode ops (``ops.lora_shrink`` +
``ops.lora_expand_add``), an fp64 reference of their own and a derived
comparator. Helper module: imported by test_lora_cases.py (CPU) and
test_gpu_lora_ops.py; not collected.

Every case is built so that the mistakes such a kernel can make move some
output by far more than the allowance:

* **Slots.** ``S = 4`` adapter slots of rank capacity ``R = 64`` hold ranks
  4, 8, 16 and 64 with four different scales. ``slot_idx`` is interleaved
  and non-monotone, has -1 rows (base model / graph padding) mixed in and
  one row with ``slot_idx = S`` (out of range); both kinds must come back
  bit-identical. One slot per case (it rotates with the case number, so
  every rank is used and every rank is left out somewhere) is referenced by
  no row.
* **Poison.** The unreferenced slot's whole A and B, and every A row / B
  column at or past ``round_up(rank, 8)`` of the used slots, hold +-3e38.
  Rows ``[rank, round_up(rank, 8))`` are zero, as the manager's zero-filled
  stacks make them. Any read of poison breaks the allowance by orders of
  magnitude.
* **Strided y.** ``y`` is a view into a wider bf16 buffer pre-filled with a
  sentinel, and the delta lands at ``out_offset`` 0 or 64 of the view. Every
  element outside ``[out_offset, out_offset + N)`` must keep its bits.

The comparator is elementwise

    |got - ref| <= 2^-8 |ref| + (K + R + 2) 2^-24 absmass + 1e-6
    absmass = |y| + |scale| sum_r |B[n, r]| sum_k |x_k| |A[r, k]|

The first term is the single bf16 rounding of the output. The second is the
standard worst-case bound of fp32 summation, in any order, over what was
actually summed: bf16 x bf16 products are exact in fp32, the shrink sum has
at most K - 1 roundings, the expand sum R (products of an fp32 and a bf16
round once each, or not at all under FMA), scale and the add to y one each.
It is derived, not fitted. The reference computes in fp64 from the
bf16-rounded inputs.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional

import torch

S = 4
R = 64
RANKS = (4, 8, 16, 64)
SCALES = (0.5, 2.0, 1.0, 1.5)
KS = (64, 512, 1088)
NS = (64, 256, 1024)
TS = (1, 3, 33, 130)
POISON = 3e38
SENTINEL = 777.0
LEAD = 8        # columns of the wide buffer in front of the y view
TAIL = 8        # columns behind it
VIEW_PAD = 80   # the view is N + VIEW_PAD wide: room for out_offset 64
OUT_ULP = 2.0 ** -8
EPS32 = 2.0 ** -24
ABS_FLOOR = 1e-6


@dataclass(frozen=True)
class Case:
    name: str
    K: int
    N: int
    T: int
    off: int
    unused_slot: int
    seed: int


def _cases() -> List[Case]:
    out = []
    i = 0
    for K in KS:
        for N in NS:
            for T in TS:
                off = 64 * (i % 2)
                # + i // 4: T advances fastest, so a plain i % 4 would tie
                # the unused slot to T
                unused = (i + i // 4) % S
                out.append(Case(f"k{K}_n{N}_t{T}_o{off}_u{unused}", K, N, T,
                                off, unused, 1000 + i))
                i += 1
    return out


CASES = _cases()
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)


def round_up8(r: int) -> int:
    return (r + 7) // 8 * 8


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


def _slot_pattern(case: Case) -> List[int]:
    """Interleaved, non-monotone slots over the used ones, with -1 rows and
    one out-of-range row (= S) where the batch has room."""
    used = [s for s in range(S) if s != case.unused_slot]
    T = case.T
    if T == 1:
        return [used[case.seed % len(used)]]
    if T == 3:
        return [used[2], -1, used[0]] if case.seed % 2 else [used[1], S, -1]
    order = [used[2], used[0], -1, used[1], used[0], used[2], used[1], -1]
    slots = [order[(t * 3 + t // 8) % len(order)] for t in range(T)]
    slots[T // 2] = S          # out of range
    slots[0] = used[1]
    slots[T - 1] = -1
    return slots


@functools.lru_cache(maxsize=None)
def build(case: Case) -> SimpleNamespace:
    """Inputs of a case as float32 CPU tensors holding bf16-exact values
    (``scale`` fp32, ``ranks`` / ``slot_idx`` int32). ``wide`` is the whole
    y buffer [T, LEAD + N + VIEW_PAD + TAIL]. Cached: do not modify."""
    g = torch.Generator().manual_seed(case.seed)
    K, N, T = case.K, case.N, case.T
    x = _bf16(torch.randn(T, K, generator=g))
    a = _bf16(torch.randn(S, R, K, generator=g) / K ** 0.5)
    b = _bf16(torch.randn(S, N, R, generator=g))
    sgn_a = torch.ones(R, K)
    sgn_a[:, 1::2] = -1.0
    sgn_a[1::2] *= -1.0
    sgn_b = torch.ones(N, R)
    sgn_b[:, 1::2] = -1.0
    sgn_b[1::2] *= -1.0
    pa, pb = _bf16(sgn_a * POISON), _bf16(sgn_b * POISON)
    for s in range(S):
        if s == case.unused_slot:
            a[s], b[s] = pa, pb
            continue
        rank, rr = RANKS[s], round_up8(RANKS[s])
        b[s, :, :rank] = _bf16(b[s, :, :rank] / rank ** 0.5)
        a[s, rank:rr] = 0.0
        b[s, :, rank:rr] = 0.0
        a[s, rr:] = pa[rr:]
        b[s, :, rr:] = pb[:, rr:]
    width = LEAD + N + VIEW_PAD + TAIL
    wide = torch.full((T, width), SENTINEL)
    c0 = LEAD + case.off
    wide[:, c0:c0 + N] = _bf16(torch.randn(T, N, generator=g))
    return SimpleNamespace(
        case=case, x=x, a_stack=a, b_stack=b,
        scale=torch.tensor(SCALES, dtype=torch.float32),
        ranks=torch.tensor(RANKS, dtype=torch.int32),
        slot_idx=torch.tensor(_slot_pattern(case), dtype=torch.int32),
        wide=wide,
    )


def written_mask(inp: SimpleNamespace) -> torch.Tensor:
    """[T, width] bool: the elements the ops may change."""
    case = inp.case
    m = torch.zeros(inp.wide.shape, dtype=torch.bool)
    c0 = LEAD + case.off
    for t, s in enumerate(inp.slot_idx.tolist()):
        if 0 <= s < S:
            m[t, c0:c0 + case.N] = True
    return m


# ---------------------------------------------------------------------------
# fp64 reference with mutants
# ---------------------------------------------------------------------------
MUTANTS = (
    "wrong_slot",       # weights of slot + 1
    "rank_plus8",       # rank bound off by 8: reads rows past round_up(rank)
    "ignore_offset",    # delta written at out_offset 0
    "other_scale",      # scale of slot + 1
    "base_as_slot0",    # a slot -1 row treated as slot 0
)


def reference(inp: SimpleNamespace, mutate: Optional[str] = None):
    """Row-wise float64 result over the whole wide buffer. Returns
    ``(out, absmass)``, both [T, width] float64."""
    assert mutate is None or mutate in MUTANTS, mutate
    case: Case = inp.case
    x = inp.x.double()
    a, b = inp.a_stack.double(), inp.b_stack.double()
    out = inp.wide.double().clone()
    absmass = out.abs()
    off = 0 if mutate == "ignore_offset" else case.off
    c0 = LEAD + off
    for t, s in enumerate(inp.slot_idx.tolist()):
        if mutate == "base_as_slot0" and s == -1:
            s = 0
        if s < 0 or s >= S:
            continue
        w = (s + 1) % S if mutate == "wrong_slot" else s
        rr = round_up8(int(inp.ranks[w]))
        if mutate == "rank_plus8":
            rr = min(R, rr + 8)
        sc = float(inp.scale[(s + 1) % S if mutate == "other_scale" else w])
        tmp = a[w, :rr] @ x[t]                       # [rr]
        out[t, c0:c0 + case.N] += sc * (b[w, :, :rr] @ tmp)
        tmass = a[w, :rr].abs() @ x[t].abs()
        absmass[t, c0:c0 + case.N] += abs(sc) * (b[w, :, :rr].abs() @ tmass)
    return out, absmass


@functools.lru_cache(maxsize=None)
def expected(case: Case):
    """(out, absmass) of the unmutated reference; cached, do not modify."""
    return reference(build(case))


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def allowance(ref: torch.Tensor, absmass: torch.Tensor, K: int) -> torch.Tensor:
    return OUT_ULP * ref.abs() + (K + R + 2) * EPS32 * absmass + ABS_FLOOR


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, absmass: torch.Tensor,
                K: int) -> float:
    """max over elements of |got - ref| / allowance; inf if anything in
    ``got`` is not finite. <= 1 passes."""
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r = (got - ref).abs() / allowance(ref, absmass, K)
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------
# running a case through kserve_amd.ops
# ---------------------------------------------------------------------------
def device_inputs(case: Case, dev) -> SimpleNamespace:
    """Fresh bf16 tensors of the case on ``dev``; ``y`` is the strided view
    of ``wide`` the ops get."""
    inp = build(case)
    wide = inp.wide.to(torch.bfloat16).to(dev)
    y = wide[:, LEAD:LEAD + case.N + VIEW_PAD]
    assert case.T == 1 or not y.is_contiguous()
    return SimpleNamespace(
        x=inp.x.to(torch.bfloat16).to(dev),
        a_stack=inp.a_stack.to(torch.bfloat16).to(dev),
        b_stack=inp.b_stack.to(torch.bfloat16).to(dev),
        scale=inp.scale.to(dev), ranks=inp.ranks.to(dev),
        slot_idx=inp.slot_idx.to(dev), wide=wide, y=y,
    )


def run_ops(case: Case, dev, d: Optional[SimpleNamespace] = None) -> torch.Tensor:
    """shrink + expand_add through the public ops (HIP kernels on a GPU,
    torch_ref on the CPU); returns the whole wide buffer afterwards."""
    from kserve_amd import ops

    d = d or device_inputs(case, dev)
    tmp = ops.lora_shrink(d.x, d.a_stack, d.ranks, d.slot_idx)
    assert tmp.dtype == torch.float32 and tmp.shape == (case.T, R)
    got = ops.lora_expand_add(d.y, tmp, d.b_stack, d.scale, d.ranks,
                              d.slot_idx, out_offset=case.off)
    assert got is d.y
    return d.wide


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def check_case(case: Case, dev):
    """Run the case on ``dev``. Returns ``(ratio, untouched_ok)``: the worst
    error / allowance over the whole buffer, and whether every element
    outside the written region kept its bits."""
    inp = build(case)
    before = inp.wide.to(torch.bfloat16)
    after = run_ops(case, dev).cpu()
    ref, absmass = expected(case)
    keep = ~written_mask(inp)
    untouched_ok = bool((bits(after)[keep] == bits(before)[keep]).all())
    return worst_ratio(after, ref, absmass, case.K), untouched_ok
