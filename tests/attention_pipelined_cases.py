"""Decode cases aimed at the pipelined wide-V page loop
(paged_attention_v4p_kernel, KS_ATTN_V4PIPE). Helper module: imported by
test_attention_pipelined_cases.py (CPU), test_gpu_attention_pipelined.py and
attention_pipelined_child.py; not collected.

All cases have S = 129 and Hkv = 4, so the wide-V slot is dispatched by
batch size and S * Hkv = 516 > 512 leaves the context unsplit: one wave
walks all pages of a sequence. What the cases plant:

* page counts 1, 2 (odd tail of the two-page unroll), 3 and 4 next to the
  usual 15/16/17 token edges;
* 63, 64, 65, 66, 128 and 129 pages, where the 64-entry block-id register
  is refilled, and a window that makes the page range start at page 62/63
  and still span more than 64 pages;
* GQA groups 1 and 3, where waves >= group leave before the loop;
* a longest sequence in the last table row, even and odd page count, for a
  run with a table narrowed to exactly that many columns: the prefetch of
  "the next page" then points one entry past the table's allocation.
"""

from __future__ import annotations

from typing import List, Tuple

import torch

from tests import attention_cases as ac

S = 129
HKV = 4
PLANTED = (1, 15, 16, 17, 31, 32, 33, 48)
# 63, 64, 65, 65 (full), 66, 128 and 129 pages
REFILL_CTX = (1008, 1024, 1025, 1040, 1041, 2033, 2049)
REFILL_WINDOW = 1030


def _ctx(seed: int, hi: int, planted: Tuple[int, ...],
         last: int = 0) -> Tuple[int, ...]:
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(1, hi + 1, (S,), generator=g).tolist()
    c[:len(planted)] = planted
    if last:
        c[-1] = last
    return tuple(c)


def _cases() -> List[ac.Case]:
    short = _ctx(11, 40, PLANTED)
    out = [
        ac.Case("pipe_unsplit_g4", "decode", HKV, 4, 128, ctx=short, seed=900),
        ac.Case("pipe_unsplit_g4_w24", "decode", HKV, 4, 128, ctx=short,
                window=24, seed=901),
    ]
    # the rest short so the cache stays small
    refill = _ctx(12, 20, REFILL_CTX)
    out.append(ac.Case("pipe_refill", "decode", HKV, 4, 128, ctx=refill,
                       seed=902))
    out.append(ac.Case(f"pipe_refill_w{REFILL_WINDOW}", "decode", HKV, 4, 128,
                       ctx=refill, window=REFILL_WINDOW, seed=903))
    for i, g in enumerate((1, 3)):
        out.append(ac.Case(f"pipe_unsplit_g{g}", "decode", HKV, g, 128,
                           ctx=short, seed=904 + i))
    # longest sequence last: 6 pages (even) and 5 pages (odd)
    out.append(ac.Case("pipe_edge_even", "decode", HKV, 4, 128,
                       ctx=_ctx(13, 40, PLANTED, last=81), seed=906))
    out.append(ac.Case("pipe_edge_odd", "decode", HKV, 4, 128,
                       ctx=_ctx(14, 40, PLANTED, last=80), seed=907))
    return out


CASES = _cases()
CASES_BY_NAME = {c.name: c for c in CASES}
EDGE_CASES = [c for c in CASES if c.name.startswith("pipe_edge")]
FIRST_CASES = CASES[:2]   # what the KS_ATTN_V4PIPE=0 child runs


def run_decode(case: ac.Case, dev, narrow_table: bool = False) -> torch.Tensor:
    """ac.run_gpu for a decode case; with ``narrow_table`` the block table
    is cut to the columns the longest sequence needs (its own allocation, no
    slack), the way the engine passes it."""
    from kserve_amd import ops

    inp = ac.build(case)
    q = ac._strided_rows(inp.q, dev, 32, 32)
    kc = ac._cache_to(inp.k_cache, case, dev)
    vc = ac._cache_to(inp.v_cache, case, dev)
    bt = inp.block_tables
    if narrow_table:
        bt = bt[:, :inp.needed_blocks].contiguous()
    out = torch.full(inp.q.shape, ac.OUT_SENTINEL, dtype=torch.bfloat16,
                     device=dev)
    ops.paged_attention_decode(q, kc, vc, bt.to(dev), inp.context_lens.to(dev),
                               inp.scale, out=out, window=case.window)
    assert not bool((out == ac.OUT_SENTINEL).any()), \
        f"{case.name}: output rows left unwritten"
    return out


def ratio(case: ac.Case, dev, narrow_table: bool = False) -> float:
    ref, absmass = ac.expected(case)
    return ac.worst_ratio(run_decode(case, dev, narrow_table), ref, absmass,
                          case.eps_p)
