"""CPU checks of the cases in tests/attention_pipelined_cases.py: the fp64
reference is finite on each, and every applicable mutant of the reference
misses the allowance by >= 10x, the bar of
test_attention_cases.py::test_every_applicable_mutant_is_killed.
"""

import pytest
import torch

from tests import attention_cases as ac
from tests import attention_pipelined_cases as pc
from tests.test_attention_cases import KILL_EPS, KILL_FACTOR, _kinds

CASE_IDS = [c.name for c in pc.CASES]


def test_cases_are_what_they_claim():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for c in pc.CASES:
        assert c.S == 129 and c.Hkv == 4 and c.D == 128 and c.kind == "decode"
        assert ac.expected_decode_kernel(c, {}) == "v4"
        width = -(-max(c.ctx) // ac.PAGE) + ac.TABLE_SLACK
        assert ac.decode_n_splits(c.S, c.H, c.Hkv, width) == 1
    first = pc.CASES_BY_NAME["pipe_unsplit_g4"]
    assert first.ctx[:8] == (1, 15, 16, 17, 31, 32, 33, 48)
    assert pc.CASES_BY_NAME["pipe_unsplit_g4_w24"].ctx == first.ctx
    refill = pc.CASES_BY_NAME["pipe_refill"]
    assert [-(-c // ac.PAGE) for c in refill.ctx[:7]] == [63, 64, 65, 65, 66,
                                                          128, 129]
    win = pc.CASES_BY_NAME[f"pipe_refill_w{pc.REFILL_WINDOW}"]
    # first_blk > 0 and still more than 64 pages in range
    for c in (2033, 2049):
        first_blk = (c - win.window) // ac.PAGE
        assert first_blk > 0 and -(-c // ac.PAGE) - first_blk > 64
    assert {pc.CASES_BY_NAME[f"pipe_unsplit_g{g}"].group for g in (1, 3)} == {1, 3}
    assert {-(-c.ctx[-1] // ac.PAGE) % 2 for c in pc.EDGE_CASES} == {0, 1}
    for c in pc.EDGE_CASES:
        assert c.ctx[-1] == max(c.ctx) and c.ctx.count(c.ctx[-1]) == 1


@pytest.mark.parametrize("name", CASE_IDS)
def test_reference_is_finite(name):
    ref, absmass = ac.expected(pc.CASES_BY_NAME[name])
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(absmass).all())


@pytest.mark.parametrize("name", CASE_IDS)
def test_every_applicable_mutant_is_killed(name):
    case = pc.CASES_BY_NAME[name]
    inp = ac.build(case)
    ref, absmass = ac.expected(case)
    sig = ac.reference(inp)[2]
    survivors = []
    for m in ac.MUTANTS:
        if case.kind not in _kinds(m):
            continue
        out, _, msig = ac.reference(inp, mutate=m)
        if msig == sig:
            continue
        r = ac.worst_ratio(out, ref, absmass, KILL_EPS)
        if r < KILL_FACTOR:
            survivors.append((m, r))
    assert not survivors, f"{name}: mutants not killed 10x: {survivors}"
