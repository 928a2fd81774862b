"""CPU checks of the attention test harness itself (tests/attention_cases.py).

The GPU tests are only worth something if the cases can tell a right kernel
from a nearly right one. So, without a GPU:

* the bf16-rounded fp64 reference stays inside the comparator's allowance;
* every mutant of the reference (window off by one, block table ignored,
  first invalid slot read, ...) misses the allowance by at least 10x on at
  least one element of every case it changes anything on;
* torch_ref, which the CPU engine runs on and which had the same
  identity-table blind spot, agrees with the new reference on every case.
"""

import pytest
import torch

from kserve_amd.ops import torch_ref
from tests import attention_cases as ac

CASE_IDS = [c.name for c in ac.ALL_CASES]

# The kill condition is checked at the loosest eps_P any kernel gets.
KILL_EPS = ac.EPS_MFMA
KILL_FACTOR = 10.0

# fp32 noise of torch_ref against fp64: a D-term dot, a softmax over n keys
# and an n-term PV sum accumulate at most ~(D + 2n) roundings of 2^-24 each,
# relative to the summed mass; D + 2n <= 128 + 2*201 < 2^10 here. The
# comparator's own 2^-8 |ref| output-ulp term is not granted.
TORCH_REF_EPS = 2.0 ** -14


def _kinds(m):
    """Which case kinds a mutant is defined for."""
    return {
        "drop_last": ("decode", "context", "flash"),
        "include_first_invalid": ("decode", "context", "flash"),
        "window_plus": ("decode", "context", "flash"),
        "window_minus": ("decode", "context", "flash"),
        "ignore_table": ("decode", "context"),
        "row_stride": ("decode", "context"),
        "head_mod": ("decode", "context", "flash"),
        "drop_page_first": ("decode", "context"),
        "drop_after_split": ("decode",),
        "causal_strict": ("flash",),
        "ctx_offset_minus": ("context",),
        "ctx_offset_plus": ("context",),
        "prev_seq_leak": ("flash",),
        "noncausal_as_causal": ("flash",),
    }[m]


def test_case_lists_cover_the_issue():
    names = set(CASE_IDS)
    assert len(names) == len(CASE_IDS)
    dec = ac.DECODE_CASES
    assert {c.group for c in dec} == {1, 3, 4, 5, 8}
    assert {c.Hkv for c in dec} == {1, 2}
    assert {c.group for c in dec if c.D == 64} == {1, 8}
    assert any(c.S > 128 and c.window == 0 for c in dec)
    assert any(c.S > 128 and c.window > 0 for c in dec)
    assert any(c.share_prefix for c in dec)
    assert {c.group for c in ac.DECODE_FP8_CASES} == {1, 2, 4}
    assert {(c.H, c.Hkv) for c in ac.FLASH_CASES} == {(4, 1), (3, 3), (8, 2)}
    assert {c.D for c in ac.FLASH_CASES} == {64, 128}
    assert {c.window for c in ac.FLASH_CASES} == {0, 1, 16, 63, 64, 65}
    assert any(not c.causal for c in ac.FLASH_CASES)
    assert {c.window for c in ac.CONTEXT_CASES} == {0, 16, 48, 65}
    assert {c.fp8 for c in ac.CONTEXT_CASES} == {False, True}


@pytest.mark.parametrize("name", CASE_IDS)
def test_tables_are_permuted_wide_and_poisoned(name):
    case = ac.CASES_BY_NAME[name]
    if case.kind == "flash":
        return
    inp = ac.build(case)
    bt = inp.block_tables
    S, width = bt.shape
    assert width >= inp.needed_blocks + ac.TABLE_SLACK
    assert int(bt.min()) >= 0 and int(bt.max()) < inp.num_blocks
    ident = torch.arange(1, S * width + 1).reshape(S, width)
    nb = [-(-c // ac.PAGE) for c in case.ctx]
    used = torch.cat([bt[s, :nb[s]] for s in range(S)])
    assert not torch.equal(used.long(),
                           torch.cat([ident[s, :nb[s]] for s in range(S)]))
    mag = ac.POISON_FP8 if case.fp8 else ac.POISON_BF16
    # block 0 and every page behind an unused entry are poison, finite
    for s in range(S):
        for p in range(nb[s], width):
            pg = int(bt[s, p])
            assert float(inp.k_cache[pg, :, 1:].abs().min()) >= 0.99 * mag
            assert float(inp.v_cache[pg, :, 1:].abs().min()) >= 0.99 * mag
        tail = case.ctx[s] % ac.PAGE
        if tail and tail + 1 < ac.PAGE:
            pg = int(bt[s, nb[s] - 1])
            assert float(inp.v_cache[pg, :, tail + 1:].abs().min()) >= 0.99 * mag
    assert float(inp.k_cache[0, :, 1:].abs().min()) >= 0.99 * mag
    assert bool(torch.isfinite(inp.k_cache).all())
    assert bool(torch.isfinite(inp.v_cache).all())
    if case.share_prefix:
        firsts = bt[:, 0].tolist()
        assert len(set(firsts)) < len(firsts)


@pytest.mark.parametrize("name", CASE_IDS)
def test_rounded_reference_passes(name):
    case = ac.CASES_BY_NAME[name]
    ref, absmass = ac.expected(case)
    assert bool(torch.isfinite(ref).all())
    got = ref.to(torch.bfloat16)
    # eps_P = 0: rounding the output alone must fit the output-ulp term
    assert ac.worst_ratio(got, ref, absmass, 0.0) <= 1.0
    assert ac.worst_ratio(got, ref, absmass, case.eps_p) <= 1.0
    # and a NaN is never accepted
    bad = got.clone()
    bad.view(-1)[0] = float("nan")
    assert ac.worst_ratio(bad, ref, absmass, case.eps_p) == float("inf")


@pytest.mark.parametrize("name", CASE_IDS)
def test_every_applicable_mutant_is_killed(name):
    """A mutant applies to a case when it changes, for at least one query
    row, which stored tokens are attended or through which kv head; then it
    must miss the allowance by >= 10x somewhere. (A mutant that changes
    nothing on a case, such as W+1 without a window or `h % Hkv` at
    group 1, is the reference itself.)"""
    case = ac.CASES_BY_NAME[name]
    inp = ac.build(case)
    ref, absmass, sig = ac.reference(inp)
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


def test_every_mutant_applies_where_it_should():
    """The structural applicability rule must not quietly empty the list:
    each mutant changes something on the cases it was written for."""
    def applies(m, case):
        inp = ac.build(case)
        return ac.reference(inp, mutate=m)[2] != ac.reference(inp)[2]

    paged = (ac.DECODE_CASES + ac.DECODE_FP8_CASES + ac.CONTEXT_CASES)
    want = {
        "drop_last": ac.ALL_CASES,
        "include_first_invalid": ac.ALL_CASES,
        "window_plus": [c for c in ac.ALL_CASES if c.window > 0],
        "window_minus": [c for c in ac.ALL_CASES if c.window > 0],
        "ignore_table": paged,
        "row_stride": paged,
        "head_mod": [c for c in ac.ALL_CASES if c.Hkv > 1 and c.group > 1],
        "drop_page_first": paged,
        "drop_after_split": ac.DECODE_CASES + ac.DECODE_FP8_CASES,
        "causal_strict": [c for c in ac.FLASH_CASES if c.causal],
        "ctx_offset_minus": ac.CONTEXT_CASES,
        "ctx_offset_plus": ac.CONTEXT_CASES,
        "prev_seq_leak": [c for c in ac.FLASH_CASES if c.S > 1],
        "noncausal_as_causal": [c for c in ac.FLASH_CASES
                                if not c.causal and max(c.q_lens) > 1],
    }
    assert set(want) == set(ac.MUTANTS)
    for m, cases in want.items():
        assert cases, m
        missing = [c.name for c in cases if not applies(m, c)]
        assert not missing, f"{m} changes nothing on {missing}"


def _torch_ref_out(case):
    inp = ac.build(case)
    if case.kind == "decode":
        return torch_ref.paged_attention_decode(
            inp.q, inp.k_cache, inp.v_cache, inp.block_tables,
            inp.context_lens, inp.scale, window=case.window)
    if case.kind == "context":
        return torch_ref.context_attention_varlen(
            inp.q, inp.k_cache, inp.v_cache, inp.block_tables,
            inp.cu_seqlens_q, inp.context_lens, inp.scale, window=case.window)
    return torch_ref.flash_prefill_varlen(
        inp.q, inp.k[:inp.T], inp.v[:inp.T], inp.cu_seqlens, inp.scale,
        causal=case.causal, window=case.window)


@pytest.mark.parametrize("name", CASE_IDS)
def test_torch_ref_agrees(name):
    case = ac.CASES_BY_NAME[name]
    ref, absmass = ac.expected(case)
    got = _torch_ref_out(case)
    assert got.dtype == torch.float32
    err = (got.double() - ref).abs()
    allow = TORCH_REF_EPS * absmass + ac.ABS_FLOOR
    worst = float((err / allow).max())
    assert worst <= 1.0, f"{name}: torch_ref off by {worst:.2f}x fp32 noise"


def test_decode_dispatch_mirror():
    """expected_decode_kernel / decode_n_splits follow the documented
    dispatch: default small batch -> packed-dot kernel, S > 128 -> wide-V,
    group 5..8 and D=64 -> generic."""
    by = ac.CASES_BY_NAME
    assert ac.expected_decode_kernel(by["dec_kv2g4d128"], {}) == "d2"
    assert ac.expected_decode_kernel(by["dec_s129_kv1g4d128"], {}) == "v4"
    assert ac.expected_decode_kernel(by["dec_kv2g8d128"], {}) == "generic_d128_hpw2"
    assert ac.expected_decode_kernel(by["dec_kv1g1d64"], {}) == "generic_d64_hpw1"
    assert ac.expected_decode_kernel(
        by["dec_kv2g4d128"], {"KS_ATTN_D2": "0", "KS_ATTN_PB": "0"}
    ) == "generic_d128_hpw1"
    assert ac.decode_n_splits(8, 8, 2, 16) == 8
    assert ac.decode_n_splits(8, 16, 2, 16) == 16
    assert ac.decode_n_splits(129, 4, 1, 6) == 8
    assert ac.decode_n_splits(600, 8, 2, 16) == 1
    assert ac.split_first_tokens(200, 0, 8) == [32, 64, 96, 128, 160, 192]
    assert ac.split_first_tokens(200, 48, 16) == [160, 176, 192]
