"""The logit-processor kernels on the GPU: logit_process against the fp64
reference of tests/logit_process_cases.py, token_count_add against bincount,
and the min-p form of the fused sampler."""

import numpy as np
import pytest
import torch

from tests import logit_process_cases as lpc

pytestmark = pytest.mark.gpu

# V = 1, odd V (rows not 16-byte aligned: scalar path), one partial chunk,
# exactly one chunk, one chunk + 3 (odd), many chunks (odd)
SHAPES = [(1, 1), (1, 7), (3, 257), (5, 2048), (2, 4099), (4, 32003)]

_CASES = {}


def _case(S, V):
    if (S, V) not in _CASES:
        case = lpc.build_case(S, V)
        _CASES[(S, V)] = (case, lpc.reference(case))
    return _CASES[(S, V)]


@pytest.mark.parametrize("S,V", SHAPES)
def test_logit_process_out_of_place(S, V):
    from kserve_amd import ops

    case, ref = _case(S, V)
    x = case["logits"].cuda()
    out = ops.logit_process(x, *lpc.op_args(case, "cuda"))
    assert out.data_ptr() != x.data_ptr()
    assert torch.equal(
        x.cpu().view(torch.int16), case["logits"].view(torch.int16)
    ), "the input changed"
    assert lpc.violations(out, case, ref) == []


@pytest.mark.parametrize("S,V", SHAPES)
def test_logit_process_in_place(S, V):
    from kserve_amd import ops

    case, ref = _case(S, V)
    x = case["logits"].cuda()
    res = ops.logit_process(x, *lpc.op_args(case, "cuda"), out=x)
    assert res.data_ptr() == x.data_ptr()
    assert lpc.violations(x, case, ref) == []


def test_token_count_add_matches_bincount():
    from kserve_amd import ops

    slots, V, n = 5, 300, 64
    g = torch.Generator().manual_seed(7)
    slot = torch.randint(-1, slots + 1, (n,), generator=g, dtype=torch.int32)
    tok = torch.randint(-2, V + 2, (n,), generator=g, dtype=torch.int64)
    # duplicates: the same (slot, token) pair nine times in one call
    slot[:9] = 2
    tok[:9] = 123
    slot[9:12] = -1
    tok[12:14] = V
    base = torch.randint(0, 4, (slots, V), generator=g, dtype=torch.int32)
    counts = base.cuda()
    ops.token_count_add(counts, slot.cuda(), tok.cuda())
    want = base.numpy().copy()
    for sl in range(slots):
        keep = (slot.numpy() == sl) & (tok.numpy() >= 0) & (tok.numpy() < V)
        want[sl] += np.bincount(tok.numpy()[keep], minlength=V).astype(np.int32)
    assert want[2, 123] >= base[2, 123] + 9
    assert np.array_equal(counts.cpu().numpy(), want)


def _minp_logits(rows, V=1000):
    g = torch.Generator().manual_seed(3)
    row = -torch.rand(V, generator=g) * 5.0  # everything else <= 0
    top = {17: 10.0, 400: 9.75, 999: 9.5, 3: 9.0, 512: 8.0}
    for t, v in top.items():
        row[t] = v
    return row.to(torch.bfloat16).repeat(rows, 1).contiguous().cuda(), top


def _sample_minp(logits, temp, min_p):
    from kserve_amd import ops

    S = logits.shape[0]
    dev = logits.device
    out = torch.empty(S, dtype=torch.int64, device=dev)
    ops.topk_topp_minp_sample_into(
        out, logits,
        torch.full((S,), temp, dtype=torch.float32, device=dev),
        torch.ones(S, dtype=torch.float32, device=dev),
        torch.zeros(S, dtype=torch.int32, device=dev),
        torch.full((S,), min_p, dtype=torch.float32, device=dev),
        torch.arange(1, S + 1, dtype=torch.int64, device=dev) * 7919,
    )
    return out.cpu().tolist()


@pytest.mark.parametrize(
    "temp,survivors", [(1.0, {17, 400, 999}), (2.0, {17, 400, 999, 3})]
)
def test_min_p_keeps_exactly_the_survivors(temp, survivors):
    """min_p = 0.5 cuts ln 2 = 0.693 below the maximum in units of T: at
    T = 1 the values 10, 9.75, 9.5 survive (9 is 1.0 away), at T = 2 the
    distances halve and 9 (0.5) survives too, 8 (1.0) does not. 200 rows
    with the same logits and different seeds: every draw is a survivor and
    every survivor is drawn (each has probability > 0.18: the least likely
    is 9 at T = 2, e^-0.5 / (1 + e^-0.125 + e^-0.25 + e^-0.5) = 0.186), so
    missing one has probability < 4 * 0.82^200 < 1e-16."""
    logits, _ = _minp_logits(200)
    drawn = _sample_minp(logits, temp, 0.5)
    assert set(drawn) <= survivors
    assert set(drawn) == survivors


def test_min_p_zero_equals_the_plain_sampler():
    from kserve_amd import ops

    logits, _ = _minp_logits(200)
    S = logits.shape[0]
    dev = logits.device
    temps = torch.full((S,), 0.9, dtype=torch.float32, device=dev)
    top_p = torch.full((S,), 0.95, dtype=torch.float32, device=dev)
    top_k = torch.full((S,), 40, dtype=torch.int32, device=dev)
    seeds = torch.arange(1, S + 1, dtype=torch.int64, device=dev) * 104729
    plain = torch.empty(S, dtype=torch.int64, device=dev)
    ops.topk_topp_sample_into(plain, logits, temps, top_p, top_k, seeds)
    minp = torch.empty(S, dtype=torch.int64, device=dev)
    ops.topk_topp_minp_sample_into(
        minp, logits, temps, top_p, top_k,
        torch.zeros(S, dtype=torch.float32, device=dev), seeds,
    )
    assert torch.equal(plain, minp)
    assert len(set(plain.tolist())) > 1  # the seeds do differ
