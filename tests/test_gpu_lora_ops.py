"""The batched multi-LoRA HIP kernels (ops.lora_shrink, ops.lora_expand_add)
against the fp64 reference and derived allowance of tests/lora_cases.py."""

import pytest
import torch

from tests import lora_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_kernels_within_allowance(case):
    """Every case within the allowance; sentinel columns, -1 rows and the
    out-of-range row bit-identical afterwards."""
    ratio, untouched_ok = lc.check_case(case, DEV)
    print(f"{case.name}: err/allowance = {ratio:.3f}")
    assert untouched_ok, "sentinel columns or skipped rows changed"
    assert ratio <= 1.0


def _t33():
    return next(c for c in lc.CASES if c.T == 33 and c.K == 1088 and c.N == 256)


def test_row_independence():
    """A row run alone (T=1) is bit-equal to the same row in the mixed
    batch: the result depends on nothing but the row and its adapter."""
    case = _t33()
    batch = lc.run_ops(case, DEV).clone()
    d = lc.device_inputs(case, DEV)
    from kserve_amd import ops

    for t in range(case.T):
        y = d.y[t : t + 1]
        slot = d.slot_idx[t : t + 1].contiguous()
        tmp = ops.lora_shrink(d.x[t : t + 1], d.a_stack, d.ranks, slot)
        ops.lora_expand_add(y, tmp, d.b_stack, d.scale, d.ranks, slot,
                            out_offset=case.off)
    assert torch.equal(lc.bits(d.wide), lc.bits(batch))
    # and the rows did change: the comparison is not between two no-ops
    before = lc.build(case).wide.to(torch.bfloat16).to(DEV)
    assert not torch.equal(lc.bits(batch), lc.bits(before))


def test_repeatable():
    case = _t33()
    a = lc.run_ops(case, DEV)
    b = lc.run_ops(case, DEV)
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(lc.bits(a), lc.bits(b))


def test_binding_rejections():
    from kserve_amd import ops

    S, R, T = 2, 8, 2
    bf = dict(dtype=torch.bfloat16, device=DEV)
    ranks = torch.full((S,), 8, dtype=torch.int32, device=DEV)
    slots = torch.zeros(T, dtype=torch.int32, device=DEV)
    scale = torch.ones(S, dtype=torch.float32, device=DEV)
    x = torch.zeros(T, 64, **bf)
    a = torch.zeros(S, R, 64, **bf)
    b = torch.zeros(S, 64, R, **bf)
    y = torch.zeros(T, 128, **bf)
    tmp = ops.lora_shrink(x, a, ranks, slots)          # the valid call
    ops.lora_expand_add(y, tmp, b, scale, ranks, slots, 64)
    torch.cuda.synchronize()

    with pytest.raises(RuntimeError):                  # K % 64 != 0
        ops.lora_shrink(torch.zeros(T, 72, **bf), torch.zeros(S, R, 72, **bf),
                        ranks, slots)
    with pytest.raises(RuntimeError):                  # non-contiguous stack
        ops.lora_shrink(x, torch.zeros(S, 2 * R, 64, **bf)[:, :R], ranks, slots)
    with pytest.raises(RuntimeError):
        ops.lora_expand_add(y, tmp, torch.zeros(S, 64, 2 * R, **bf)[:, :, :R],
                            scale, ranks, slots, 0)
    with pytest.raises(RuntimeError):                  # off + N past the row
        ops.lora_expand_add(y, tmp, b, scale, ranks, slots, 72)
    with pytest.raises(RuntimeError):                  # N % 64 != 0
        ops.lora_expand_add(y, tmp, torch.zeros(S, 72, R, **bf), scale, ranks,
                            slots, 0)
    with pytest.raises(RuntimeError):                  # misaligned rows
        ops.lora_shrink(torch.zeros(T, 72, **bf)[:, 4:68], a, ranks, slots)
    with pytest.raises(RuntimeError):                  # int64 slot index
        ops.lora_shrink(x, a, ranks, slots.long())
    torch.cuda.synchronize()
