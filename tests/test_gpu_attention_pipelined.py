"""GPU: the pipelined wide-V decode loop (KS_ATTN_V4PIPE) on the cases of
tests/attention_pipelined_cases.py, against the fp64 reference and the
allowance of tests/attention_cases.py (eps_P = 2^-12, pass at ratio <= 1).

In-process tests run whichever loop is the default. Two children, one per
setting of the switch and strictly one after the other, pin each loop: the
pipelined one on every case, the loop it replaces on the first two. After a
child that died from a signal or ran into its time limit the other is not
started.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_cases as ac
from tests import attention_pipelined_cases as pc
from tests import attention_pipelined_child as child

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120  # a healthy child takes ~15 s; this only bounds a hang

_stop = {"reason": None}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    return torch.device("cuda:0")


def _assert_ratio(name, ratio):
    print(f"{name}: worst err/allowance = {ratio:.3f}")
    assert ratio <= 1.0, (
        f"{name}: worst |got-ref| is {ratio:.2f}x the allowance (eps_P = 2^-12)")


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_decode(dev, name):
    case = pc.CASES_BY_NAME[name]
    assert ac.expected_decode_kernel(case, {}) == "v4"
    inp = ac.build(case)
    assert ac.decode_n_splits(case.S, case.H, case.Hkv,
                              inp.block_tables.shape[1]) == 1
    _assert_ratio(name, pc.ratio(case, dev))


@pytest.mark.parametrize("name", [c.name for c in pc.EDGE_CASES])
def test_table_without_slack(dev, name):
    """The longest sequence is the last row and uses every column: entry
    blk_hi of that row is the first int past the table."""
    case = pc.CASES_BY_NAME[name]
    inp = ac.build(case)
    assert max(case.ctx) == case.ctx[-1]
    assert -(-case.ctx[-1] // ac.PAGE) == inp.needed_blocks
    _assert_ratio(name, pc.ratio(case, dev, narrow_table=True))


def test_non_contiguous_tables_raise(dev):
    from kserve_amd import ops

    case = pc.CASES_BY_NAME["pipe_edge_odd"]
    inp = ac.build(case)
    q = inp.q.to(torch.bfloat16).to(dev)
    kc = inp.k_cache.to(torch.bfloat16).to(dev)
    vc = inp.v_cache.to(torch.bfloat16).to(dev)
    bt = inp.block_tables.to(dev)
    cl = inp.context_lens.to(dev)
    view = bt[:, :inp.needed_blocks]
    assert not view.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.paged_attention_decode(q, kc, vc, view, cl, inp.scale)
    cl2 = torch.stack([cl, cl], dim=1)[:, 0]
    assert not cl2.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.paged_attention_decode(q, kc, vc, bt, cl2, inp.scale)


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_switch(pipe):
    if _stop["reason"]:
        pytest.fail(f"not started: {_stop['reason']}")
    try:
        proc = subprocess.run(
            [sys.executable, "-m", "tests.attention_pipelined_child",
             "--pipe", pipe],
            env=child.child_env(pipe), cwd=REPO, timeout=CHILD_TIMEOUT_S,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
        )
    except subprocess.TimeoutExpired:
        _stop["reason"] = f"child pipe={pipe} ran into its time limit"
        pytest.fail(_stop["reason"])
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _stop["reason"] = f"child pipe={pipe} died with status {proc.returncode}"
    assert proc.returncode == 0, (
        f"child pipe={pipe} exited {proc.returncode}\n{proc.stderr[-2000:]}")
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["pipe"] == pipe
    want = {c.name for c in child.selected_cases(pipe)}
    if pipe == "1":
        want |= {c.name + "/narrow" for c in pc.EDGE_CASES}
    assert set(rec["ratios"]) == want
    print(f"pipe={pipe}: worst err/allowance = {max(rec['ratios'].values()):.3f}")
    bad = {k: round(v, 2) for k, v in rec["ratios"].items() if not v <= 1.0}
    assert not bad, f"pipe={pipe}: err/allowance above 1: {bad}"
