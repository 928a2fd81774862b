"""GPU: every env-selected attention kernel on the adversarial cases.

The switches are read once per process, so each setting runs in one fresh
child (tests/attention_variant_child.py), strictly one after another. The
child checks that its variant's kernel is what its cases dispatch to and
prints per-case err/allowance; the parent asserts on that line and on a zero
exit status. After a child that died from a signal or ran into its time
limit, no further child is started.
"""

import json
import os
import subprocess
import sys

import pytest

from tests import attention_variant_child as child

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120  # a healthy child takes ~10 s; this only bounds a hang

SETTINGS = [
    "ws", "h2", "mq", "u2", "v4_s4", "v4d2", "d2_off", "d2_pb_off", "occ5",
    "occ6", "fp8_cvtb_off", "split1", "split3", "split16", "prefill_v1",
    "prefill_as",
]

_stop = {"reason": None}


def test_settings_cover_every_switch():
    envs = [child.VARIANTS[s][0] for s in SETTINGS]
    assert {"KS_ATTN_WS": "1"} in envs
    assert {"KS_ATTN_H2": "1"} in envs
    assert {"KS_ATTN_MQ": "1"} in envs
    assert {"KS_ATTN_U2": "1"} in envs
    assert {"KS_ATTN_V4": "1"} in envs
    assert {"KS_ATTN_V4": "1", "KS_ATTN_V4D2": "1"} in envs
    assert {"KS_ATTN_D2": "0"} in envs
    assert {"KS_ATTN_D2": "0", "KS_ATTN_PB": "0"} in envs
    for occ in ("5", "6"):
        assert {"KS_ATTN_D2": "0", "KS_ATTN_PB": "0", "KS_ATTN_OCC": occ} in envs
    assert {"KS_FP8_CVTB": "0"} in envs
    for n in ("1", "3", "16"):
        assert {"KS_ATTN_SPLIT": n} in envs
    assert {"KS_PREFILL_V1": "1"} in envs
    assert {"KS_PREFILL_AS": "1"} in envs
    # each variant has cases that reach its kernel, windowed and not
    for s in SETTINGS:
        cases = child.selected_cases(s)
        assert any(c.window > 0 for c in cases), s
        assert any(c.window == 0 for c in cases), s
    assert all(c.S == 4 for c in child.selected_cases("v4_s4"))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS)
def test_variant(setting):
    if _stop["reason"]:
        pytest.fail(f"not started: {_stop['reason']}")
    try:
        proc = subprocess.run(
            [sys.executable, "-m", "tests.attention_variant_child",
             "--variant", setting],
            env=child.variant_env(setting), cwd=REPO, timeout=CHILD_TIMEOUT_S,
            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
        )
    except subprocess.TimeoutExpired:
        _stop["reason"] = f"child {setting} ran into its time limit"
        pytest.fail(_stop["reason"])
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _stop["reason"] = f"child {setting} died with status {proc.returncode}"
    assert proc.returncode == 0, (
        f"child {setting} exited {proc.returncode}\n{proc.stderr[-2000:]}")
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["variant"] == setting
    assert rec["kernel"] == child.VARIANTS[setting][2]
    assert set(rec["ratios"]) == {c.name for c in child.selected_cases(setting)}
    print(f"{setting}: worst err/allowance = {max(rec['ratios'].values()):.3f}")
    bad = {k: round(v, 2) for k, v in rec["ratios"].items() if not v <= 1.0}
    assert not bad, f"{setting}: err/allowance above 1: {bad}"
