"""Child process of tests/test_gpu_attention_pipelined.py.

KS_ATTN_V4PIPE is read once per process, so each setting needs a fresh one:

    python -m tests.attention_pipelined_child --pipe 0|1

``--pipe 1`` runs every case of tests/attention_pipelined_cases.py on the
pipelined loop, whatever the default is; ``--pipe 0`` runs the first two on
the loop it replaces. Prints one JSON line
``{"pipe": ..., "ratios": {case: err/allowance}}``; exit status 0 means it
ran, the parent asserts on the ratios.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

from tests import attention_cases as ac
from tests import attention_pipelined_cases as pc
from tests.attention_variant_child import _ENV_KEYS

SWITCH = "KS_ATTN_V4PIPE"


def child_env(pipe: str) -> dict:
    """The parent's environment without any kernel switch, plus this one."""
    env = {k: v for k, v in os.environ.items()
           if k not in _ENV_KEYS and k != SWITCH}
    env[SWITCH] = pipe
    return env


def selected_cases(pipe: str):
    return list(pc.CASES) if pipe == "1" else list(pc.FIRST_CASES)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipe", required=True, choices=("0", "1"))
    args = ap.parse_args(argv)
    assert os.environ.get(SWITCH) == args.pipe
    live = {k: os.environ[k] for k in _ENV_KEYS if k in os.environ}
    assert not live, f"other kernel switches are set: {live}"
    cases = selected_cases(args.pipe)
    for c in cases:
        assert ac.expected_decode_kernel(c, live) == "v4", c.name

    import torch

    assert torch.cuda.is_available(), "child needs a GPU"
    from kserve_amd import ops

    assert ops.has_native()
    dev = torch.device("cuda:0")
    ratios = {c.name: pc.ratio(c, dev) for c in cases}
    for c in pc.EDGE_CASES:
        if c in cases:
            ratios[c.name + "/narrow"] = pc.ratio(c, dev, narrow_table=True)
    torch.cuda.synchronize()
    print(json.dumps({"pipe": args.pipe, "ratios": ratios}))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
