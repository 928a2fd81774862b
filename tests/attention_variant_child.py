"""Child process of tests/test_gpu_attention_variants.py.

The env-selected attention kernels (KS_ATTN_*, KS_FP8_CVTB, KS_PREFILL_*) are
read once per process in static initialisers, so each setting needs a fresh
process: the parent sets the environment and runs

    python -m tests.attention_variant_child --variant NAME

This runs every case of tests/attention_cases.py the variant can take, checks
from the mirrored dispatch conditions that the variant's kernel (and not the
default) is what those cases launch, and prints one JSON line
``{"variant": ..., "kernel": ..., "ratios": {case: err/allowance}}``.
Exit status 0 means it ran; the parent asserts on the ratios.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

from tests import attention_cases as ac

_DEC = ac.DECODE_CASES
_DEC8 = ac.DECODE_FP8_CASES
_FLASH128 = [c for c in ac.FLASH_CASES if c.D == 128]

# name -> (env, cases offered, kernel every selected bf16 decode case must
# dispatch to or None, eps_P or None for the case's own)
VARIANTS = {
    "default": ({}, ac.ALL_CASES, None, None),
    "ws": ({"KS_ATTN_WS": "1"}, _DEC, "ws", None),
    "h2": ({"KS_ATTN_H2": "1"}, _DEC, "h2", None),
    # QK on MFMA: eps_P of the MFMA kernels
    "mq": ({"KS_ATTN_MQ": "1"}, _DEC, "mq", ac.EPS_MFMA),
    "u2": ({"KS_ATTN_U2": "1"}, _DEC, "u2", None),
    "v4_s4": ({"KS_ATTN_V4": "1"}, [c for c in _DEC if c.S == 4], "v4", None),
    "v4d2": ({"KS_ATTN_V4": "1", "KS_ATTN_V4D2": "1"}, _DEC, "v4d2", None),
    "d2_off": ({"KS_ATTN_D2": "0"}, _DEC, "pb", None),
    "d2_pb_off": ({"KS_ATTN_D2": "0", "KS_ATTN_PB": "0"}, _DEC,
                  "generic_d128_hpw1", None),
    "occ5": ({"KS_ATTN_D2": "0", "KS_ATTN_PB": "0", "KS_ATTN_OCC": "5"},
             _DEC, "occ5", None),
    "occ6": ({"KS_ATTN_D2": "0", "KS_ATTN_PB": "0", "KS_ATTN_OCC": "6"},
             _DEC, "occ6", None),
    "fp8_cvtb_off": ({"KS_FP8_CVTB": "0"}, _DEC8, "fp8_fma", None),
    "split1": ({"KS_ATTN_SPLIT": "1"}, _DEC + _DEC8, None, None),
    "split3": ({"KS_ATTN_SPLIT": "3"}, _DEC + _DEC8, None, None),
    "split16": ({"KS_ATTN_SPLIT": "16"}, _DEC + _DEC8, None, None),
    "prefill_v1": ({"KS_PREFILL_V1": "1"}, _FLASH128, None, None),
    "prefill_as": ({"KS_PREFILL_AS": "1"}, _FLASH128, None, None),
}

_ENV_KEYS = ("KS_ATTN_WS", "KS_ATTN_H2", "KS_ATTN_MQ", "KS_ATTN_U2",
             "KS_ATTN_V4", "KS_ATTN_V4D2", "KS_ATTN_D2", "KS_ATTN_PB",
             "KS_ATTN_OCC", "KS_ATTN_SPLIT", "KS_FP8_CVTB", "KS_PREFILL_V1",
             "KS_PREFILL_AS")


def variant_env(name: str) -> dict:
    """Environment for the child: the parent's, with every kernel switch
    removed and this variant's set."""
    env = {k: v for k, v in os.environ.items() if k not in _ENV_KEYS}
    env.update(VARIANTS[name][0])
    return env


def selected_cases(name: str):
    env, offered, kernel, _ = VARIANTS[name]
    if kernel is None:
        return list(offered)
    return [c for c in offered if ac.expected_decode_kernel(c, env) == kernel]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=sorted(VARIANTS))
    args = ap.parse_args(argv)
    env, _, kernel, eps = VARIANTS[args.variant]

    # the switches this process actually runs under must be this variant's
    live = {k: os.environ[k] for k in _ENV_KEYS if k in os.environ}
    assert live == env, f"environment {live} is not variant {env}"
    cases = selected_cases(args.variant)
    assert cases, f"variant {args.variant}: no case reaches its kernel"
    for c in cases:
        if kernel is not None:
            got = ac.expected_decode_kernel(c, live)
            assert got == kernel, f"{c.name} dispatches to {got}, not {kernel}"

    import torch

    assert torch.cuda.is_available(), "variant child needs a GPU"
    from kserve_amd import ops

    assert ops.has_native()
    dev = torch.device("cuda:0")
    ratios = {c.name: ac.gpu_ratio(c, dev, eps) for c in cases}
    torch.cuda.synchronize()
    print(json.dumps({"variant": args.variant, "kernel": kernel,
                      "ratios": ratios}))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
