"""Child process of test_gpu_lora_engine.py: the mixed-adapter batch of that
test on an engine whose decode keeps the per-segment GEMM loop
(KS_LORA_SEGMENTS=1 is read per process, hence the process). Prints one JSON
line with the tokens of each request. Not collected.

usage: python -m tests.lora_engine_child <dir of adapter A> <dir of adapter B>
"""

import json
import os
import sys


def main():
    assert os.environ.get("KS_LORA_SEGMENTS") == "1"
    from kserve_amd.engine.engine import LLMEngine
    from tests.test_gpu_engine import _cfg
    from tests.test_gpu_lora_engine import run_mixed

    engine = LLMEngine(_cfg(enforce_eager=False))
    engine.register_lora("A", sys.argv[1])
    engine.register_lora("B", sys.argv[2])
    toks = run_mixed(engine, [None, "A", "B", "A"])
    # the switch keeps LoRA decode out of the graphs
    assert not engine.runner._lora_graphs
    print("TOKENS " + json.dumps(toks), flush=True)


if __name__ == "__main__":
    main()
