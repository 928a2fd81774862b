"""GPU engine: multi-LoRA decode through the batched adapter kernels, replayed
from hipGraphs. A mixed batch (base, A, B, A) on the graph engine must equal
the eager engine token for token; the kernels add no batch-shape dependence
(tests/test_gpu_lora_ops.py::test_row_independence), so this is the same
claim test_gpu_engine.py::test_graph_matches_eager makes for the base GEMMs."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 180  # a healthy child takes ~20 s; this only bounds a hang
PROMPTS = [[1, 2, 3, 4, 5], [100, 200, 300], [7, 8, 9, 10], [11, 12, 13, 14, 15, 16]]
MAX_TOKENS = 8


def run_mixed(engine, lora_names):
    """Submit PROMPTS together, request i under adapter lora_names[i] (None =
    base model); greedy, MAX_TOKENS each. Returns the token lists in order."""
    from kserve_amd.engine.sampling_params import SamplingParams

    rids = [
        engine.add_request(
            p, SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS,
                              lora_name=name)
        )
        for p, name in zip(PROMPTS, lora_names)
    ]
    outs = {}
    while engine.has_unfinished():
        for out in engine.step():
            if out.finished:
                outs[out.request_id] = list(out.output_token_ids)
    return [outs[r] for r in rids]


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    from tests.test_gpu_engine import _cfg
    from tests.test_lora import make_adapter_dir

    cfg = _cfg().model
    return {
        name: make_adapter_dir(tmp_path_factory.mktemp(name), cfg, seed=seed)[0]
        for name, seed in (("A", 1), ("B", 2), ("C", 3))
    }


@pytest.fixture(scope="module")
def runs(adapters):
    """Everything both engines generate, computed once."""
    from kserve_amd.engine.engine import LLMEngine
    from tests.test_gpu_engine import _cfg

    res = {}
    engines = {}
    for kind, eager in (("eager", True), ("graph", False)):
        engine = LLMEngine(_cfg(enforce_eager=eager))
        engine.register_lora("A", adapters["A"])
        engine.register_lora("B", adapters["B"])
        res[kind, "mixed"] = run_mixed(engine, [None, "A", "B", "A"])
        res[kind, "graphs_after_mixed"] = len(engine.runner._lora_graphs)
        res[kind, "base"] = run_mixed(engine, [None] * 4)
        # a third adapter, registered after the LoRA graph was captured
        engine.register_lora("C", adapters["C"])
        res[kind, "late"] = run_mixed(engine, ["C", None, "A", "C"])
        res[kind, "graphs_after_late"] = len(engine.runner._lora_graphs)
        engines[kind] = engine
    res["stacks"] = engines["graph"].lora_manager.has_stacks
    del engines
    torch.cuda.empty_cache()
    return res


def test_graph_matches_eager_mixed_adapters(runs):
    assert runs["stacks"]
    assert all(len(t) == MAX_TOKENS for t in runs["graph", "mixed"])
    assert runs["graph", "mixed"] == runs["eager", "mixed"]


def test_lora_decode_replays_graphs(runs):
    assert runs["graph", "graphs_after_mixed"] >= 1
    assert runs["eager", "graphs_after_mixed"] == 0


def test_base_rows_untouched(runs):
    """The base request in the mixed batch equals the same request in an
    all-base batch of the same shape, on the same engine."""
    for kind in ("eager", "graph"):
        assert runs[kind, "mixed"][0] == runs[kind, "base"][0]


def test_adapters_change_tokens(runs):
    mixed, base = runs["graph", "mixed"], runs["graph", "base"]
    for i in (1, 2, 3):
        assert mixed[i] != base[i]
    late = runs["graph", "late"]
    assert late[0] != base[0] and late[3] != base[3]


def test_late_registration_reaches_captured_graph(runs):
    """Slot writes go to the stacks the captured graph already reads: the
    adapter registered after capture matches the eager engine, and no graph
    was captured again for it."""
    assert runs["graph", "late"] == runs["eager", "late"]
    assert runs["graph", "graphs_after_late"] == runs["graph", "graphs_after_mixed"]


def test_segment_switch_first_tokens(runs, adapters):
    """KS_LORA_SEGMENTS=1 (a child process of its own) keeps decode on the
    per-segment GEMMs; the first token of each adapter request matches the
    batched path's."""
    env = dict(os.environ)
    env["KS_LORA_SEGMENTS"] = "1"
    proc = subprocess.run(
        [sys.executable, "-m", "tests.lora_engine_child", adapters["A"],
         adapters["B"]],
        env=env, cwd=REPO, timeout=CHILD_TIMEOUT_S,
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
    )
    assert proc.returncode == 0, (
        f"child exited {proc.returncode}\n{proc.stderr[-2000:]}")
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("TOKENS ")]
    assert len(lines) == 1, proc.stdout[-2000:]
    seg = json.loads(lines[0][len("TOKENS "):])
    batched = runs["graph", "mixed"]
    print("segments:", seg)
    print("batched: ", batched)
    for i in (1, 2, 3):
        assert seg[i][0] == batched[i][0]
