"""bench.py command-line contract: the JSON result line, --steps really
setting the timed step count, --full, and --dump-outputs (format, size
budget, run-to-run reproducibility of the inputs). Runs the tiny model on
CPU so it needs no GPU."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, CONC, WINDOW = 3, 1, 5, 8


def run_bench(*extra):
    env = dict(os.environ)
    # CPU path even where a GPU is present
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    proc = subprocess.run(
        [
            sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
            "--steps", str(STEPS), "--warmup", str(WARMUP),
            "--model", "tiny", "--concurrency", str(CONC),
            "--prompt-len", "12", *extra,
        ],
        env=env, cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path_factory.mktemp(name)
        out.append((run_bench("--dump-outputs", str(d), *extra), d))
    return out


def test_result_line_fields(runs):
    for result, _ in runs:
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in result
        assert result["steps"] == STEPS and result["warmup"] == WARMUP
        assert result["unit"] == "tok/s" and result["higher_is_better"] is True
        assert result["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region: STEPS steps
        # of WINDOW tokens for each of CONC sequences
        tokens = STEPS * WINDOW * CONC
        implied = tokens / (result["ms_per_step"] * STEPS / 1000.0)
        assert result["value"] == pytest.approx(implied, rel=1e-2)


def test_dump_outputs_format(runs):
    _, d = runs[0]
    assert sorted(os.listdir(d)) == ["new_token_ids.npy",
                                     "output_token_ids.npy"]
    new = np.load(d / "new_token_ids.npy")
    every = np.load(d / "output_token_ids.npy")
    assert new.dtype == np.float32 and every.dtype == np.float32
    assert new.shape == (CONC, WINDOW)
    # first token from prefill, then one window per warmup and timed step
    assert every.shape == (CONC, 1 + (WARMUP + STEPS) * WINDOW)
    assert (new >= 0).all() and (new < 1024).all()
    # the last step's tokens are the tail of everything decoded so far
    assert (every[:, -WINDOW:] == new).all()


def test_dump_outputs_reproducible(runs):
    (_, a), (_, b) = runs
    for name in ("new_token_ids.npy", "output_token_ids.npy"):
        assert (np.load(a / name) == np.load(b / name)).all()


def test_dump_budget_keeps_seeded_row_sample(tmp_path, monkeypatch):
    import bench  # repository root is on sys.path (tests/conftest.py)

    class Out:
        def __init__(self, i):
            self.request_id = f"r{i}"
            self.new_token_ids = [i, i + 1]
            self.output_token_ids = [i] * 6

    n = 100
    ids = [f"r{i}" for i in range(n)]
    outs = [Out(i) for i in range(n) if i != 7]  # r7 not in the last batch
    row_bytes = (2 + 6) * 4
    monkeypatch.setattr(bench, "_DUMP_BUDGET_BYTES", 10 * (row_bytes + 4))
    bench._dump_outputs(str(tmp_path / "x"), 0, ids, outs)
    bench._dump_outputs(str(tmp_path / "y"), 0, ids, outs)
    total = 0
    for name in ("new_token_ids", "output_token_ids", "rows"):
        x = np.load(tmp_path / "x" / f"{name}.npy")
        y = np.load(tmp_path / "y" / f"{name}.npy")
        assert x.dtype == np.float32 and (x == y).all()
        total += x.nbytes
    assert total <= 10 * (row_bytes + 4)
    rows = np.load(tmp_path / "x" / "rows.npy").astype(int)
    assert len(rows) == 10 and len(set(rows)) == 10
    new = np.load(tmp_path / "x" / "new_token_ids.npy")
    for r, row in zip(rows, new):
        assert row.tolist() == ([-1, -1] if r == 7 else [r, r + 1])

    # under the budget every row is kept and no rows.npy is written
    monkeypatch.setattr(bench, "_DUMP_BUDGET_BYTES", 64 * 1024 * 1024)
    bench._dump_outputs(str(tmp_path / "z"), 0, ids, outs)
    assert sorted(os.listdir(tmp_path / "z")) == ["new_token_ids.npy",
                                                  "output_token_ids.npy"]
    assert np.load(tmp_path / "z" / "new_token_ids.npy")[7].tolist() == [-1, -1]
