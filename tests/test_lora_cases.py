"""CPU checks of the batched multi-LoRA ops' reference path and of the test
cases themselves (tests/lora_cases.py): the fp32 torch_ref ops meet the
derived allowance, agree with the per-segment GEMM path, `_lora_meta`'s row
slots agree with its segments, every mutant of the reference misses the
allowance by 10x on some case, and the adapter manager enforces its caps."""

import json
from types import SimpleNamespace

import pytest
import torch

from tests import lora_cases as lc


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_torch_ref_within_allowance(case):
    ratio, untouched_ok = lc.check_case(case, "cpu")
    print(f"{case.name}: err/allowance = {ratio:.3f}")
    assert untouched_ok, "sentinel columns or skipped rows changed"
    assert ratio <= 1.0


def test_cases_cover_the_edges():
    """Every rank is used somewhere and left out somewhere; batches with room
    have -1 rows, an out-of-range row and a non-monotone slot order."""
    used, unused = set(), set()
    for case in lc.CASES:
        slots = lc.build(case).slot_idx.tolist()
        assert case.unused_slot not in slots
        unused.add(case.unused_slot)
        used.update(s for s in slots if 0 <= s < lc.S)
        if case.T >= 3:
            assert -1 in slots
        if case.T >= 33:
            assert lc.S in slots
            valid = [s for s in slots if 0 <= s < lc.S]
            assert len(set(valid)) == lc.S - 1
            assert valid != sorted(valid)
    assert used == set(range(lc.S)) and unused == set(range(lc.S))


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_mutant_misses_allowance(mutant):
    """The cases can fail: each wrong reading of the contract is off by at
    least 10x the allowance on at least one case."""
    worst = 0.0
    for case in lc.CASES:
        ref, absmass = lc.expected(case)
        got, _ = lc.reference(lc.build(case), mutate=mutant)
        worst = max(worst, lc.worst_ratio(got, ref, absmass, case.K))
    assert worst >= 10.0, f"{mutant}: worst err/allowance {worst:.2f}"


# ---------------------------------------------------------------------------
# torch_ref ops against the per-segment path of the engine
# ---------------------------------------------------------------------------
class _Batch(SimpleNamespace):
    pass


def _runner(manager=None):
    from kserve_amd.engine.model_runner import ModelRunner

    r = ModelRunner.__new__(ModelRunner)
    r.device = torch.device("cpu")
    r.lora_manager = manager
    return r


def _batch(lora_ids, widths):
    return _Batch(
        requests=[SimpleNamespace(lora_id=i) for i in lora_ids],
        num_scheduled_tokens=list(widths),
    )


@pytest.mark.parametrize("per_request_rows", [True, False])
def test_row_slots_agree_with_segments(per_request_rows):
    g = torch.Generator().manual_seed(5)
    for trial in range(20):
        n = int(torch.randint(1, 12, (1,), generator=g))
        ids = torch.randint(0, 4, (n,), generator=g).tolist()
        widths = torch.randint(1, 6, (n,), generator=g).tolist()
        meta = _runner()._lora_meta(_batch(ids, widths), per_request_rows)
        assert meta.decode is per_request_rows
        total = n if per_request_rows else sum(widths)
        assert meta.row_slots.dtype == torch.int32
        assert meta.row_slots.shape == (total,)
        from_segments = torch.full((total,), -1, dtype=torch.int32)
        for aid, s, e in meta.segments:
            assert aid > 0 and 0 <= s < e <= total
            assert bool((from_segments[s:e] == -1).all())
            from_segments[s:e] = aid - 1
        assert torch.equal(meta.row_slots, from_segments)


def test_torch_ref_matches_segment_path():
    """ops.lora_shrink + ops.lora_expand_add on stacks == LoRALayerWeights
    .delta over `_lora_meta` segments, on random mixed batches (fp32, where
    the two differ only by summation order)."""
    from kserve_amd import ops
    from kserve_amd.engine.lora import LoRABatchMeta, LoRALayerWeights

    g = torch.Generator().manual_seed(11)
    K, N, Rcap, nslots = 128, 192, 16, 3
    ranks = [4, 8, 12]
    scales = [2.0, 0.5, 1.25]
    weights = {}
    a_stack = torch.zeros(nslots, Rcap, K)
    b_stack = torch.zeros(nslots, N, Rcap)
    for s in range(nslots):
        a = torch.randn(ranks[s], K, generator=g) / K ** 0.5
        b = torch.randn(N, ranks[s], generator=g) / ranks[s] ** 0.5
        weights[s + 1] = LoRALayerWeights(a, b, scales[s])
        a_stack[s, : ranks[s]] = a
        b_stack[s, :, : ranks[s]] = b
    manager = SimpleNamespace(
        layer_weights=lambda aid, layer, module: weights.get(aid),
        has_stacks=False,
    )
    for trial in range(8):
        n = int(torch.randint(1, 20, (1,), generator=g))
        ids = torch.randint(0, nslots + 1, (n,), generator=g).tolist()
        meta = _runner(manager)._lora_meta(_batch(ids, [1] * n), True)
        x = torch.randn(n, K, generator=g)
        y0 = torch.randn(n, N + 64, generator=g)
        seg = y0.clone()
        LoRABatchMeta(meta.segments, manager).apply(0, "q_proj", x, seg, 64)
        got = y0.clone()
        tmp = ops.lora_shrink(
            x, a_stack, torch.tensor(ranks, dtype=torch.int32), meta.row_slots
        )
        ops.lora_expand_add(
            got, tmp, b_stack, torch.tensor(scales),
            torch.tensor(ranks, dtype=torch.int32), meta.row_slots, 64,
        )
        torch.testing.assert_close(got, seg, rtol=1e-5, atol=1e-5)
        base_rows = [i for i, a in enumerate(ids) if a == 0]
        assert torch.equal(got[base_rows], y0[base_rows])
        assert torch.equal(got[:, :64], y0[:, :64])


# ---------------------------------------------------------------------------
# adapter manager caps
# ---------------------------------------------------------------------------
def _adapter_dir(path, rank, hidden=64):
    from safetensors.torch import save_file

    path.mkdir()
    pre = "base_model.model.model.layers.0.self_attn.q_proj"
    save_file(
        {
            f"{pre}.lora_A.weight": torch.zeros(rank, hidden),
            f"{pre}.lora_B.weight": torch.zeros(hidden, rank),
        },
        str(path / "adapter_model.safetensors"),
    )
    (path / "adapter_config.json").write_text(
        json.dumps({"r": rank, "lora_alpha": rank})
    )
    return str(path)


def test_manager_rejects_rank_over_cap(tmp_path):
    from kserve_amd.engine.lora import LoRAManager

    mgr = LoRAManager("cpu", torch.float32, max_lora_rank=16)
    assert mgr.register("ok", _adapter_dir(tmp_path / "ok", 16)) == 1
    with pytest.raises(ValueError, match="max_lora_rank"):
        mgr.register("big", _adapter_dir(tmp_path / "big", 24))
    # the rejected adapter used up neither a name nor an id
    assert mgr.names() == ["ok"]
    assert mgr.register("next", _adapter_dir(tmp_path / "next", 8)) == 2


def test_manager_rejects_ninth_adapter(tmp_path):
    from kserve_amd.engine.config import EngineConfig
    from kserve_amd.engine.lora import LoRAManager

    cfg = EngineConfig().lora
    assert (cfg.max_loras, cfg.max_lora_rank) == (8, 64)
    mgr = LoRAManager("cpu", torch.float32, max_loras=cfg.max_loras,
                      max_lora_rank=cfg.max_lora_rank)
    path = _adapter_dir(tmp_path / "a", 4)
    for i in range(8):
        assert mgr.register(f"a{i}", path) == i + 1
    with pytest.raises(ValueError, match="max_loras"):
        mgr.register("a8", path)
    assert mgr.register("a3", path) == 4  # known names still resolve
