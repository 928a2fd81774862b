"""Engine-level checks of in-graph logit processors, shared by the CPU run
(eager fallback of multi_step_decode, tests/test_logit_window.py) and the GPU
run (captured graphs, tests/test_gpu_logit_window.py). The engine is the tiny
one of tests/test_gpu_engine.py::_cfg with multi_step=4."""

import numpy as np
import torch

PROMPTS = [[1, 2, 3, 4, 5], [100, 200, 300], [7, 8, 9, 10]]


def make_cfg(device, multi_step=4, slots=2):
    from kserve_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        ModelConfig,
        SchedulerConfig,
    )

    return EngineConfig(
        model=ModelConfig(
            vocab_size=2048,
            hidden_size=512,
            intermediate_size=1024,
            num_layers=4,
            num_heads=4,
            num_kv_heads=2,
            head_dim=128,
            max_position_embeddings=1024,
            model_name="gpu-tiny",
        ),
        cache=CacheConfig(block_size=16, num_gpu_blocks=128),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=2048, max_model_len=512,
            multi_step=multi_step, logit_processor_slots=slots,
        ),
        device=device,
        seed=0,
        eos_token_id=-1,
        enforce_eager=False,
    )


def make_engine(device, multi_step=4, slots=2):
    from kserve_amd.engine.engine import LLMEngine

    engine = LLMEngine(make_cfg(device, multi_step, slots))
    calls = []
    real = engine.runner.multi_step_decode

    def spy(batch, block_manager, k_steps, sampled=False, processed=False):
        calls.append(
            {"k": k_steps, "sampled": sampled, "processed": processed,
             "n": len(batch.requests)}
        )
        return real(
            batch, block_manager, k_steps, sampled=sampled,
            processed=processed,
        )

    engine.runner.multi_step_decode = spy
    return engine, calls


def tokens(out):
    return [o.output_token_ids for o in out.values()]


def check_windows_are_used(device):
    from kserve_amd.engine.sampling_params import SamplingParams

    sp = SamplingParams(
        temperature=0.0, max_tokens=13, repetition_penalty=1.1,
        frequency_penalty=0.2,
    )
    engine, calls = make_engine(device, slots=2)
    out = engine.generate(PROMPTS[:2], sp)
    assert all(len(t) == 13 for t in tokens(out))
    assert calls and all(c["processed"] and c["k"] > 1 for c in calls)
    # every slot came back
    assert engine.runner.logit_state.num_free == 2

    engine, calls = make_engine(device, slots=0)
    assert engine.runner.logit_state is None
    out = engine.generate(PROMPTS[:2], sp)
    assert all(len(t) == 13 for t in tokens(out))
    assert calls == []


def check_no_repeats(device):
    from kserve_amd.engine.sampling_params import SamplingParams

    engine, calls = make_engine(device, slots=3)
    out = engine.generate(
        PROMPTS,
        SamplingParams(temperature=0.0, max_tokens=24, presence_penalty=1e4),
    )
    assert any(c["processed"] for c in calls)
    for toks in tokens(out):
        assert len(toks) == 24
        assert len(set(toks)) == 24, toks


def check_device_path_equals_host_path(device):
    """presence 0.5, frequency 0.25, repetition 2.0 and bias 2.0 on bf16
    logits: every operation is exact in fp32, so the two paths round the
    same numbers and greedy tokens are identical."""
    from kserve_amd.engine.sampling_params import SamplingParams

    sp = SamplingParams(
        temperature=0.0, max_tokens=17, presence_penalty=0.5,
        frequency_penalty=0.25, repetition_penalty=2.0, logit_bias={5: 2.0},
    )
    host, host_calls = make_engine(device, multi_step=1, slots=0)
    want = tokens(host.generate(PROMPTS, sp))
    assert host_calls == []
    del host
    dev, dev_calls = make_engine(device, multi_step=4, slots=3)
    got = tokens(dev.generate(PROMPTS, sp))
    assert dev_calls and all(c["processed"] for c in dev_calls)
    assert got == want


def _run_four(device, slots):
    """3 penalty requests (6, 14, 22 tokens) and a plain one, stepped by
    hand; with slots > 0 the state invariants are checked after every
    step. Returns (tokens of the plain request, log of the checks)."""
    from kserve_amd.engine.sampling_params import SamplingParams

    engine, calls = make_engine(device, slots=slots)
    state = engine.runner.logit_state
    prompts = PROMPTS + [[40, 41, 42, 43, 44, 45]]
    lens = [6, 14, 22]
    reqs = []
    for i, p in enumerate(prompts):
        if i < 3:
            sp = SamplingParams(
                temperature=0.0, max_tokens=lens[i], presence_penalty=0.5,
                frequency_penalty=0.25,
            )
        else:
            sp = SamplingParams(temperature=0.0, max_tokens=22)
        rid = engine.add_request(p, sp, request_id=f"r{i}")
        reqs.append(rid)
    live = {r.request_id: r for r in engine.scheduler.waiting}
    assert set(live) == {"r0", "r1", "r2", "r3"}
    log = {"third_slot_step": None, "windows_checked": 0, "steps": 0}
    final = {}
    while engine.has_unfinished():
        n_calls = len(calls)
        for o in engine.step():
            if o.finished:
                final[o.request_id] = list(o.output_token_ids)
        log["steps"] += 1
        if state is None:
            continue
        windowed = len(calls) > n_calls and calls[-1]["processed"]
        counts = state.counts.cpu().numpy()
        for rid, r in live.items():
            slot = state.slot_of(rid)
            if r.is_finished:
                assert slot == -1, "finished request still holds a slot"
                continue
            if slot < 0:
                continue
            synced = state.synced(rid)
            want = np.bincount(
                np.asarray(r.output_token_ids[:synced], dtype=np.int64),
                minlength=counts.shape[1],
            )
            assert np.array_equal(counts[slot], want), (rid, log["steps"])
            if windowed:
                assert synced == len(r.output_token_ids)
                log["windows_checked"] += 1
        assert state.slot_of("r3") == -1
        if log["third_slot_step"] is None and state.slot_of("r2") >= 0:
            log["third_slot_step"] = log["steps"]
            # it could only get the slot that r0 (6 tokens) gave back
            assert live["r0"].is_finished
            assert not live["r1"].is_finished
            assert state.slot_of("r1") >= 0
            assert len(live["r2"].output_token_ids) >= 6
    log["calls"] = list(calls)
    assert [len(final[r]) for r in ("r0", "r1", "r2", "r3")] == [6, 14, 22, 22]
    return final, log


def check_count_invariant_and_slot_reuse(device):
    final, log = _run_four(device, slots=2)
    assert log["third_slot_step"] is not None
    assert log["windows_checked"] > 0
    calls = log["calls"]
    # no window while r2 had no slot (all four were in the batch)
    assert all(c["processed"] for c in calls)
    assert all(c["n"] < 4 for c in calls)
    plain, plain_log = _run_four(device, slots=0)
    assert plain_log["calls"] == []
    assert final["r3"] == plain["r3"]


def check_min_p_rides_windows(device):
    """top_k = 1 adds no noise and breaks ties like greedy, and the row
    maximum always survives min-p, so the tokens are the greedy ones."""
    from kserve_amd.engine.sampling_params import SamplingParams

    engine, calls = make_engine(device, slots=3)
    got = tokens(
        engine.generate(
            PROMPTS,
            SamplingParams(temperature=0.7, top_k=1, min_p=0.5, max_tokens=13),
        )
    )
    assert calls and all(c["processed"] for c in calls)
    n_lp = len(calls)
    want = tokens(
        engine.generate(PROMPTS, SamplingParams(temperature=0.0, max_tokens=13))
    )
    assert all(not c["processed"] for c in calls[n_lp:])
    assert got == want
