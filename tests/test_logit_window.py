"""In-graph logit processors through the engine, on the CPU: the eager
fallback of ModelRunner.multi_step_decode(processed=True) applies the same
ops per step as the captured graph (tests/test_gpu_logit_window.py)."""

from tests import logit_window_common as lw


def test_windows_are_used():
    lw.check_windows_are_used("cpu")


def test_no_repeats_under_a_huge_presence_penalty():
    lw.check_no_repeats("cpu")


def test_device_path_equals_host_path():
    lw.check_device_path_equals_host_path("cpu")


def test_count_invariant_and_slot_reuse():
    lw.check_count_invariant_and_slot_reuse("cpu")


def test_min_p_rides_windows():
    lw.check_min_p_rides_windows("cpu")


def test_long_bias_list_stays_on_the_host_path():
    from kserve_amd.engine.logit_state import MAX_BIAS
    from kserve_amd.engine.sampling_params import SamplingParams

    engine, calls = lw.make_engine("cpu", slots=2)
    bias = {t: 0.5 for t in range(MAX_BIAS + 1)}
    out = engine.generate(
        lw.PROMPTS[:1],
        SamplingParams(temperature=0.0, max_tokens=6, logit_bias=bias),
    )
    assert [len(t) for t in lw.tokens(out)] == [6]
    assert calls == []
    assert engine.runner.logit_state.num_free == 2


def test_abort_gives_the_slot_back():
    from kserve_amd.engine.sampling_params import SamplingParams

    engine, calls = lw.make_engine("cpu", slots=1)
    rid = engine.add_request(
        lw.PROMPTS[0],
        SamplingParams(temperature=0.0, max_tokens=40, presence_penalty=0.5),
    )
    while not calls:
        engine.step()
    assert engine.runner.logit_state.num_free == 0
    engine.abort_request(rid)
    assert engine.runner.logit_state.num_free == 1
