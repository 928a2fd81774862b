"""End-to-end LLMEngine tests on CPU (tiny model, torch-ref ops)."""

import pytest
import torch

from kserve_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    ModelConfig,
    SchedulerConfig,
)
from kserve_amd.engine.engine import LLMEngine
from kserve_amd.engine.sampling_params import SamplingParams


def make_engine(**kw):
    cfg = EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(block_size=4, num_gpu_blocks=128),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=256, max_model_len=128
        ),
        device="cpu",
        eos_token_id=-1,  # disable EOS for random-weight tests
        **kw,
    )
    return LLMEngine(cfg)


@pytest.fixture(scope="module")
def engine():
    torch.manual_seed(0)
    return make_engine()


def test_generate_greedy_lengths(engine):
    sp = SamplingParams(temperature=0.0, max_tokens=5)
    prompts = [[1, 2, 3], [4, 5, 6, 7, 8]]
    results = engine.generate(prompts, sp)
    assert len(results) == 2
    for out in results.values():
        assert out.finished
        assert out.finish_reason == "length"
        assert len(out.output_token_ids) == 5


def test_greedy_deterministic(engine):
    sp = SamplingParams(temperature=0.0, max_tokens=8)
    r1 = engine.generate([[10, 11, 12]], sp)
    r2 = engine.generate([[10, 11, 12]], sp)
    toks1 = list(r1.values())[0].output_token_ids
    toks2 = list(r2.values())[0].output_token_ids
    assert toks1 == toks2


def test_batched_equals_single(engine):
    """Continuous batching must not change greedy outputs."""
    sp = SamplingParams(temperature=0.0, max_tokens=6)
    single = {}
    prompts = [[1, 2, 3, 4], [9, 8, 7], [20, 21, 22, 23, 24, 25]]
    for p in prompts:
        out = list(engine.generate([p], sp).values())[0]
        single[tuple(p)] = out.output_token_ids
    batched = engine.generate(prompts, sp)
    outs = list(batched.values())
    for p, out in zip(prompts, outs):
        assert out.output_token_ids == single[tuple(p)], f"prompt {p}"


def test_sampling_with_seed(engine):
    sp = SamplingParams(temperature=0.8, top_k=20, max_tokens=6, seed=42)
    out = list(engine.generate([[5, 6, 7]], sp).values())[0]
    assert len(out.output_token_ids) == 6
    assert all(0 <= t < 128 for t in out.output_token_ids)


def test_stop_token(engine):
    # discover the greedy continuation, then use its 3rd token as a stop token
    sp = SamplingParams(temperature=0.0, max_tokens=8)
    base = list(engine.generate([[30, 31]], sp).values())[0].output_token_ids
    stop_tok = base[2]
    sp2 = SamplingParams(temperature=0.0, max_tokens=8, stop_token_ids=[stop_tok])
    out = list(engine.generate([[30, 31]], sp2).values())[0]
    assert out.finish_reason == "stop"
    assert out.output_token_ids == base[:3]


def test_many_concurrent_requests(engine):
    """More requests than max_num_seqs: queueing + multiple waves."""
    sp = SamplingParams(temperature=0.0, max_tokens=3)
    prompts = [[i, i + 1, i + 2] for i in range(20)]
    results = engine.generate(prompts, sp)
    assert len(results) == 20
    for out in results.values():
        assert len(out.output_token_ids) == 3


def test_preemption_recovers():
    """Tiny KV pool forces preemption; all requests must still finish with
    identical greedy outputs to an unconstrained engine."""
    torch.manual_seed(0)
    engine_small = make_engine()
    # rebuild with small pool
    torch.manual_seed(0)
    cfg = EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(block_size=4, num_gpu_blocks=14),
        scheduler=SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=256, max_model_len=128
        ),
        device="cpu",
        eos_token_id=-1,
    )
    engine_tiny = LLMEngine(cfg)
    sp = SamplingParams(temperature=0.0, max_tokens=10)
    prompts = [[1, 2, 3, 4], [9, 8, 7, 6], [15, 16, 17, 18]]
    big = engine_small.generate(prompts, sp)
    small = engine_tiny.generate(prompts, sp)
    big_outs = [o.output_token_ids for o in big.values()]
    small_outs = [o.output_token_ids for o in small.values()]
    assert big_outs == small_outs


def test_repetition_penalty_changes_output(engine):
    """A strong repetition penalty must break greedy loops."""
    base = SamplingParams(temperature=0.0, max_tokens=12)
    out_base = list(engine.generate([[40, 41]], base).values())[0].output_token_ids
    pen = SamplingParams(
        temperature=0.0, max_tokens=12, repetition_penalty=5.0
    )
    out_pen = list(engine.generate([[40, 41]], pen).values())[0].output_token_ids
    # with random weights greedy usually repeats; penalty must diverge and
    # produce fewer repeats
    def max_run(toks):
        best = run_len = 1
        for a, b in zip(toks, toks[1:]):
            run_len = run_len + 1 if a == b else 1
            best = max(best, run_len)
        return best

    assert out_pen != out_base or max_run(out_pen) <= max_run(out_base)
    assert len(set(out_pen)) >= len(set(out_base))


def test_chunked_prefill_matches_full():
    """Chunked prefill (paged-context attention) must reproduce full-prefill
    greedy outputs exactly: chunk boundaries change kernel tiling, not math."""
    torch.manual_seed(0)
    full = make_engine()
    torch.manual_seed(0)
    cfg = EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(block_size=4, num_gpu_blocks=128),
        scheduler=SchedulerConfig(
            max_num_seqs=8,
            max_num_batched_tokens=8,  # prompts below are longer -> chunks
            max_model_len=128,
            enable_chunked_prefill=True,
        ),
        device="cpu",
        eos_token_id=-1,
    )
    chunked = LLMEngine(cfg)
    sp = SamplingParams(temperature=0.0, max_tokens=6)
    prompts = [
        list(range(1, 20)),          # 19 tokens -> 3 chunks
        list(range(30, 39)),         # 9 tokens -> 2 chunks
        [3, 1, 4],                   # fits one chunk
    ]
    a = full.generate(prompts, sp)
    b = chunked.generate(prompts, sp)
    assert [o.output_token_ids for o in a.values()] == [
        o.output_token_ids for o in b.values()
    ]


def test_fp8_kv_cache_cpu():
    """fp8 E4M3 KV cache (opt-in): engine runs and its greedy logits stay
    close to the bf16-KV engine's (quantization noise only)."""
    torch.manual_seed(0)
    base = make_engine()
    torch.manual_seed(0)
    cfg = EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(block_size=4, num_gpu_blocks=128, kv_cache_dtype="fp8"),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=256, max_model_len=128
        ),
        device="cpu",
        eos_token_id=-1,
    )
    fp8 = LLMEngine(cfg)
    assert fp8.runner.kv_caches[0][0].dtype == torch.float8_e4m3fn
    sp = SamplingParams(temperature=0.0, max_tokens=8)
    a = list(base.generate([[1, 2, 3, 4, 5]], sp).values())[0]
    b = list(fp8.generate([[1, 2, 3, 4, 5]], sp).values())[0]
    assert len(b.output_token_ids) == 8
    # prefill (first token) ignores the cache entirely -> identical
    assert a.output_token_ids[0] == b.output_token_ids[0]


@pytest.mark.timeout(180)
def test_engine_fuzz_mixed_workload():
    """Mini-soak: 150 requests with randomized lengths/sampling params under
    a small KV pool (preemption active). Everything must finish, with the
    right lengths, and the pool must drain back to empty."""
    import random

    rng = random.Random(1234)
    torch.manual_seed(0)
    cfg = EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(
            block_size=4, num_gpu_blocks=64, enable_prefix_caching=True
        ),
        scheduler=SchedulerConfig(
            max_num_seqs=6,
            max_num_batched_tokens=64,
            max_model_len=96,
            enable_chunked_prefill=True,
            speculative_ngram=3,
        ),
        device="cpu",
        eos_token_id=-1,
    )
    engine = LLMEngine(cfg)
    expected = {}
    shared = [7, 8, 9, 10, 11, 12, 13, 14]
    for i in range(150):
        plen = rng.randint(1, 40)
        prompt = (shared if rng.random() < 0.4 else []) + [
            rng.randint(0, 127) for _ in range(plen)
        ]
        prompt = prompt[:40]
        max_toks = rng.randint(1, 12)
        sp = SamplingParams(
            temperature=rng.choice([0.0, 0.0, 0.8]),
            top_k=rng.choice([-1, 5]),
            top_p=rng.choice([1.0, 0.9]),
            max_tokens=max_toks,
            seed=i,
        )
        rid = engine.add_request(prompt, sp, request_id=f"f{i}")
        expected[rid] = max_toks
    done = {}
    steps = 0
    while engine.has_unfinished():
        for out in engine.step():
            if out.finished:
                done[out.request_id] = len(out.output_token_ids)
        steps += 1
        assert steps < 5000, "engine wedged"
    assert len(done) == 150
    for rid, n in done.items():
        assert n == expected[rid], (rid, n, expected[rid])
    bm = engine.scheduler.block_manager
    assert bm.num_free_blocks == bm.num_blocks - 1  # all blocks returned


def test_min_p_restricts_support(engine):
    """min_p close to 1 forces near-greedy sampling; support must collapse
    to the argmax token across seeds."""
    greedy = engine.generate(
        [[1, 2, 3]], SamplingParams(temperature=0.0, max_tokens=1)
    )
    g_tok = list(greedy.values())[0].output_token_ids[0]
    for seed in range(5):
        out = engine.generate(
            [[1, 2, 3]],
            SamplingParams(
                temperature=1.0, min_p=0.999, max_tokens=1, seed=seed
            ),
        )
        assert list(out.values())[0].output_token_ids[0] == g_tok


def test_logit_bias(engine):
    """+100 bias forces a token; -100 bans the greedy choice."""
    base = engine.generate(
        [[4, 5, 6]], SamplingParams(temperature=0.0, max_tokens=1)
    )
    g_tok = list(base.values())[0].output_token_ids[0]
    forced = engine.generate(
        [[4, 5, 6]],
        SamplingParams(temperature=0.0, max_tokens=1, logit_bias={77: 100.0}),
    )
    assert list(forced.values())[0].output_token_ids[0] == 77
    banned = engine.generate(
        [[4, 5, 6]],
        SamplingParams(
            temperature=0.0, max_tokens=1, logit_bias={g_tok: -100.0}
        ),
    )
    assert list(banned.values())[0].output_token_ids[0] != g_tok


class TestSampledWindows:
    """Multi-step decode windows at temperature>0 (round-2: the in-graph
    fused sampler removes the greedy-only window restriction; CPU exercises
    the eager path of ModelRunner.multi_step_decode(sampled=True))."""

    def _engine(self):
        torch.manual_seed(0)
        cfg = EngineConfig(
            model=ModelConfig.tiny(vocab_size=128),
            cache=CacheConfig(block_size=4, num_gpu_blocks=256),
            scheduler=SchedulerConfig(
                max_num_seqs=8,
                max_num_batched_tokens=256,
                max_model_len=128,
                multi_step=4,
            ),
            device="cpu",
            eos_token_id=-1,
        )
        return LLMEngine(cfg)

    def test_sampled_batch_uses_windows(self):
        eng = self._engine()
        sp = SamplingParams(temperature=0.8, top_p=0.9, max_tokens=12,
                            seed=7, ignore_eos=True)
        for i in range(3):
            eng.add_request([1 + i, 2, 3], sp, request_id=f"s{i}")
        steps = 0
        outs = {}
        while eng.scheduler.has_unfinished() and steps < 40:
            for o in eng.step():
                outs.setdefault(o.request_id, []).extend(o.new_token_ids)
            steps += 1
        assert all(len(v) == 12 for v in outs.values())
        # windows mean fewer engine steps than tokens: 1 prefill + ceil(12/4)
        # window steps (vs 12 single-token steps without windows)
        assert steps <= 1 + 3 + 2

    def test_mixed_greedy_and_sampled_window(self):
        eng = self._engine()
        greedy = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
        samp = SamplingParams(temperature=1.0, max_tokens=8, seed=3,
                              ignore_eos=True)
        eng.add_request([5, 6, 7], greedy, request_id="g")
        eng.add_request([5, 6, 7], samp, request_id="s")
        outs = {}
        steps = 0
        while eng.scheduler.has_unfinished() and steps < 40:
            for o in eng.step():
                outs.setdefault(o.request_id, []).extend(o.new_token_ids)
            steps += 1
        assert len(outs["g"]) == 8 and len(outs["s"]) == 8
        # the greedy row must match a pure-greedy run exactly
        ref_eng = self._engine()
        ref = ref_eng.generate([[5, 6, 7]], greedy)
        assert outs["g"] == list(ref.values())[0].output_token_ids

    def test_penalties_fall_back_to_stepwise(self):
        """Requests with penalties can't window (host must see history);
        they still produce max_tokens tokens via single steps."""
        eng = self._engine()
        sp = SamplingParams(
            temperature=0.8, max_tokens=6, presence_penalty=0.5,
            ignore_eos=True,
        )
        eng.add_request([9, 9, 9], sp, request_id="p")
        outs = []
        steps = 0
        while eng.scheduler.has_unfinished() and steps < 40:
            for o in eng.step():
                outs.extend(o.new_token_ids)
            steps += 1
        assert len(outs) == 6
        # no windows: one token per step (prefill samples the first token,
        # then 5 single-token decode steps)
        assert steps >= 6


@pytest.mark.parametrize("kv_dtype", ["auto", "fp8"])
def test_gpu_kv_cache_allocation_is_zero_filled(engine, monkeypatch, kv_dtype):
    """The attention kernels are exact for any finite stale cache data and
    undefined for non-finite, so the pool the runner allocates for a GPU
    must not be uninitialised memory. No GPU needed: flip the runner's
    device flag, forbid torch.empty, and look at what it allocates."""
    from kserve_amd.engine import model_runner as mr

    runner = engine.runner
    assert runner._kv_allocator() is torch.zeros
    saved = (runner.is_cuda, runner.kv_caches, runner.num_gpu_blocks,
             runner.config.cache.kv_cache_dtype)

    def no_empty(*a, **k):
        raise AssertionError("KV cache allocated with torch.empty")

    monkeypatch.setattr(runner, "is_cuda", True)
    monkeypatch.setattr(runner, "_allocate_cpu_kv", lambda: None)
    monkeypatch.setattr(runner.config.cache, "kv_cache_dtype", kv_dtype)
    monkeypatch.setattr(mr.torch, "empty", no_empty)
    try:
        runner.allocate_kv_cache(3)
        assert len(runner.kv_caches) == runner._num_local_layers()
        for k, v in runner.kv_caches:
            assert k.shape[0] == 3
            assert not bool(k.view(torch.uint8).any())
            assert not bool(v.view(torch.uint8).any())
    finally:
        monkeypatch.undo()
        (runner.is_cuda, runner.kv_caches, runner.num_gpu_blocks,
         runner.config.cache.kv_cache_dtype) = saved
