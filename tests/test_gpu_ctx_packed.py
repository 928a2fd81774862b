"""GPU: the GQA-packed split-KV context kernel
(ops.context_attention_varlen(kernel="packed")) on the adversarial cases of
tests/attention_cases.py, against the fp64 reference and the elementwise
allowance the tiled kernel is held to (EPS_MFMA, ratio <= 1)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from kserve_amd import ops
from tests import attention_cases as ac

# (group, Hkv, D, ((q_len, past), ...)) mixed in one batch: contexts on both
# sides of page, page-pair and split boundaries, empty pasts, every RT
SHAPES = {
    "g4kv2d128": (4, 2, 128, ((1, 0), (1, 200), (4, 0), (4, 61), (5, 123),
                              (16, 48), (16, 497), (9, 1015))),
    "g8kv1d128": (8, 1, 128, ((1, 0), (8, 0), (8, 56), (3, 253), (8, 1016),
                              (7, 130))),
    "g3kv2d128": (3, 2, 128, ((1, 0), (21, 0), (21, 43), (5, 123), (13, 500))),
    "g1kv3d128": (1, 3, 128, ((1, 0), (64, 0), (64, 64), (33, 31), (17, 600))),
    "g4kv2d64": (4, 2, 64, ((1, 0), (4, 61), (16, 48), (9, 519))),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.has_native(), "native extension must be present on the GPU box"
    return torch.device("cuda:0")


def _case(shape, window, fp8):
    group, hkv, d, qp = SHAPES[shape]
    return ac.Case(
        f"pk{'8' if fp8 else ''}_{shape}_w{window}", "context", hkv, group, d,
        ctx=tuple(q + p for q, p in qp), q_lens=tuple(q for q, _ in qp),
        window=window, fp8=fp8, share_prefix=True,
        seed=900 + 7 * sorted(SHAPES).index(shape) + window + int(fp8))


def _run(case, dev, **kw):
    inp = ac.build(case)
    return ops.context_attention_varlen(
        ac._strided_rows(inp.q, dev, 32, 32),
        ac._cache_to(inp.k_cache, case, dev),
        ac._cache_to(inp.v_cache, case, dev),
        inp.block_tables.to(dev), inp.cu_seqlens_q.to(dev),
        inp.context_lens.to(dev), inp.max_q_len, inp.scale,
        window=case.window, **kw)


@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("window", [0, 16, 65])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_packed_matches_fp64_reference(dev, shape, window, fp8, splits):
    case = _case(shape, window, fp8)
    ref, absmass = ac.expected(case)
    got = _run(case, dev, kernel="packed", splits=splits)
    ratio = ac.worst_ratio(got, ref, absmass, ac.EPS_MFMA)
    print(f"{case.name} splits={splits}: worst err/allowance = {ratio:.3f}")
    assert ratio <= 1.0, f"{case.name} splits={splits}: {ratio:.2f}x allowance"


@pytest.mark.parametrize("q_len,group", [(65, 1), (17, 4), (9, 8), (22, 3)])
def test_packed_range_and_kernel_names(dev, q_len, group):
    """65 or more packed rows and unknown names raise; "tiled" is today's
    path bit for bit."""
    case = ac.Case(f"pk_rows_{q_len}x{group}", "context", 2, group, 128,
                   ctx=(q_len + 40, q_len + 35), q_lens=(q_len, q_len),
                   share_prefix=True, seed=990 + group)
    assert q_len * group >= 65
    assert not ops.context_packed_supported(q_len, 2 * group, 2, 128)
    with pytest.raises(ValueError):
        _run(case, dev, kernel="packed")
    with pytest.raises(ValueError):
        _run(case, dev, kernel="ring")
    assert torch.equal(_run(case, dev, kernel="tiled"), _run(case, dev))


def test_engine_speculation_with_packed_kernel(dev, monkeypatch):
    """Greedy prompt-lookup speculation on the tiny engine with
    ctx_attn="packed": every verify step runs the packed kernel (none falls
    back to "tiled"), the tokens are repeatable, and the first token is the
    tiled engine's. Later tokens are not compared across kernels (bf16
    near-ties on a random model)."""
    from kserve_amd.engine.config import SchedulerConfig
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams
    from tests.test_gpu_engine import _cfg

    prompts = [[1, 2, 3, 4] * 6 + [1, 2], [7, 8, 9] * 5]
    sp = SamplingParams(temperature=0.0, max_tokens=16)
    real, calls = ops.context_attention_varlen, []

    def spy(*args, **kw):
        calls.append(kw.get("kernel", "tiled"))
        return real(*args, **kw)

    monkeypatch.setattr(ops, "context_attention_varlen", spy)
    runs = {}
    for kernel in ("tiled", "packed"):
        cfg = _cfg(enforce_eager=True)
        cfg.model.ctx_attn = kernel
        cfg.scheduler = SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=2048, max_model_len=512,
            speculative_ngram=4)
        torch.manual_seed(0)
        engine = LLMEngine(cfg)
        runs[kernel] = [
            [o.output_token_ids for o in engine.generate(prompts, sp).values()]
            for _ in range(2 if kernel == "packed" else 1)]
        assert calls and set(calls) == {kernel}, (kernel, set(calls))
        calls.clear()
        del engine
        torch.cuda.empty_cache()
    assert runs["packed"][0] == runs["packed"][1]
    assert all(len(t) == 16 for t in runs["packed"][0])
    assert [t[0] for t in runs["packed"][0]] == [t[0] for t in runs["tiled"][0]]
