"""GPU: the fused-dequant MFMA tile GEMM (csrc/wq_tile_gemm.hip) for fp8 and
MXFP4 weights: exact placement on one-hot inputs, numerics against fp64,
ops.linear_w8 / linear_w4 dispatch with tile=True, hipGraph replay and the
engine with quant_gemm="tile". Inputs are those of the existing quant tests."""

import pytest
import torch

from tests import test_gpu_quant_fp8 as t8
from tests import test_gpu_quant_mxfp4 as t4

pytestmark = pytest.mark.gpu

FORMATS = ["fp8", "mxfp4"]
TILE = {"fp8": "wq_tile_gemm_w8", "mxfp4": "wq_tile_gemm_w4"}
SKINNY = {"fp8": "skinny_gemm_w8", "mxfp4": "skinny_gemm_w4"}
DEQUANT = {"fp8": "dequant_fp8_rows", "mxfp4": "dequant_mxfp4_rows"}
LINEAR = {"fp8": "linear_w8", "mxfp4": "linear_w4"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    return "cuda"


def _exact_weight(fmt, M, K):
    """(codes, scales, dequantized [M, K] f32, exact in bf16) on the CPU"""
    from kserve_amd.ops import quant

    if fmt == "fp8":
        q, scale = t8._all_codes_weight(M, K, row_step=37)
        want = q.float() * scale[:, None]
    else:
        q, scale = t4._all_codes_weight(M, K)  # scale codes in [115, 130]
        want = quant.dequantize_mxfp4(q, scale)
    assert torch.equal(want.bfloat16().float(), want)
    return q, scale, want


def _random_case(fmt, N, K, M, dev):
    return (t8._w8_case if fmt == "fp8" else t4._w4_case)(N, K, M, dev)


def _dequant64(fmt, q, scale):
    from kserve_amd.ops import quant

    if fmt == "fp8":
        return q.cpu().double() * scale.cpu().double()[:, None]
    return quant.dequantize_mxfp4(q.cpu(), scale.cpu()).double()


# -- 1: exact placement -------------------------------------------------------


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize(
    "N,M,steps",
    [
        (1, 64, 1),     # a lone clamped row, half feature tile, prologue only
        (129, 192, 2),  # full + 1-row tile, full + half tile, prologue + tail
        (300, 64, 3),   # three row tiles, ragged last, once round the loop
    ],
)
@pytest.mark.parametrize("n_splits", [1, 4])
def test_exact_placement(dev, fmt, N, M, steps, n_splits):
    """One-hot x: row n selects column (off + n) % K, so out[n][m] must be
    the dequantized w[m][(off + n) % K] bit for bit, for windows that cover
    all of K. K = steps * n_splits K steps of 64; every partial but one is
    zero, so a forced split stays exact. MXFP4 needs K % 128 == 0: an odd
    step count is rounded up there (n_splits = 1: 2, 2 and 4 steps)."""
    import kserve_amd_C

    K = steps * n_splits * 64
    if fmt == "mxfp4":
        K = -(-K // 128) * 128
    q, scale, want = _exact_weight(fmt, M, K)
    qd, sd, want = q.to(dev), scale.to(dev), want.to(dev)
    rows = torch.arange(N, device=dev)
    for off in range(0, K, N):
        cols = (off + rows) % K
        x = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
        x[rows, cols] = 1.0
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        getattr(kserve_amd_C, TILE[fmt])(out, x, qd, sd, None, n_splits)
        assert torch.equal(out.float(), want[:, cols].t()), f"window {off}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_placement_policy_split(dev, fmt):
    """n_splits = 0 on a weight the (M, K) policy itself splits"""
    import kserve_amd_C

    N, M, K = 129, 64, 512
    assert kserve_amd_C.wq_tile_nsplit(M, K) > 1
    q, scale, want = _exact_weight(fmt, M, K)
    rows = torch.arange(N, device=dev)
    for off in range(0, K, N):
        cols = (off + rows) % K
        x = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
        x[rows, cols] = 1.0
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        getattr(kserve_amd_C, TILE[fmt])(out, x, q.to(dev), scale.to(dev))
        assert torch.equal(out.float().cpu(), want[:, cols.cpu()].t())


# -- 2: numerics against fp64 -------------------------------------------------


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N,K,M", [(129, 256, 192), (300, 512, 64)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("n_splits", [1, 2])
def test_matches_fp64_reference(dev, fmt, N, K, M, with_bias, n_splits):
    """Allowance per element: one bf16 rounding of the result, 2^-8 |ref|,
    plus the f32 accumulation bound with a factor two of slack,
    K 2^-23 sum_k |x w|."""
    import kserve_amd_C

    K = K * 2 if fmt == "mxfp4" else K
    x, q, scale = _random_case(fmt, N, K, M, dev)
    bias = None
    if with_bias:
        gen = torch.Generator().manual_seed(1)
        bias = (torch.randn(M, generator=gen) / 8).to(torch.bfloat16).to(dev)
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    getattr(kserve_amd_C, TILE[fmt])(out, x, q, scale, bias, n_splits)
    x64, w64 = x.cpu().double(), _dequant64(fmt, q, scale)
    ref = x64 @ w64.t()
    if with_bias:
        ref = ref + bias.cpu().double()
    allow = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x64.abs() @ w64.abs().t())
    err = (out.cpu().double() - ref).abs()
    print(f"max err/allowance {float((err / allow).max()):.3f}")
    assert bool((err <= allow).all())


# -- 3: dispatch ---------------------------------------------------------------


def _spy(monkeypatch, fmt):
    """the _spy of the quant tests, counting the tile binding too"""
    from kserve_amd import ops

    calls = {TILE[fmt]: 0, SKINNY[fmt]: 0, DEQUANT[fmt]: 0}

    class Spy:
        def __getattr__(self, name):
            fn = getattr(ops._C, name)
            if name in calls:
                def wrapped(*a):
                    calls[name] += 1
                    return fn(*a)
                return wrapped
            return fn

    monkeypatch.setattr(ops, "_native", lambda op: Spy())
    return calls


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize(
    "N,M,tile,path",
    [
        (300, 128, True, TILE),
        (16, 128, True, SKINNY),
        (300, 96, True, DEQUANT),   # M % 64 != 0
        (None, 128, True, DEQUANT),  # N = WQ_TILE_MAX_TOKENS[fmt] + 1
        (300, 128, False, DEQUANT),
    ],
)
def test_linear_dispatch(dev, monkeypatch, fmt, N, M, tile, path):
    from kserve_amd import ops

    if N is None:
        if ops.WQ_TILE_MAX_TOKENS[fmt] == 0:
            pytest.skip("the tile kernel is off for this format")
        N = ops.WQ_TILE_MAX_TOKENS[fmt] + 1
    calls = _spy(monkeypatch, fmt)
    x, q, scale = _random_case(fmt, N, 128, M, dev)
    gen = torch.Generator().manual_seed(1)
    bias = (torch.randn(M, generator=gen) / 8).to(torch.bfloat16).to(dev)
    ref = t8._ref if fmt == "fp8" else t4._ref
    for b in (None, bias):
        got = getattr(ops, LINEAR[fmt])(x, q, scale, b, tile=tile)
        torch.testing.assert_close(
            got.float().cpu(), ref(x, q, scale, b), atol=0.05, rtol=0.05
        )
    assert calls[path[fmt]] >= 2, calls
    assert sum(calls.values()) == calls[path[fmt]], calls


@pytest.mark.parametrize("fmt", FORMATS)
def test_layer_dispatch(dev, monkeypatch, fmt):
    from kserve_amd.parallel.layers import ColumnParallelLinear

    calls = _spy(monkeypatch, fmt)
    layer = ColumnParallelLinear(128, 128, quantization=fmt).to(dev)
    layer.random_init_weight(0.1, torch.Generator(device=dev).manual_seed(0))
    x = torch.randn(300, 128, device=dev).to(torch.bfloat16)
    want = layer(x)
    dequants = calls[DEQUANT[fmt]]  # one per row chunk of the scratch
    assert calls[TILE[fmt]] == 0 and dequants >= 1, calls
    layer.quant_gemm = "tile"
    got = layer(x)
    assert calls[TILE[fmt]] == 1 and calls[DEQUANT[fmt]] == dequants, calls
    torch.testing.assert_close(got.float(), want.float(), atol=0.05, rtol=0.05)


# -- 4: hipGraph ---------------------------------------------------------------


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay_is_bit_equal(dev, fmt):
    import kserve_amd_C

    N, K, M = 129, 256, 192
    fn = getattr(kserve_amd_C, TILE[fmt])
    x, q, scale = _random_case(fmt, N, K, M, dev)
    eager = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    fn(eager, x, q, scale, None, 2)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn(out, x, q, scale, None, 2)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# -- 5: engine -----------------------------------------------------------------


@pytest.mark.parametrize("fmt", FORMATS)
def test_engine_prefill_runs_the_tile_kernel(dev, monkeypatch, fmt):
    """Tokens are not compared with the "dequant" engine: the two GEMMs sum
    in different orders and near-ties flip on a random model."""
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    cfg = t8._cfg(quantization=fmt)
    cfg.model.quant_gemm = "tile"
    engine = LLMEngine(cfg)
    calls = _spy(monkeypatch, fmt)
    prompt = [(7 * i + 3) % 2048 for i in range(300)]
    sp = SamplingParams(temperature=0.0, max_tokens=8)
    runs = []
    for _ in range(2):
        out = engine.generate([prompt], sp)
        runs.append([o.output_token_ids for o in out.values()])
    assert calls[TILE[fmt]] > 0 and calls[DEQUANT[fmt]] == 0, calls
    assert len(runs[0][0]) == 8 and runs[0] == runs[1]
