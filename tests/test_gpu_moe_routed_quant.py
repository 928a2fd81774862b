"""GPU: the routed MoE MLP with quantized experts (fp8, MXFP4; csrc/moe.hip)
against the fp64 pair-by-pair reference and derived allowance of
tests/test_gpu_moe_routed.py, called with the experts' codes dequantized
exactly in fp64 (fp8: q * scale; MXFP4: table value * 2^(s-127)). The converts
in the kernel are exact and the scales multiply in f32, which the
(H + I) 2^-23 term of that allowance covers, so there is no new tolerance.
(`reference` uses that module's H = 128 in this term for every H here: a
little stricter.) Nothing is compared with the weights before quantization.

Weights are N(0,1)/sqrt(fan_in) with every 32-wide K block of every row
scaled by a random power of two in 2^-2..2^2, so indexing mistakes move the
result. From the CPU reference alone (torch_ref, T=17 E=4 k=2 H=256, error
over allowance, median and share of elements above 1), at I=128 / I=1024:
MXFP4 scale byte of the neighbouring block 53x, 99% / 22x, 97%; MXFP4
nibbles of every byte swapped 50x, 99% / 20x, 98%; gate and up scales
exchanged, MXFP4 44x, 99% / 18x, 97%, fp8 2.4x, 79% / 1.0x, 51% (fp8 row
scales, absmax / 448, differ little between rows of one distribution).
"""

import functools

import pytest
import torch

from kserve_amd import ops
from kserve_amd.ops import quant
from tests.test_gpu_moe_routed import check, reference, routing

pytestmark = pytest.mark.gpu

QUANTS = ("fp8", "mxfp4")


def exact_dequant(q, codes, scale):
    if q == "fp8":
        return codes.double() * scale.double().unsqueeze(-1)
    flat = quant.dequantize_mxfp4(codes.flatten(0, 1), scale.flatten(0, 1))
    return flat.double().view(*codes.shape[:2], -1)  # f32 ldexp is exact


@functools.lru_cache(maxsize=None)
def experts(q, E, hidden, inter):
    """((codes, scale) of gate_up, of down) and their fp64 values, on GPU."""
    g = torch.Generator().manual_seed(E + hidden + inter)
    fmt = quant.WEIGHT_FORMATS[q]
    out = []
    for rows, cols in ((2 * inter, hidden), (hidden, inter)):
        w = torch.randn(E, rows, cols // 32, 32, generator=g) / cols ** 0.5
        w = w * 2.0 ** torch.randint(-2, 3, (E, rows, cols // 32, 1), generator=g)
        qs = [fmt.shard_to_codes(e.reshape(rows, cols), None, "cuda") for e in w]
        codes, scale = (torch.stack(t) for t in zip(*qs))
        out.append((codes, scale, exact_dequant(q, codes, scale)))
    return out


def inputs(T, hidden, mode, E=4, k=2, seed=0):
    x, topi, topw = routing(T, E, k, mode, seed)
    if hidden != x.shape[1]:
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(T, hidden, generator=g).bfloat16()
    return x.cuda(), topi.cuda(), topw.cuda()


def run(q, x, topi, topw, gu, dn, lo=0, sl=slice(None)):
    return ops.moe_routed_mlp(
        x, topi, topw, gu[0][sl].contiguous(), dn[0][sl].contiguous(), lo,
        gate_up_scale=gu[1][sl].contiguous(),
        down_scale=dn[1][sl].contiguous(), quantization=q,
    )


# (H / BK, I - i_bk * BK, i_bk, T): K loops of 1-4 steps; the K split, even
# and with a shorter last split; one tile, a ragged second, > 128 rows
SHAPES = [(1, 0, 1, 17), (2, 0, 1, 17), (3, 0, 1, 17), (4, 0, 1, 17),
          (2, 1024, 0, 17), (2, 1024, 1, 17), (2, 0, 1, 1), (2, 0, 1, 130)]


@pytest.mark.parametrize("q", QUANTS)
@pytest.mark.parametrize("h_bk,i_fix,i_bk,T", SHAPES)
def test_op_matches_reference(q, h_bk, i_fix, i_bk, T):
    BK = ops.MOE_ROUTED_K_STEP[q]
    hidden, inter = h_bk * BK, i_fix + i_bk * BK
    gu, dn = experts(q, 4, hidden, inter)
    for mode in ("uniform", "same"):
        x, topi, topw = inputs(T, hidden, mode)
        got = run(q, x, topi, topw, gu, dn)
        check(got, *reference(x, topi, topw, gu[2], dn[2]))
    if (h_bk, inter, T) != (2, BK, 17):
        return  # one expert-parallel case: experts 2, 3 local
    x, topi, topw = inputs(17, hidden, "remote0")
    got = run(q, x, topi, topw, gu, dn, lo=2, sl=slice(2, 4))
    check(got, *reference(x, topi, topw, gu[2][2:], dn[2][2:], expert_lo=2))
    assert not got[0].any(), "a token with no local expert must be 0"


@pytest.mark.parametrize("q", QUANTS)
def test_rows_permute_and_runs_repeat(q):
    BK = ops.MOE_ROUTED_K_STEP[q]
    gu, dn = experts(q, 4, 2 * BK, 1024 + BK)
    x, topi, topw = inputs(17, 2 * BK, "uniform")
    out = run(q, x, topi, topw, gu, dn)
    assert torch.equal(out, run(q, x, topi, topw, gu, dn))
    perm = torch.randperm(17, generator=torch.Generator().manual_seed(1)).cuda()
    out_p = run(q, x[perm].contiguous(), topi[perm].contiguous(),
                topw[perm].contiguous(), gu, dn)
    assert torch.equal(out_p, out[perm])


@pytest.mark.parametrize("q", QUANTS)
def test_one_capture_serves_any_routing(q):
    BK = ops.MOE_ROUTED_K_STEP[q]
    gu, dn = experts(q, 8, 2 * BK, 1024)
    x, topi, topw = inputs(17, 2 * BK, "same", E=8)
    run(q, x, topi, topw, gu, dn)  # load code before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(q, x, topi, topw, gu, dn)
    for seed in (5, 6, 7):  # experts that were empty at capture included
        nx, ni, nw = inputs(17, 2 * BK, "uniform", E=8, seed=seed)
        x.copy_(nx), topi.copy_(ni), topw.copy_(nw)
        graph.replay()
        assert ni.unique().numel() == 8
        assert torch.equal(out, run(q, x, topi, topw, gu, dn))
        check(out, *reference(x, topi, topw, gu[2], dn[2]))


def sparse_path_extra(x, topi, topw, w_gu, w_d):
    """Extra allowance of the per-expert fallback (T > 384), e = 2^-9: gate
    and up carry e (|gu| + |x| @ |w|^T) (bf16 GEMM output; fp8 weights
    rounded to bf16 in the dequant scratch), which passes through act =
    silu(g) u with |silu'| <= 1.1, plus e for silu_and_mul; down adds 5 e:
    dequantized weights, bf16 GEMM output, bf16 topw, product, bf16 sum."""
    e, inter = 2.0 ** -9, w_d.shape[2]
    extra = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for le in range(w_gu.shape[0]):
        t, j = (topi == le).nonzero(as_tuple=True)
        xa = x[t].double()
        gu = xa @ w_gu[le].t()
        d_gu = e * (gu.abs() + xa.abs() @ w_gu[le].abs().t())
        s, u = torch.nn.functional.silu(gu[:, :inter]), gu[:, inter:]
        d_g, d_u = d_gu[:, :inter], d_gu[:, inter:]
        d_act = 1.1 * d_g * (u.abs() + d_u) + s.abs() * d_u + e * (s * u).abs()
        rows = (d_act + 5 * e * (s * u).abs()) @ w_d[le].abs().t()
        extra.index_add_(0, t, rows * topw[t, j].double().unsqueeze(1))
    return extra


@pytest.mark.parametrize("q", QUANTS)
@pytest.mark.parametrize("T", [17, 400])  # routed kernel; sparse fallback
def test_module_matches_reference_of_its_weights(q, T):
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    cfg = ModelConfig(
        vocab_size=128, hidden_size=128, intermediate_size=1024, num_layers=1,
        num_heads=2, num_kv_heads=1, head_dim=64, num_local_experts=4,
        num_experts_per_tok=2, moe_kernel="routed", quantization=q,
    )
    moe = MixtralMoE(cfg, dtype=torch.bfloat16).cuda()
    gu, dn = experts(q, 4, 128, 1024)
    moe.w_gate_up.data.copy_(gu[0]), moe.w_gate_up_scale.data.copy_(gu[1])
    moe.w_down.data.copy_(dn[0]), moe.w_down_scale.data.copy_(dn[1])
    moe.gate.data.normal_(0, 1, generator=torch.Generator("cuda").manual_seed(2))
    ops.reserve_w8_scratch("cuda", 2048, 128)
    moe._forward_dense = None  # never reached with quantized experts
    x = inputs(T, 128, "uniform", seed=3)[0]
    got = moe(x)
    logits = torch.nn.functional.linear(x.float(), moe.gate.float())
    topw, topi = torch.softmax(logits, dim=-1).topk(2, dim=-1)
    topw = topw / topw.sum(dim=-1, keepdim=True)
    ref, allow = reference(x, topi, topw, gu[2], dn[2])
    if T > MixtralMoE.ROUTED_MAX_TOKENS:
        allow = allow + sparse_path_extra(x, topi, topw, gu[2], dn[2])
    check(got, ref, allow)


@pytest.mark.parametrize("q", QUANTS)
def test_engine_quantized_routed_graphs_match_eager_and_single(q):
    from kserve_amd.engine import config as C
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    torch.manual_seed(3)
    cfg = C.EngineConfig(  # test_engine_routed_graphs_match_eager_and_single's
        model=C.ModelConfig(
            vocab_size=2048, hidden_size=256, intermediate_size=512,
            num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128,
            max_position_embeddings=512, num_local_experts=4,
            num_experts_per_tok=2, moe_kernel="routed", quantization=q),
        cache=C.CacheConfig(block_size=16, num_gpu_blocks=64),
        scheduler=C.SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=1024, max_model_len=256),
        device="cuda", seed=0, eos_token_id=-1,
    )
    engine = LLMEngine(cfg)
    assert engine.runner._graphs, "routed MoE decode graphs must be captured"
    sp = SamplingParams(temperature=0.0, max_tokens=10)
    prompts = [[1, 2, 3], [9, 8, 7, 6]]
    out = [o.output_token_ids for o in engine.generate(prompts, sp).values()]
    single = engine.generate(prompts[:1], sp)
    assert list(single.values())[0].output_token_ids == out[0]
    del engine
    cfg.enforce_eager = True
    eager = LLMEngine(cfg).generate(prompts, sp)
    assert [o.output_token_ids for o in eager.values()] == out
