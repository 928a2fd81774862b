"""GPU: the fused MoE router (ops.moe_route, csrc/moe_router.hip) against the
fp64 reference of tests/test_moe_router.py on its exact-logit inputs: ids
equal in every row, weights within 2^-16 relative.

Where 2^-16 comes from: the logits are exact, their span within a row is at
most about 23, so the f32 exponent argument (l - m) * log2(e) is off by at
most about 33 * 2^-24 and exp by a relative 2^-19; exp itself, the sum of at
most 8 terms and the divide add a few ulp. 2^-16 leaves about 8x over that,
and a wrongly included expert moves a weight by O(1). Measured on an MI355X:
profiles/moe_routed.md, "Router".
"""

import copy

import pytest
import torch

from kserve_amd import ops
from tests.test_gpu_moe_routed import I_SPLIT, check, reference as mlp_reference
from tests.test_gpu_moe_routed import routing, weights
from tests.test_moe_router import exact_inputs, reference

pytestmark = pytest.mark.gpu


def check_router(H, E, k, T, T_gen):
    x, gate = (a.cuda() for a in exact_inputs(H, E, T_gen))
    ref_i, ref_w, ties = (a[:T] for a in reference(H, E, k, T_gen))
    topi, topw = ops.moe_route(x[:T].contiguous(), gate, k)
    assert topi.dtype == torch.int64 and topw.dtype == torch.float32
    err = ((topw.cpu().double() - ref_w).abs() / ref_w).max().item()
    print(f"boundary ties in {int(ties.sum())}/{T} rows, max rel err {err:.3g}")
    assert torch.equal(topi.cpu(), ref_i)
    assert err <= 2.0 ** -16


# H: one K step per wave, then a loop with an odd trip count; E: below one
# 16-expert block, no multiple of 16, every kernel instantiation's widest use;
# T: one row, ragged / full / two tiles, several workgroups
@pytest.mark.parametrize("T", [1, 15, 16, 17, 130])
@pytest.mark.parametrize("E,k", [(4, 1), (4, 2), (8, 2), (8, 8), (60, 8), (256, 8)])
@pytest.mark.parametrize("H", [128, 640])
def test_op_matches_fp64_reference(H, E, k, T):
    check_router(H, E, k, T, 130)


def test_large_grid_matches_fp64_reference():
    check_router(128, 8, 2, 4099, 4099)


# H = 4128 is 129 K chunks: with 8 waves and 8-step load groups (E <= 16)
# wave 0 has 17 steps, so the group loop runs twice before a ragged last group
@pytest.mark.parametrize("E,k", [(8, 2), (32, 8)])
def test_long_rows_match_fp64_reference(E, k):
    check_router(4128, E, k, 17, 17)


def random_inputs(T, H, E, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).bfloat16()
    return x, torch.randn(E, H, generator=g).bfloat16()


def test_rows_are_independent_and_runs_repeat():
    x, gate = (a.cuda() for a in random_inputs(130, 640, 8, 1))
    topi, topw = ops.moe_route(x, gate, 2)
    again = ops.moe_route(x, gate, 2)
    assert torch.equal(topi, again[0]) and torch.equal(topw, again[1])
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(2)).cuda()
    pi, pw = ops.moe_route(x[perm].contiguous(), gate, 2)
    assert torch.equal(pi, topi[perm]) and torch.equal(pw, topw[perm])
    alone = [ops.moe_route(x[t:t + 1], gate, 2) for t in range(130)]
    assert torch.equal(torch.cat([a[0] for a in alone]), topi)
    assert torch.equal(torch.cat([a[1] for a in alone]), topw)


def test_one_capture_serves_any_input():
    x, gate = (a.cuda() for a in random_inputs(17, 640, 8, 3))
    ops.moe_route(x, gate, 2)  # load code before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        topi, topw = ops.moe_route(x, gate, 2)
    for seed in (5, 6, 7):
        nx, ng = random_inputs(17, 640, 8, seed)
        x.copy_(nx), gate.copy_(ng)
        graph.replay()
        ei, ew = ops.moe_route(x, gate, 2)
        assert torch.equal(topi, ei) and torch.equal(topw, ew)


def test_module_fused_router_feeds_the_routed_kernels(monkeypatch):
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    cfg = ModelConfig(
        vocab_size=128, hidden_size=128, intermediate_size=I_SPLIT,
        num_layers=1, num_heads=2, num_kv_heads=1, head_dim=64,
        num_local_experts=4, num_experts_per_tok=2, moe_kernel="routed",
        moe_router="fused",
    )
    moe = MixtralMoE(cfg, dtype=torch.bfloat16)
    w_gu, w_d = weights(4, I_SPLIT, "cpu")
    moe.w_gate_up.data.copy_(w_gu), moe.w_down.data.copy_(w_d)
    moe.gate.data.normal_(0, 1, generator=torch.Generator().manual_seed(2))
    x, _, _ = routing(17, 4, 2, "uniform")
    gpu = copy.deepcopy(moe).cuda()
    topi, topw = ops.moe_route(x.cuda(), gpu.gate, 2)

    def no_torch_router(*args, **kwargs):
        raise AssertionError("the torch router ran")

    monkeypatch.setattr(torch, "softmax", no_torch_router)
    monkeypatch.setattr(torch.Tensor, "topk", no_torch_router)
    got = gpu(x.cuda())
    monkeypatch.undo()
    ref, allow = mlp_reference(x, topi.cpu(), topw.cpu(), w_gu, w_d)
    check(got.cpu(), ref, allow)


def test_engine_fused_router_graphs_match_eager_and_single():
    from kserve_amd.engine.config import (
        CacheConfig, EngineConfig, ModelConfig, SchedulerConfig,
    )
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    torch.manual_seed(3)
    cfg = EngineConfig(
        model=ModelConfig(
            vocab_size=2048, hidden_size=256, intermediate_size=512,
            num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128,
            max_position_embeddings=512, num_local_experts=4,
            num_experts_per_tok=2, model_name="moe-gpu-tiny",
            moe_kernel="routed", moe_router="fused",
        ),
        cache=CacheConfig(block_size=16, num_gpu_blocks=64),
        scheduler=SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=1024, max_model_len=256
        ),
        device="cuda", seed=0, eos_token_id=-1,
    )
    engine = LLMEngine(cfg)
    assert engine.runner._graphs, "decode graphs must be captured"
    sp = SamplingParams(temperature=0.0, max_tokens=10)
    prompts = [[1, 2, 3], [9, 8, 7, 6]]
    out = [o.output_token_ids for o in engine.generate(prompts, sp).values()]
    single = engine.generate(prompts[:1], sp)
    assert list(single.values())[0].output_token_ids == out[0]
    del engine
    torch.cuda.empty_cache()
    cfg.enforce_eager = True
    eager = LLMEngine(cfg).generate(prompts, sp)
    assert [o.output_token_ids for o in eager.values()] == out
