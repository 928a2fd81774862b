"""GPU: the routed MoE prefill MLP with quantized experts (fp8, MXFP4;
ops.moe_routed_prefill_mlp, csrc/moe_prefill.hip) against the fp64 result of
the exactly dequantized codes and the derived allowance of
tests/test_gpu_moe_prefill.py. The converts in the kernel are exact and the
fp8 scale is one f32 multiply, which the (H + I) 2^-23 term covers: there is
no new tolerance. Experts are those of tests/test_gpu_moe_routed_quant.py
(every 32-wide K block scaled by its own power of two).

Shapes (H, I) = (128, 64) and (256, 192): 2 and 4 K steps in gate/up, 1 and 3
in down; for MXFP4 4 and 8 scale blocks per gate/up row, 2 and 6 per down row
(I = 192 makes a down row's scale bytes start on both halves of a dword).
T = 127 is one ragged tile under "same" routing, 129 a full tile and a tile of
one row, 385 several tiles per expert.

Margin, CPU (torch_ref on these inputs, both formats and shapes, T in
{129, 385}): the f32 reference reaches at most 0.42 of the allowance; with the
down scales rolled by one position 93 to 98 % of the elements miss it.
Measured max err / allowance on an MI355X: profiles/moe_routed.md,
"Quantized prefill".
"""

import pytest
import torch

from kserve_amd import ops
from tests.test_gpu_moe_prefill import SHAPES, check, reference, routing
from tests.test_gpu_moe_routed_quant import QUANTS, experts

pytestmark = pytest.mark.gpu


def run(q, x, topi, topw, gu, dn, lo=0, sl=slice(None)):
    return ops.moe_routed_prefill_mlp(
        x, topi, topw, gu[0][sl].contiguous(), dn[0][sl].contiguous(), lo,
        gate_up_scale=gu[1][sl].contiguous(),
        down_scale=dn[1][sl].contiguous(), quantization=q,
    )


@pytest.mark.parametrize("q", QUANTS)
@pytest.mark.parametrize("H,inter", SHAPES)
@pytest.mark.parametrize("T", [1, 127, 129, 385])
def test_op_matches_reference(q, T, H, inter):
    gu, dn = experts(q, 4, H, inter)
    for mode in ("uniform", "same"):
        x, topi, topw = (a.cuda() for a in routing(T, 4, 2, H, mode))
        got = run(q, x, topi, topw, gu, dn)
        check(got, *reference(x, topi, topw, gu[2], dn[2]))


@pytest.mark.parametrize("q", QUANTS)
def test_expert_parallel_slice(q):
    H, inter = SHAPES[1]
    gu, dn = experts(q, 4, H, inter)  # experts 2, 3 local
    x, topi, topw = (a.cuda() for a in routing(129, 4, 2, H, "remote0"))
    got = run(q, x, topi, topw, gu, dn, lo=2, sl=slice(2, 4))
    check(got, *reference(x, topi, topw, gu[2][2:], dn[2][2:], expert_lo=2))
    assert not got[0].any(), "a token with no local expert must be 0"


@pytest.mark.parametrize("q", QUANTS)
def test_scales_cross_the_wrapper_chunks(q):
    H, inter = SHAPES[0]
    gu, dn = experts(q, 4, H, inter)
    T = ops.MOE_PREFILL_CHUNK_TOKENS + 1
    x, topi, topw = (a.cuda() for a in routing(T, 4, 2, H, "uniform"))
    got = run(q, x, topi, topw, gu, dn)
    check(got, *reference(x, topi, topw, gu[2], dn[2]))


@pytest.mark.parametrize("q", QUANTS)
def test_rows_permute_and_runs_repeat(q):
    H, inter = SHAPES[1]
    gu, dn = experts(q, 4, H, inter)
    x, topi, topw = (a.cuda() for a in routing(385, 4, 2, H, "uniform"))
    out = run(q, x, topi, topw, gu, dn)
    assert torch.equal(out, run(q, x, topi, topw, gu, dn))
    perm = torch.randperm(385, generator=torch.Generator().manual_seed(1)).cuda()
    out_p = run(q, x[perm].contiguous(), topi[perm].contiguous(),
                topw[perm].contiguous(), gu, dn)
    assert torch.equal(out_p, out[perm])


@pytest.mark.parametrize("q", QUANTS)
def test_module_prefill_needs_no_sparse_loop(q):
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
    moe._forward_sparse = None  # T = 400 must run the prefill kernels
    moe._forward_dense = None
    x = routing(400, 4, 2, 128, "uniform", seed=3)[0].cuda()
    got = moe(x)
    logits = torch.nn.functional.linear(x.float(), moe.gate.float())
    topw, topi = torch.softmax(logits, dim=-1).topk(2, dim=-1)
    topw = topw / topw.sum(dim=-1, keepdim=True)
    check(got, *reference(x, topi, topw, gu[2], dn[2]))  # no sparse_path_extra
