"""CPU: the routed MoE reference and its config switch."""

import pytest
import torch

from kserve_amd.engine.config import ModelConfig
from kserve_amd.ops import torch_ref


@pytest.mark.parametrize("expert_lo,e_local", [(0, 4), (2, 2)])
def test_reference_equals_sparse_loop(expert_lo, e_local):
    from kserve_amd.models.llama import MixtralMoE

    cfg = ModelConfig(
        vocab_size=128, hidden_size=64, intermediate_size=96, num_layers=1,
        num_heads=2, num_kv_heads=1, head_dim=32, num_local_experts=4,
        num_experts_per_tok=2,
    )
    torch.manual_seed(3)
    moe = MixtralMoE(cfg, dtype=torch.float32)
    for p in moe.parameters():
        p.data.normal_(0, 0.1)
    # the EP slice: this rank holds experts [expert_lo, expert_lo + e_local)
    moe.expert_lo, moe.experts_per_rank = expert_lo, e_local
    moe.w_gate_up.data = moe.w_gate_up.data[expert_lo:expert_lo + e_local]
    moe.w_down.data = moe.w_down.data[expert_lo:expert_lo + e_local]
    x = torch.randn(12, 64)
    topw, topi = torch.softmax(x @ moe.gate.t(), -1).topk(2, dim=-1)
    got = torch_ref.moe_routed_mlp(
        x, topi, topw, moe.w_gate_up, moe.w_down, expert_lo
    )
    torch.testing.assert_close(
        got, moe._forward_sparse(x, topi, topw), atol=1e-6, rtol=1e-5
    )


def test_moe_kernel_is_validated(monkeypatch):
    monkeypatch.delenv("KS_MOE_KERNEL", raising=False)
    assert ModelConfig().moe_kernel == "dense"
    assert ModelConfig(moe_kernel="routed").moe_kernel == "routed"
    with pytest.raises(ValueError):
        ModelConfig(moe_kernel="bogus")
    monkeypatch.setenv("KS_MOE_KERNEL", "routed")
    assert ModelConfig().moe_kernel == "routed"
