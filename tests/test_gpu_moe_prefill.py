"""GPU: the routed MoE prefill MLP (ops.moe_routed_prefill_mlp, csrc/
moe_prefill.hip) against the fp64 reference and the derived elementwise
allowance of tests/test_gpu_moe_routed.py,
    2^-8 |ref| + (2^-8 + (H + I) 2^-23) sum_j topw_j (|act_j| @ |w_down|^T),
which holds for any f32-accumulating kernel. The helpers below are that
file's with H as a parameter.

Shapes (H, I) = (128, 64) and (256, 192): 2 and 4 K steps in gate/up, 1 and 3
in down, 1 and 3 feature blocks in gate/up, 1 and 2 in down. Under "same"
routing k experts hold every row and the others none: T = 127 is one ragged
tile, 129 an exactly full tile and a tile of one row, 385 and up several
tiles per expert. 1100 x 2 pairs cross the 1024-pair align blocks, and
chunk + 1 tokens the wrapper's chunk.

Margin (test_allowance_tells_a_swapped_expert, CPU): at T = 129, E = 4,
k = 2 the f32 reference stays inside the allowance everywhere, and with two
experts' weights swapped it misses on most elements of the rows that use
them.
"""

import copy
import functools

import pytest
import torch

from kserve_amd import ops
from kserve_amd.ops import torch_ref
from tests.test_gpu_moe_routed import check

SHAPES = [(128, 64), (256, 192)]
CHUNK = ops.MOE_PREFILL_CHUNK_TOKENS


@functools.lru_cache(maxsize=None)
def weights(E, H, inter, device="cuda"):
    g = torch.Generator().manual_seed(100 * E + inter)
    w_gu = torch.randn(E, 2 * inter, H, generator=g) / H ** 0.5
    w_d = torch.randn(E, H, inter, generator=g) / inter ** 0.5
    return w_gu.bfloat16().to(device), w_d.bfloat16().to(device)


def routing(T, E, k, H, mode, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).bfloat16()
    topw, topi = torch.softmax(torch.randn(T, E, generator=g), -1).topk(k, -1)
    if mode == "same":  # one expert set holds every row, the others are empty
        topi = topi[:1].expand(T, k).contiguous()
    if mode == "remote0":  # token 0 routed only below the EP slice
        topi[0] = torch.arange(k)
    return x, topi, (topw / topw.sum(-1, keepdim=True)).float()


def reference(x, topi, topw, w_gu, w_d, expert_lo=0):
    """fp64 result and the elementwise allowance (module docstring)."""
    H, inter = w_d.shape[1], w_d.shape[2]
    ref = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    bound = torch.zeros_like(ref)
    for le in range(w_gu.shape[0]):
        t, j = (topi == expert_lo + le).nonzero(as_tuple=True)
        gu = x[t].double() @ w_gu[le].double().t()
        act = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        act = act.bfloat16().double()
        w = topw[t, j].double().unsqueeze(1)
        ref.index_add_(0, t, act @ w_d[le].double().t() * w)
        bound.index_add_(0, t, act.abs() @ w_d[le].double().abs().t() * w)
    eps = 2.0 ** -8
    return ref, eps * ref.abs() + (eps + (H + inter) * 2.0 ** -23) * bound


@pytest.mark.parametrize("H,inter", SHAPES)
def test_allowance_tells_a_swapped_expert(H, inter):
    w_gu, w_d = weights(4, H, inter, "cpu")
    x, topi, topw = routing(129, 4, 2, H, "uniform")
    ref, allow = reference(x, topi, topw, w_gu, w_d)
    good = torch_ref.moe_routed_mlp(x, topi, topw, w_gu, w_d)
    assert bool(((good.double() - ref).abs() <= allow).all())
    swap = [1, 0, 2, 3]
    bad = torch_ref.moe_routed_mlp(x, topi, topw, w_gu[swap], w_d[swap])
    moved = topi.lt(2).any(-1)  # rows that use a swapped expert
    miss = (bad.double() - ref).abs()[moved] > allow[moved]
    print(f"H={H} I={inter}: missing {miss.double().mean().item():.3f}")
    assert miss.double().mean() > 0.5  # "most elements"


@pytest.mark.gpu
@pytest.mark.parametrize("H,inter", SHAPES)
@pytest.mark.parametrize("E,k", [(4, 2), (8, 2), (4, 1)])
@pytest.mark.parametrize("T", [1, 127, 129, 385, 1100, CHUNK + 1])
def test_op_matches_reference(T, E, k, H, inter):
    w_gu, w_d = weights(E, H, inter)
    for mode in ("uniform", "same"):
        x, topi, topw = (a.cuda() for a in routing(T, E, k, H, mode))
        got = ops.moe_routed_prefill_mlp(x, topi, topw, w_gu, w_d)
        check(got, *reference(x, topi, topw, w_gu, w_d))
    if E == 4:  # EP slice: experts 2, 3 local, pairs of 0, 1 dropped
        x, topi, topw = (a.cuda() for a in routing(T, E, k, H, "remote0"))
        lo_gu, lo_d = w_gu[2:].contiguous(), w_d[2:].contiguous()
        got = ops.moe_routed_prefill_mlp(x, topi, topw, lo_gu, lo_d, expert_lo=2)
        check(got, *reference(x, topi, topw, lo_gu, lo_d, expert_lo=2))
        assert not got[0].any(), "a token with no local expert must be 0"


@pytest.mark.gpu
def test_rows_are_independent_and_runs_repeat():
    H, inter = SHAPES[1]
    w_gu, w_d = weights(4, H, inter)
    x, topi, topw = (a.cuda() for a in routing(385, 4, 2, H, "uniform"))
    out = ops.moe_routed_prefill_mlp(x, topi, topw, w_gu, w_d)
    assert torch.equal(out, ops.moe_routed_prefill_mlp(x, topi, topw, w_gu, w_d))
    perm = torch.randperm(385, generator=torch.Generator().manual_seed(1)).cuda()
    out_p = ops.moe_routed_prefill_mlp(
        x[perm].contiguous(), topi[perm].contiguous(),
        topw[perm].contiguous(), w_gu, w_d,
    )
    assert torch.equal(out_p, out[perm])


@pytest.mark.gpu
def test_module_routed_prefill_matches_its_sparse_path():
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    H, inter = SHAPES[1]
    cfg = ModelConfig(
        vocab_size=128, hidden_size=H, intermediate_size=inter,
        num_layers=1, num_heads=2, num_kv_heads=1, head_dim=64,
        num_local_experts=4, num_experts_per_tok=2, moe_kernel="routed",
    )
    moe = MixtralMoE(cfg, dtype=torch.bfloat16)
    w_gu, w_d = weights(4, H, inter, "cpu")
    moe.w_gate_up.data.copy_(w_gu), moe.w_down.data.copy_(w_d)
    moe.gate.data.normal_(0, 1, generator=torch.Generator().manual_seed(2))
    x, _, _ = routing(400, 4, 2, H, "uniform")
    gpu = copy.deepcopy(moe).cuda()
    gpu._forward_sparse = None  # the prefill kernels must not need either
    gpu._forward_dense = None
    got = gpu(x.cuda()).cpu()
    # forward()'s router, then the module's own sparse loop in fp64
    logits = torch.nn.functional.linear(x.cuda().float(), gpu.gate.float())
    topw, topi = torch.softmax(logits, dim=-1).topk(2, dim=-1)
    topw, topi = (topw / topw.sum(dim=-1, keepdim=True)).cpu(), topi.cpu()
    sparse = moe.double()._forward_sparse(x.double(), topi, topw.double())
    _, allow = reference(x, topi, topw, w_gu, w_d)
    check(got, sparse, allow)
