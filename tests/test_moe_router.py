"""CPU: the MoE router's config switch and its f32 reference
(torch_ref.moe_route) against an fp64 reference on inputs whose logits are
exact: x entries are integers in [-2, 2] and gate entries integers in [-2, 2]
times 2^-4, so every product and every partial sum is a multiple of 2^-4 far
below 2^24 of them and any summation order gives the same f32. A wrong index
then moves a logit by a multiple of 2^-4, and exact ties between the k-th and
(k+1)-th logit occur by themselves, so the tie rule (lowest expert id) is
exercised without being constructed."""

import functools

import pytest
import torch

from kserve_amd.engine.config import ModelConfig
from kserve_amd.ops import torch_ref

T_MAX = 130


@functools.lru_cache(maxsize=None)
def exact_inputs(H, E, T=T_MAX):
    g = torch.Generator().manual_seed(H + E)
    gate = torch.randint(-2, 3, (E, H), generator=g).double() / 16
    x = torch.randint(-2, 3, (T, H), generator=g).double()
    return x.bfloat16(), gate.bfloat16()


@functools.lru_cache(maxsize=None)
def reference(H, E, k, T=T_MAX):
    """fp64 router of exact_inputs: (topi, topw, rows with a boundary tie)."""
    x, gate = exact_inputs(H, E, T)
    logits = x.double() @ gate.double().t()
    srt, order = torch.sort(logits, dim=-1, descending=True, stable=True)
    p = torch.exp(srt[:, :k] - srt[:, :1])
    ties = (srt[:, k - 1] == srt[:, k]) if k < E else torch.zeros(T).bool()
    return order[:, :k], p / p.sum(-1, keepdim=True), ties


def test_moe_router_is_validated(monkeypatch):
    monkeypatch.delenv("KS_MOE_ROUTER", raising=False)
    assert ModelConfig().moe_router == "torch"
    assert ModelConfig(moe_router="fused").moe_router == "fused"
    with pytest.raises(ValueError):
        ModelConfig(moe_router="bogus")
    monkeypatch.setenv("KS_MOE_ROUTER", "fused")
    assert ModelConfig().moe_router == "fused"


@pytest.mark.parametrize("E,k", [(4, 1), (4, 2), (8, 2), (8, 8), (60, 8), (256, 8)])
@pytest.mark.parametrize("H", [128, 640])
def test_torch_ref_matches_fp64_on_exact_inputs(H, E, k):
    x, gate = exact_inputs(H, E)
    ref_i, ref_w, ties = reference(H, E, k)
    topi, topw = torch_ref.moe_route(x, gate, k)
    assert topi.dtype == torch.int64 and topw.dtype == torch.float32
    err = ((topw.double() - ref_w).abs() / ref_w).max().item()
    print(f"boundary ties in {int(ties.sum())}/{T_MAX} rows, "
          f"max rel err {err:.3g}")
    assert torch.equal(topi, ref_i)
    assert err <= 2.0 ** -16


def test_torch_ref_reproduces_the_module_router():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T_MAX, 256, generator=g).bfloat16()
    gate = torch.randn(8, 256, generator=g).bfloat16()
    # MixtralMoE.forward's four lines
    logits = torch.nn.functional.linear(x.float(), gate.float())
    probs = torch.softmax(logits, dim=-1)
    w, i = probs.topk(2, dim=-1)
    w = w / w.sum(dim=-1, keepdim=True)
    topi, topw = torch_ref.moe_route(x, gate, 2)
    same = (topi == i).all(-1)
    print(f"rows that disagree on ids: {int((~same).sum())}")
    assert bool(same.all())
    assert bool(((topw - w).abs() <= 2.0 ** -20 * w)[same].all())
