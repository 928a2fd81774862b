"""CPU: quantized (fp8, MXFP4) experts of MixtralMoE: loading, the
construction-time refusals, the CPU forward and random_init."""

import pytest
import torch

from kserve_amd import ops
from kserve_amd.engine.config import ModelConfig
from kserve_amd.models.llama import LlamaForCausalLM
from kserve_amd.ops import quant
from tests.test_gpu_moe_routed import reference

QUANTS = ("fp8", "mxfp4")
H, I, E = 128, 256, 4
L0 = "model.layers.0."
EXPERT = L0 + "block_sparse_moe.experts.{}.{}"


def config(q, **kw):
    kw = {"moe_kernel": "routed", "hidden_size": H, "intermediate_size": I,
          "num_local_experts": E, "num_experts_per_tok": 2, **kw}
    return ModelConfig(
        vocab_size=64, num_layers=1, num_heads=2, num_kv_heads=1, head_dim=64,
        quantization=q, **kw,
    )


def checkpoint(q=None):
    """Classic-layout Mixtral tensors; with ``q`` the expert projections are
    that format's codes (fp8: one per-tensor scale on w1, per-channel else)."""
    g = torch.Generator().manual_seed(0)
    shapes = {"model.embed_tokens": (64, H), L0 + "block_sparse_moe.gate": (E, H)}
    for n, rows in (("q", H), ("k", 64), ("v", 64), ("o", H)):
        shapes[L0 + f"self_attn.{n}_proj"] = (rows, H)
    for j in range(E):
        for n, s in (("w1", (I, H)), ("w3", (I, H)), ("w2", (H, I))):
            shapes[EXPERT.format(j, n)] = s
    t = {k + ".weight": (torch.randn(*s, generator=g) / s[1] ** 0.5).bfloat16()
         for k, s in shapes.items()}
    for n in ("model.norm", L0 + "input_layernorm", L0 + "post_attention_layernorm"):
        t[n + ".weight"] = torch.ones(H)
    for k in [k[:-7] for k in t if ".experts." in k and q]:
        w = t[k + ".weight"]
        codes, s = quant.WEIGHT_FORMATS[q].shard_to_codes(w, None, "cpu")
        if q == "fp8" and k.endswith("w1"):
            s = s.max().reshape(1)
            codes = (w.float() / s).clamp(-448, 448).to(quant.FP8_DTYPE)
        t[k + ".weight"], t[k + ".weight_scale"] = codes, s
    return t


def load(q, t):
    model = LlamaForCausalLM(config(q))
    model.load_hf_state_dict(t)
    return model.layers[0].mlp


def projections(moe):
    """(checkpoint name, codes, scales) of every expert projection."""
    for j in range(E):
        yield EXPERT.format(j, "w1"), moe.w_gate_up[j, :I], moe.w_gate_up_scale[j, :I]
        yield EXPERT.format(j, "w3"), moe.w_gate_up[j, I:], moe.w_gate_up_scale[j, I:]
        yield EXPERT.format(j, "w2"), moe.w_down[j], moe.w_down_scale[j]


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("q", QUANTS)
def test_load_hf_state_dict_stores_codes_and_scales(q, pre):
    """bf16 experts come out as shard_to_codes of the weights; pre-quantized
    ones round-trip, refuse the other format's model, and dequantize with
    their scales into an unquantized model."""
    t, fmt = checkpoint(q if pre else None), quant.WEIGHT_FORMATS[q]
    for name, codes, scales in projections(load(q, t)):
        want, ws = t[name + ".weight"], t.get(name + ".weight_scale")
        if not pre:
            want, ws = fmt.shard_to_codes(want, None, "cpu")
        elif q == "fp8":
            ws = quant.expand_scale(ws, want.shape[0])
        assert torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
        assert torch.equal(scales, ws)
    if pre:
        with pytest.raises(ValueError, match="cannot be loaded"):
            load("mxfp4" if q == "fp8" else "fp8", t)
        assert torch.equal(  # the last projection: expert E-1's w2
            load(None, t).w_down[E - 1], fmt.dequantize(want, ws, torch.bfloat16)
        )


@pytest.mark.parametrize("q", QUANTS)
def test_construction_refusals(q):
    with pytest.raises(ValueError, match="mixture-of-experts"):
        LlamaForCausalLM(config(q, moe_kernel="dense"))
    step = ops.MOE_ROUTED_K_STEP[q]
    for bad in ({"intermediate_size": I + 64}, {"hidden_size": H + 64}):
        with pytest.raises(ValueError, match=f"multiples of {step}"):
            LlamaForCausalLM(config(q, **bad))
    with pytest.raises(ValueError, match="experts per token"):
        LlamaForCausalLM(config(q, num_local_experts=16, num_experts_per_tok=9))


@pytest.mark.parametrize("q", QUANTS)
def test_cpu_forward_matches_reference_on_dequantized_weights(q):
    moe, fmt = load(q, checkpoint()), quant.WEIGHT_FORMATS[q]
    w_gu = torch.stack([fmt.dequantize(moe.w_gate_up[j], moe.w_gate_up_scale[j])
                        for j in range(E)])
    w_d = torch.stack([fmt.dequantize(moe.w_down[j], moe.w_down_scale[j])
                       for j in range(E)])
    x = torch.randn(17, H, generator=torch.Generator().manual_seed(1)).bfloat16()
    probs = torch.softmax(x.float() @ moe.gate.float().t(), dim=-1)
    topw, topi = probs.topk(2, dim=-1)
    topw = topw / topw.sum(dim=-1, keepdim=True)
    ref, allow = reference(x, topi, topw, w_gu, w_d)  # its H is ours
    assert bool(((moe(x).double() - ref).abs() <= allow).all())
    same = ops.moe_routed_mlp(
        x, topi, topw, moe.w_gate_up, moe.w_down,
        gate_up_scale=moe.w_gate_up_scale, down_scale=moe.w_down_scale,
        quantization=q,
    )
    assert bool(((same.double() - ref).abs() <= allow).all())


def test_random_init_of_unquantized_moe_is_unchanged():
    """The unquantized draw is parameter by parameter in parameters() order,
    as it was before quantized experts existed."""
    a = LlamaForCausalLM(config(None)).random_init(seed=5)
    b = LlamaForCausalLM(config(None)).random_init(seed=5)
    gen = torch.Generator().manual_seed(5)
    for p, r in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, r)
        if p.dim() >= 2:
            want = torch.empty_like(p).normal_(0.0, 0.02, generator=gen)
            assert torch.equal(p, want)
