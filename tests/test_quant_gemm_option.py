"""ModelConfig.quant_gemm and the tile keyword of ops.linear_w8 / linear_w4 on
the CPU, where it is ignored."""

import pytest
import torch

from kserve_amd import ops
from kserve_amd.engine.config import ModelConfig
from kserve_amd.ops import quant


def test_quant_gemm_is_validated(monkeypatch):
    monkeypatch.delenv("KS_QUANT_GEMM", raising=False)
    assert ModelConfig().quant_gemm == "dequant"
    assert ModelConfig(quant_gemm="tile").quant_gemm == "tile"
    with pytest.raises(ValueError):
        ModelConfig(quant_gemm="bogus")
    monkeypatch.setenv("KS_QUANT_GEMM", "tile")
    assert ModelConfig().quant_gemm == "tile"


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_tile_is_ignored_on_cpu(fmt):
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(130, 128, generator=gen)
    w = torch.randn(64, 128, generator=gen) / 8
    if fmt == "fp8":
        linear, (q, scale) = ops.linear_w8, quant.quantize_fp8_per_channel(w)
    else:
        linear, (q, scale) = ops.linear_w4, quant.quantize_mxfp4(w)
    assert torch.equal(
        linear(x, q, scale, tile=True), linear(x, q, scale, tile=False)
    )


def test_model_sets_quant_gemm_on_its_layers():
    from kserve_amd.models.llama import LlamaForCausalLM

    cfg = ModelConfig.tiny()
    cfg.quantization = "fp8"
    cfg.quant_gemm = "tile"
    model = LlamaForCausalLM(cfg)
    assert model.layers[0].mlp.down_proj.quant_gemm == "tile"
    assert model.layers[0].self_attn.qkv_proj.quant_gemm == "tile"
