"""ModelConfig.ctx_attn, --ctx-attn, and the kernel / splits keywords of
ops.context_attention_varlen on the CPU, where they are ignored."""

import pytest
import torch

from kserve_amd import ops
from kserve_amd.engine.config import ModelConfig
from kserve_amd.ops import torch_ref
from tests import attention_cases as ac


def test_ctx_attn_is_validated(monkeypatch):
    monkeypatch.delenv("KS_CTX_ATTN", raising=False)
    assert ModelConfig().ctx_attn == "tiled"
    assert ModelConfig(ctx_attn="packed").ctx_attn == "packed"
    with pytest.raises(ValueError):
        ModelConfig(ctx_attn="bogus")
    monkeypatch.setenv("KS_CTX_ATTN", "packed")
    assert ModelConfig().ctx_attn == "packed"


def test_parser_takes_ctx_attn():
    from kserve_amd.runtimes.huggingfaceserver import build_parser

    parser = build_parser()
    assert parser.parse_args(["--ctx-attn", "packed"]).ctx_attn == "packed"
    assert parser.parse_args([]).ctx_attn is None
    with pytest.raises(SystemExit):
        parser.parse_args(["--ctx-attn", "ring"])


def test_kernel_is_ignored_on_cpu():
    inp = ac.build(ac.CASES_BY_NAME["ctx_kv2g4_w16"])
    args = (inp.q, inp.k_cache, inp.v_cache, inp.block_tables,
            inp.cu_seqlens_q, inp.context_lens)
    ref = torch_ref.context_attention_varlen(*args, inp.scale, window=16)
    got = ops.context_attention_varlen(*args, inp.max_q_len, inp.scale,
                                       window=16, kernel="packed", splits=3)
    assert torch.equal(got, ref)
    with pytest.raises(ValueError):
        ops.context_attention_varlen(*args, inp.max_q_len, inp.scale,
                                     kernel="ring")
    assert ops.context_packed_supported(16, 32, 8, 128)
    assert not ops.context_packed_supported(17, 32, 8, 128)
    assert not ops.context_packed_supported(4, 32, 8, 96)
    assert ops.CTX_PACKED_MAX_ROWS == 64
