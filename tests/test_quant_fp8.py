"""Weight-only fp8 (E4M3, W8A16) quantization: format, quantizer, layer
plumbing, checkpoint loading, TP sharding, CLI and LoRA — all on CPU, where
``ops.linear_w8`` is the fp32 reference the HIP kernel is tested against
(tests/test_gpu_quant_fp8.py)."""

import json
import multiprocessing as mp
import os
import subprocess
import sys
import types

import pytest
import torch

from kserve_amd import ops
from kserve_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    ModelConfig,
    SchedulerConfig,
)
from kserve_amd.models.llama import AttentionMetadata, LlamaForCausalLM
from kserve_amd.ops import quant, torch_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn
# the 254 finite e4m3fn codes (0x7F / 0xFF are the two NaNs)
FINITE_CODES = torch.tensor(
    [c for c in range(256) if c not in (0x7F, 0xFF)], dtype=torch.uint8
)


def representable(M, K, gen):
    """W = Q * 2^-k_row with Q drawn from the finite codes and +-448 in
    every row, k_row in [4, 12): exactly representable, so quantization
    must be lossless (scale == 2^-k, codes == Q). Exact in bf16 too."""
    codes = FINITE_CODES[torch.randint(0, 254, (M, K), generator=gen)]
    codes[:, 0] = 0x7E  # +448
    codes[:, 1] = 0xFE  # -448
    k = torch.randint(4, 12, (M,), generator=gen)
    scale = torch.pow(2.0, -k.float())
    w = codes.view(FP8).float() * scale[:, None]
    return w, codes, scale


# -- 1-3: the quantizer ------------------------------------------------------


def test_quantizer_lossless_on_representable_weights():
    gen = torch.Generator().manual_seed(0)
    w, codes, scale = representable(96, 128, gen)
    assert torch.equal(w.bfloat16().float(), w)  # exact in bf16
    for src in (w, w.bfloat16()):
        q, s = quant.quantize_fp8_per_channel(src)
        assert q.dtype == FP8 and s.dtype == torch.float32
        assert s.shape == (96,)
        assert torch.equal(s, scale)
        assert torch.equal(q.view(torch.uint8), codes)


def test_quantizer_saturates_instead_of_nan():
    w = torch.randn(4, 64) * 0.02
    w[1, 7] = 3.0e38  # one huge outlier
    w[2] = 0.0  # all-zero row -> scale 1.0
    q, s = quant.quantize_fp8_per_channel(w)
    raw = q.view(torch.uint8)
    assert not ((raw == 0x7F) | (raw == 0xFF)).any()
    deq = quant.dequantize_fp8(q, s)
    assert torch.isfinite(deq).all()
    assert s[2] == 1.0 and (deq[2] == 0).all()
    # the documented reason for the clamp
    assert torch.isnan(torch.tensor(500.0).to(FP8).float())


def test_quantizer_error_bound_gaussian():
    """E4M3 has 3 mantissa bits: per-element relative rounding <= 2^-4, so
    the Frobenius error is bounded by 2^-4 * ||W||."""
    gen = torch.Generator().manual_seed(1)
    w = torch.randn(4096, 4096, generator=gen) * 0.02
    q, s = quant.quantize_fp8_per_channel(w)
    err = (quant.dequantize_fp8(q, s) - w).norm()
    print(f"relative Frobenius error {float(err / w.norm()):.5f}")
    assert err <= 2.0**-4 * w.norm()


# -- 4: model equivalence on representable weights ---------------------------


def tiny_state_dict(cfg, gen):
    """HF-format fp32 state dict whose projections are representable."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    D = cfg.head_dim
    sd = {
        "model.embed_tokens.weight": torch.randn(cfg.vocab_size, H, generator=gen) * 0.5,
        "lm_head.weight": torch.randn(cfg.vocab_size, H, generator=gen) * 0.1,
        "model.norm.weight": torch.ones(H),
    }
    shapes = {
        "self_attn.q_proj": (cfg.num_heads * D, H),
        "self_attn.k_proj": (cfg.num_kv_heads * D, H),
        "self_attn.v_proj": (cfg.num_kv_heads * D, H),
        "self_attn.o_proj": (H, cfg.num_heads * D),
        "mlp.gate_proj": (I, H),
        "mlp.up_proj": (I, H),
        "mlp.down_proj": (H, I),
    }
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"] = torch.ones(H)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(H)
        for name, (m, k) in shapes.items():
            # 2^-k * 448 with k in [4,12) spans 0.1..28: rescale so the
            # activations stay O(1); a power of two keeps it representable
            w, _, _ = representable(m, k, gen)
            sd[p + name + ".weight"] = w * 2.0**-7
    return sd


def prefill_logits(model, ids):
    T = len(ids)
    meta = AttentionMetadata(
        is_prefill=True,
        slot_mapping=torch.zeros(T, dtype=torch.int32),
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32),
        max_seqlen=T,
    )
    caches = [(torch.empty(0), torch.empty(0))] * model.config.num_layers
    hidden = model(torch.tensor(ids), torch.arange(T), caches, meta)
    return model.compute_logits(hidden)


@pytest.fixture(scope="module")
def tiny_sd():
    return tiny_state_dict(ModelConfig.tiny(), torch.Generator().manual_seed(2))


def test_model_equivalence_on_representable_weights(tiny_sd):
    ref = LlamaForCausalLM(ModelConfig.tiny(), dtype=torch.float32)
    ref.load_hf_state_dict(tiny_sd)
    cfg = ModelConfig.tiny()
    cfg.quantization = "fp8"
    qm = LlamaForCausalLM(cfg, dtype=torch.float32)
    qm.load_hf_state_dict(tiny_sd)
    ids = [3, 17, 200, 45, 9, 128, 77, 1, 0, 255, 31]
    with torch.no_grad():
        a = prefill_logits(ref, ids)
        b = prefill_logits(qm, ids)
    # BLAS kernel selection only: the weights are represented exactly
    torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)


def _cpu_engine(quantization, sd):
    from kserve_amd.engine.engine import LLMEngine

    mcfg = ModelConfig.tiny()
    mcfg.quantization = quantization
    mcfg.dtype = "float32"
    engine = LLMEngine(
        EngineConfig(
            model=mcfg,
            cache=CacheConfig(block_size=4, num_gpu_blocks=128),
            scheduler=SchedulerConfig(
                max_num_seqs=8, max_num_batched_tokens=256, max_model_len=128
            ),
            device="cpu",
            eos_token_id=-1,
        )
    )
    engine.model.load_hf_state_dict(sd)
    return engine


def test_engine_greedy_tokens_equal_on_representable_weights(tiny_sd):
    from kserve_amd.engine.sampling_params import SamplingParams

    prompts = [[1, 2, 3, 4, 5], [100, 200, 30], [7, 8, 9, 10]]
    sp = SamplingParams(temperature=0.0, max_tokens=16)
    toks = []
    for quantization in (None, "fp8"):
        out = _cpu_engine(quantization, tiny_sd).generate(prompts, sp)
        toks.append([o.output_token_ids for o in out.values()])
    assert all(len(t) == 16 for t in toks[0])
    assert toks[0] == toks[1]


# -- 5: layer plumbing -------------------------------------------------------


def test_layer_plumbing():
    from kserve_amd.parallel.layers import (
        ColumnParallelLinear,
        MergedColumnParallelLinear,
        QKVParallelLinear,
        RowParallelLinear,
    )

    layers = {
        "col": (ColumnParallelLinear(64, 128, quantization="fp8"), 128, 64),
        "qkv": (QKVParallelLinear(64, 16, 4, 2, quantization="fp8"), 128, 64),
        "row": (RowParallelLinear(128, 64, quantization="fp8"), 64, 128),
        "merged": (MergedColumnParallelLinear(64, 128, quantization="fp8"), 256, 64),
    }
    for name, (layer, out_local, in_local) in layers.items():
        names = dict(layer.named_parameters())
        assert "weight" not in names and not hasattr(layer, "weight"), name
        assert layer.qweight.dtype == FP8
        assert layer.qweight.shape == (out_local, in_local)
        assert layer.weight_scale.dtype == torch.float32
        assert layer.weight_scale.shape == (out_local,)
        assert not layer.qweight.requires_grad
    with pytest.raises(ValueError):
        ColumnParallelLinear(64, 128, quantization="int4")
    # default: exactly the old parameters
    plain = ColumnParallelLinear(64, 128)
    assert set(dict(plain.named_parameters())) == {"weight"}


def test_model_plumbing_and_random_init():
    cfg = ModelConfig.tiny()
    cfg.quantization = "fp8"
    model = LlamaForCausalLM(cfg).random_init(seed=3)  # bf16 model
    assert model.lm_head.weight.dtype == torch.bfloat16
    assert not hasattr(model.lm_head, "qweight")
    assert model.embed_tokens.weight.dtype == torch.bfloat16
    for layer in model.layers:
        for lin in (
            layer.self_attn.qkv_proj, layer.self_attn.o_proj,
            layer.mlp.gate_up_proj, layer.mlp.down_proj,
        ):
            raw = lin.qweight.view(torch.uint8)
            assert not ((raw == 0x7F) | (raw == 0xFF)).any()
            # every row was scaled to its absmax: +-448 appears in each
            assert (lin.qweight.float().abs().amax(dim=1) == 448).all()
            assert (lin.weight_scale > 0).all()
            deq = quant.dequantize_fp8(lin.qweight, lin.weight_scale)
            assert 0.015 < float(deq.std()) < 0.025  # std = 0.02 draw
    # num_parameters keeps counting elements
    plain = LlamaForCausalLM(ModelConfig.tiny())
    n_scales = sum(
        p.numel() for n, p in model.named_parameters() if n.endswith("weight_scale")
    )
    assert model.num_parameters() == plain.num_parameters() + n_scales
    # the default model is untouched by the feature
    assert all(p.dtype == torch.bfloat16 for p in plain.parameters())


def test_config_validation():
    assert ModelConfig.tiny().quantization is None
    with pytest.raises(ValueError):
        ModelConfig(quantization="int4")
    cfg = ModelConfig.tiny()
    cfg.num_local_experts = 4
    cfg.quantization = "fp8"
    with pytest.raises(ValueError, match="mixture-of-experts"):
        LlamaForCausalLM(cfg)


# -- 6: pre-quantized checkpoints --------------------------------------------


def _write_fp8_checkpoint(tmp_path, cfg, gen, blockwise=False):
    """q/k/v/o/gate/up/down in fp8: per-tensor scalar scales on some
    projections ([] and [1]), per-channel on others ([M] and [M, 1])."""
    from safetensors.torch import save_file

    H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    sd = {
        "model.embed_tokens.weight": torch.randn(cfg.vocab_size, H, generator=gen) * 0.5,
        "lm_head.weight": torch.randn(cfg.vocab_size, H, generator=gen) * 0.1,
        "model.norm.weight": torch.ones(H),
    }
    # name -> (shape, scale layout)
    projs = {
        "self_attn.q_proj": ((cfg.num_heads * D, H), "scalar"),
        "self_attn.k_proj": ((cfg.num_kv_heads * D, H), "channel"),
        "self_attn.v_proj": ((cfg.num_kv_heads * D, H), "one"),
        "self_attn.o_proj": ((H, cfg.num_heads * D), "column"),
        "mlp.gate_proj": ((I, H), "channel"),
        "mlp.up_proj": ((I, H), "scalar"),
        "mlp.down_proj": ((H, I), "one"),
    }
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}."
        sd[p + "input_layernorm.weight"] = torch.ones(H)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(H)
        for name, ((m, k), layout) in projs.items():
            w = torch.randn(m, k, generator=gen) * 0.1
            if layout in ("scalar", "one"):
                s = w.abs().max() / 448.0
                q = (w / s).clamp(-448, 448).to(FP8)
                s = s.reshape(()) if layout == "scalar" else s.reshape(1)
            else:
                q, s = quant.quantize_fp8_per_channel(w)
                if layout == "column":
                    s = s[:, None]
            sd[p + name + ".weight"] = q
            key = ".weight_scale_inv" if blockwise else ".weight_scale"
            sd[p + name + key] = s.contiguous()
            sd[p + name + ".input_scale"] = torch.tensor(0.123)  # ignored
    d = tmp_path / ("ckpt_block" if blockwise else "ckpt")
    d.mkdir()
    save_file(sd, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps({
        "vocab_size": cfg.vocab_size, "hidden_size": H,
        "intermediate_size": I, "num_hidden_layers": cfg.num_layers,
        "num_attention_heads": cfg.num_heads,
        "num_key_value_heads": cfg.num_kv_heads,
        "max_position_embeddings": cfg.max_position_embeddings,
        "rope_theta": cfg.rope_theta,
        "quantization_config": {"quant_method": "fp8",
                                "activation_scheme": "static"},
    }))
    return str(d), sd


def test_prequantized_checkpoint(tmp_path):
    pytest.importorskip("safetensors")
    from kserve_amd.engine.weights import load_safetensors_weights

    base = ModelConfig.tiny()
    gen = torch.Generator().manual_seed(4)
    path, sd = _write_fp8_checkpoint(tmp_path, base, gen)
    cfg = ModelConfig.from_hf_config(os.path.join(path, "config.json"))
    assert cfg.quantization == "fp8"
    model = LlamaForCausalLM(cfg, dtype=torch.float32)
    load_safetensors_weights(model, path)

    # the same tensors placed by hand: bytes copied, scales broadcast to
    # per-channel, fused projections concatenated
    hand = LlamaForCausalLM(cfg, dtype=torch.float32)

    def ch(name):
        w = sd[name + ".weight"]
        return w, sd[name + ".weight_scale"].float().reshape(-1).expand(
            w.shape[0] if sd[name + ".weight_scale"].numel() == 1 else -1
        )

    with torch.no_grad():
        hand.embed_tokens.weight.copy_(sd["model.embed_tokens.weight"])
        hand.lm_head.weight.copy_(sd["lm_head.weight"])
        hand.norm.copy_(sd["model.norm.weight"])
        for i, layer in enumerate(hand.layers):
            p = f"model.layers.{i}."
            layer.input_layernorm.fill_(1.0)
            layer.post_attention_layernorm.fill_(1.0)
            for lin, names in (
                (layer.self_attn.qkv_proj,
                 ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"]),
                (layer.self_attn.o_proj, ["self_attn.o_proj"]),
                (layer.mlp.gate_up_proj, ["mlp.gate_proj", "mlp.up_proj"]),
                (layer.mlp.down_proj, ["mlp.down_proj"]),
            ):
                parts = [ch(p + n) for n in names]
                lin.qweight.copy_(torch.cat([q for q, _ in parts]))
                lin.weight_scale.copy_(torch.cat([s for _, s in parts]))
    for (n1, p1), (n2, p2) in zip(
        model.named_parameters(), hand.named_parameters()
    ):
        assert n1 == n2
        if p1.dtype == FP8:
            assert torch.equal(p1.view(torch.uint8), p2.view(torch.uint8)), n1
        else:
            assert torch.equal(p1, p2), n1
    ids = [5, 6, 7, 250, 3, 99, 12]
    with torch.no_grad():
        assert torch.equal(prefill_logits(model, ids), prefill_logits(hand, ids))

    # a bf16 model given the fp8 checkpoint dequantizes it: same function
    plain = LlamaForCausalLM(base, dtype=torch.float32)
    load_safetensors_weights(plain, path)
    with torch.no_grad():
        torch.testing.assert_close(
            prefill_logits(plain, ids), prefill_logits(model, ids),
            rtol=1e-4, atol=1e-4,
        )


def test_blockwise_checkpoint_is_refused(tmp_path):
    pytest.importorskip("safetensors")
    from kserve_amd.engine.weights import load_safetensors_weights

    gen = torch.Generator().manual_seed(5)
    path, _ = _write_fp8_checkpoint(tmp_path, ModelConfig.tiny(), gen, blockwise=True)
    cfg = ModelConfig.from_hf_config(os.path.join(path, "config.json"))
    model = LlamaForCausalLM(cfg, dtype=torch.float32)
    with pytest.raises(ValueError, match="weight_scale_inv"):
        load_safetensors_weights(model, path)


# -- 7: TP=2 under gloo ------------------------------------------------------


def _tp2_w8_worker(rank, world, port, q):
    try:
        os.environ.update(
            RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
            MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
        )
        from kserve_amd.parallel import comm
        from kserve_amd.parallel.layers import (
            ColumnParallelLinear,
            MergedColumnParallelLinear,
            QKVParallelLinear,
            RowParallelLinear,
        )

        comm.init_distributed(tp_size=2, backend="gloo")
        torch.manual_seed(0)
        full_w1 = torch.randn(32, 16)
        full_w2 = torch.randn(16, 32)
        x = torch.randn(4, 16)
        x2 = torch.randn(4, 32)
        qz = quant.quantize_fp8_per_channel
        ref = torch_ref.linear_w8

        # column: per-rank row shards, gathered
        col = ColumnParallelLinear(
            16, 32, dtype=torch.float32, gather_output=True, quantization="fp8"
        )
        col.load_shard(full_w1)
        ref_y = torch.cat(
            [ref(x, *qz(full_w1[r * 16 : (r + 1) * 16])) for r in range(2)], dim=-1
        )
        torch.testing.assert_close(col(x), ref_y, atol=1e-5, rtol=1e-5)

        # row: per-rank COLUMN shards quantized after slicing (per-rank
        # scales), partials summed by the all-reduce
        lo, hi = rank * 16, (rank + 1) * 16
        row = RowParallelLinear(32, 16, dtype=torch.float32, quantization="fp8")
        row.load_shard(full_w2)
        q_r, s_r = qz(full_w2[:, lo:hi])
        assert torch.equal(row.qweight.view(torch.uint8), q_r.view(torch.uint8))
        assert torch.equal(row.weight_scale, s_r)
        ref_z = sum(
            ref(x2[:, r * 16 : (r + 1) * 16], *qz(full_w2[:, r * 16 : (r + 1) * 16]))
            for r in range(2)
        )
        torch.testing.assert_close(row(x2[:, lo:hi]), ref_z, atol=1e-4, rtol=1e-4)
        # the overlap path slices codes and scales together
        over = RowParallelLinear(
            32, 16, dtype=torch.float32, quantization="fp8", overlap_chunks=3
        )
        over.load_shard(full_w2)
        over.OVERLAP_MIN_NUMEL = 1
        torch.testing.assert_close(over(x2[:, lo:hi]), ref_z, atol=1e-4, rtol=1e-4)

        # fused QKV: 4 heads / 2 kv heads of dim 8 -> 2 + 1 + 1 heads per rank
        wq, wk, wv = torch.randn(32, 16), torch.randn(16, 16), torch.randn(16, 16)
        qkv = QKVParallelLinear(16, 8, 4, 2, dtype=torch.float32, quantization="fp8")
        qkv.load_shards(wq, wk, wv)
        got = torch.cat(qkv(x), dim=-1)
        shard = torch.cat(
            [wq[rank * 16 : (rank + 1) * 16], wk[rank * 8 : (rank + 1) * 8],
             wv[rank * 8 : (rank + 1) * 8]]
        )
        torch.testing.assert_close(got, ref(x, *qz(shard)), atol=1e-5, rtol=1e-5)

        # merged gate/up
        wg, wu = torch.randn(32, 16), torch.randn(32, 16)
        merged = MergedColumnParallelLinear(
            16, 32, dtype=torch.float32, quantization="fp8"
        )
        merged.load_shards(wg, wu)
        shard = torch.cat([wg[lo:hi], wu[lo:hi]])
        torch.testing.assert_close(
            merged(x), ref(x, *qz(shard)), atol=1e-5, rtol=1e-5
        )
        comm.destroy_distributed()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {type(e).__name__}: {e}\n{traceback.format_exc()}"))


@pytest.mark.timeout(300)
def test_tp2_quantized_parallel_linears():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(target=_tp2_w8_worker, args=(r, 2, 29641, q)) for r in range(2)
    ]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"


# -- 8: CLI ------------------------------------------------------------------


def test_cli_quantization_flag(tmp_path):
    from kserve_amd.runtimes.huggingfaceserver import (
        build_parser,
        engine_model_config,
    )

    cfg = ModelConfig.tiny()
    (tmp_path / "config.json").write_text(json.dumps({
        "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden_size,
        "intermediate_size": cfg.intermediate_size,
        "num_hidden_layers": cfg.num_layers,
        "num_attention_heads": cfg.num_heads,
        "num_key_value_heads": cfg.num_kv_heads,
    }))
    base = ["--model_dir", str(tmp_path)]
    parser = build_parser()
    assert engine_model_config(parser.parse_args(base)).quantization is None
    assert engine_model_config(
        parser.parse_args(base + ["--quantization", "none"])
    ).quantization is None
    assert engine_model_config(
        parser.parse_args(base + ["--quantization", "fp8"])
    ).quantization == "fp8"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--quantization", "int4"])


# -- 9: LoRA on a quantized base ---------------------------------------------


def test_lora_on_quantized_base_layer():
    """LoRA deltas sit outside ops.linear_w8: a quantized MLP with an
    adapter equals torch_ref.linear_w8 plus the explicit deltas."""
    from kserve_amd.engine.lora import LoRABatchMeta, LoRALayerWeights
    from kserve_amd.models.llama import LlamaMLP

    RANK, ALPHA = 4, 8.0
    cfg = ModelConfig.tiny()
    cfg.quantization = "fp8"
    gen = torch.Generator().manual_seed(6)
    mlp = LlamaMLP(cfg, torch.float32, layer_idx=0)
    H, I = cfg.hidden_size, cfg.intermediate_size
    mlp.gate_up_proj.load_shards(
        torch.randn(I, H, generator=gen) * 0.1, torch.randn(I, H, generator=gen) * 0.1
    )
    mlp.down_proj.load_shard(torch.randn(H, I, generator=gen) * 0.1)

    def lw(out, inp):
        return LoRALayerWeights(
            a=torch.randn(RANK, inp, generator=gen) * 0.05,
            b=torch.randn(out, RANK, generator=gen) * 0.05,
            scale=ALPHA / RANK,
        )

    weights = {"gate_proj": lw(I, H), "up_proj": lw(I, H), "down_proj": lw(H, I)}
    manager = types.SimpleNamespace(
        layer_weights=lambda aid, layer, module: weights.get(module)
        if aid == 1 else None
    )
    T = 6
    x = torch.randn(T, H, generator=gen)
    meta = types.SimpleNamespace(lora=LoRABatchMeta([(1, 0, T)], manager))
    with torch.no_grad():
        base = mlp(x, types.SimpleNamespace(lora=None))
        got = mlp(x, meta)
        gu = torch_ref.linear_w8(
            x, mlp.gate_up_proj.qweight, mlp.gate_up_proj.weight_scale
        )
        gu[:, :I] += weights["gate_proj"].delta(x)
        gu[:, I:] += weights["up_proj"].delta(x)
        act = torch_ref.silu_and_mul(gu)
        want = torch_ref.linear_w8(
            act, mlp.down_proj.qweight, mlp.down_proj.weight_scale
        ) + weights["down_proj"].delta(act)
    assert not torch.allclose(got, base)  # the adapter changes the output
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)


def test_lora_on_quantized_engine(tmp_path):
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_lora import make_adapter_dir

    torch.manual_seed(0)
    mcfg = ModelConfig.tiny(vocab_size=128)
    mcfg.quantization = "fp8"
    engine = LLMEngine(EngineConfig(
        model=mcfg,
        cache=CacheConfig(block_size=4, num_gpu_blocks=128),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=256, max_model_len=128
        ),
        device="cpu",
        eos_token_id=-1,
    ))
    path, _ = make_adapter_dir(tmp_path, engine.config.model)
    engine.register_lora("adapt", path)
    prompts = [[1, 2, 3, 4, 5], [9, 8, 7]]
    base = engine.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6))
    lora = engine.generate(
        prompts, SamplingParams(temperature=0.0, max_tokens=6, lora_name="adapt")
    )
    base = [o.output_token_ids for o in base.values()]
    lora = [o.output_token_ids for o in lora.values()]
    assert all(len(t) == 6 for t in lora)
    assert base != lora


# -- static check: the extension cross-compiles and exports the bindings -----


def test_extension_builds_and_exports_w8_bindings():
    """python build_hip.py must succeed by cross-compile and the module
    must export both new bindings (symbol list only)."""
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "build_hip.py")],
        cwd=REPO, capture_output=True, text=True,
    )
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    code = (
        "import kserve_amd_C as C; "
        "print(hasattr(C, 'skinny_gemm_w8'), hasattr(C, 'dequant_fp8_rows'))"
    )
    r = subprocess.run(
        [sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True
    )
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["True", "True"]


def test_cpu_dispatch_is_the_reference():
    x = torch.randn(3, 64)
    q, s = quant.quantize_fp8_per_channel(torch.randn(32, 64))
    b = torch.randn(32)
    assert torch.equal(ops.linear_w8(x, q, s, b), torch_ref.linear_w8(x, q, s, b))
    want = (x @ quant.dequantize_fp8(q, s).t()) + b
    torch.testing.assert_close(ops.linear_w8(x, q, s, b), want, rtol=1e-5, atol=1e-5)
