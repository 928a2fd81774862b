"""Weight-only fp8 (E4M3) on the GPU: the fp8-weight skinny GEMM, the row
dequantizer, ops.linear_w8 dispatch and the engine with quantization="fp8".

Every shape is the smallest that reaches its code path (see the table in
test_w8_gemm_matches_reference)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    return "cuda"


def _finite_bytes(shape, gen):
    """random e4m3 byte codes with the two NaN codes replaced by 0"""
    b = torch.randint(0, 256, shape, generator=gen, dtype=torch.int32)
    b[(b == 0x7F) | (b == 0xFF)] = 0
    return b.to(torch.uint8)


# -- 1: every byte code converts exactly -------------------------------------


def _all_codes_weight(M, K, row_step=None):
    """byte[m][k] = (m * row_step + k) % 256 (row_step = K: the bytes count
    up through the rows) with the two NaN codes replaced by 0, and
    power-of-two scales 2^-12..2^3, so that code x scale is exact in bf16."""
    m = torch.arange(M, dtype=torch.int32)[:, None]
    k = torch.arange(K, dtype=torch.int32)[None, :]
    codes = (m * (K if row_step is None else row_step) + k) % 256
    codes[(codes == 0x7F) | (codes == 0xFF)] = 0
    assert len(torch.unique(codes)) == 254  # all finite codes present
    scale = torch.pow(2.0, (torch.arange(M) % 16 - 12).float())
    return codes.to(torch.uint8).view(FP8), scale


def test_every_code_converts_exactly(dev):
    """x = I: out[n][m] must be q[m][n] * scale[m] exactly. Catches a wrong
    nibble/half in the packed convert, a wrong scale<->feature mapping and
    any K-order mismatch between the X and W fragments. N=64, K=64, M=256:
    single K step, no K-split."""
    import kserve_amd_C

    N, K, M = 64, 64, 256
    q, scale = _all_codes_weight(M, K)
    q, scale = q.to(dev), scale.to(dev)
    x = torch.eye(N, K, dtype=torch.bfloat16, device=dev)
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.skinny_gemm_w8(out, x, q, scale)
    torch.cuda.synchronize()
    want = (q.float() * scale[:, None]).t()  # [n][m]
    assert torch.equal(out.float(), want)


_EXACT_M = 64  # one feature workgroup: the policy splits K 8 ways


@functools.lru_cache(maxsize=None)
def _exact_weight(K):
    """(q, scale, want [M, K] f32) on the CPU, shared by the cases of a K.
    code x 2^e has at most 4 significant bits, so want is exact in bf16."""
    q, scale = _all_codes_weight(_EXACT_M, K, row_step=37)
    want = q.float() * scale[:, None]
    assert torch.equal(want.bfloat16().float(), want)
    return q, scale, want


@pytest.mark.parametrize(
    "NT,steps",
    # every NT the launcher can select, at 3 steps per split: once round
    # the pipelined loop, then the single-step tail
    [(nt, 3) for nt in (1, 2, 3, 4, 5, 6, 8, 12, 16)]
    # 2: no loop + the two-step tail; 4: loop + the two-step tail
    + [(3, 2), (3, 4)],
)
def test_every_instantiation_is_exact(dev, NT, steps):
    """One-hot x selects N = 16 NT - 3 consecutive columns (a ragged last
    token tile: the row clamp): out[n][m] must be q[m][off + n] * scale[m]
    exactly, for windows that cover all of K. M = 64 and K = 8 * steps * 64
    make every launch the 8-way split kernel plus the reduce; all partials
    but one are zero, so the sum is exact too."""
    import kserve_amd_C

    N, M, K = 16 * NT - 3, _EXACT_M, 8 * steps * 64
    q, scale, want = _exact_weight(K)
    qd, sd, want = q.to(dev), scale.to(dev), want.to(dev)
    x = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    rows = torch.arange(N, device=dev)
    for off in list(range(0, K - N, N)) + [K - N]:
        x[rows, off + rows] = 1.0
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.skinny_gemm_w8(out, x, qd, sd)
        x[rows, off + rows] = 0.0
        assert torch.equal(
            out.float(), want[:, off:off + N].t()
        ), f"columns {off}..{off + N - 1}"


# -- 2: numerics vs torch_ref.linear_w8 --------------------------------------


def _w8_case(N, K, M, dev, x_cols=None):
    """x = randn/8; codes and scales from quantizing randn/8 (the input
    scaling TestSkinnyGemm uses, so its tolerance carries over), then the
    per-channel scale is spread over 2^-10..2^3 by moving magnitude
    between code and scale: row m is re-encoded against scale * 2^(m % 14).
    The dequantized weights stay within randn/8, only the split differs."""
    from kserve_amd.ops.quant import quantize_fp8_per_channel

    gen = torch.Generator().manual_seed(N * 7 + K + M)
    x_full = torch.randn(N, x_cols or K, generator=gen) / 8
    w = torch.randn(M, K, generator=gen) / 8
    _, s0 = quantize_fp8_per_channel(w)  # ~2^-10
    scale = s0 * torch.pow(2.0, (torch.arange(M) % 14).float())
    q = (w / scale[:, None]).clamp(-448, 448).to(FP8)
    x = x_full.to(torch.bfloat16).to(dev)[:, :K]
    return x, q.to(dev), scale.to(dev)


def _ref(x, q, scale, bias=None):
    """fp32 on the GPU tensors moved to CPU"""
    from kserve_amd.ops import torch_ref

    return torch_ref.linear_w8(
        x.float().cpu(), q.cpu(), scale.cpu(),
        None if bias is None else bias.float().cpu(),
    )


@pytest.mark.parametrize(
    "N,K,M",
    [
        (1, 64, 64),        # the minimum
        (17, 512, 128),     # ragged N, split-K
        (97, 1024, 192),    # NT=7 -> the NT=8 instantiation
        (256, 256, 64),     # NT=16
        (64, 4096, 4096),   # a real o_proj shape
        (33, 128, 49152),   # no split at wide M
    ],
)
def test_w8_gemm_matches_reference(dev, N, K, M):
    import kserve_amd_C

    x, q, scale = _w8_case(N, K, M, dev)
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.skinny_gemm_w8(out, x, q, scale)
    torch.cuda.synchronize()
    ref = _ref(x, q, scale)
    print(f"max abs err {float((out.float().cpu() - ref).abs().max()):.5f}")
    torch.testing.assert_close(out.float().cpu(), ref, atol=0.05, rtol=0.05)


def test_w8_gemm_strided_x(dev):
    import kserve_amd_C

    N, K, M = 64, 512, 256
    x, q, scale = _w8_case(N, K, M, dev, x_cols=2 * K)
    assert x.stride(0) == 2 * K  # x_full[:, :K]
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.skinny_gemm_w8(out, x, q, scale)
    torch.cuda.synchronize()
    torch.testing.assert_close(
        out.float().cpu(), _ref(x, q, scale), atol=0.05, rtol=0.05
    )


# -- 3: dequant kernel -------------------------------------------------------


@pytest.mark.parametrize("M,K", [(64, 64), (192, 1088), (5, 24)])
def test_dequant_rows_exact(dev, M, K):
    """(5, 24): K not a multiple of 16 takes the per-element kernel.
    Scales in [2^-12, 2^3] keep every product a normal f32."""
    import kserve_amd_C

    gen = torch.Generator().manual_seed(M + K)
    q = _finite_bytes((M, K), gen).view(FP8)
    scale = torch.pow(2.0, torch.randint(-12, 4, (M,), generator=gen).float())
    out = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.dequant_fp8_rows(out, q.to(dev), scale.to(dev))
    torch.cuda.synchronize()
    want = (q.float() * scale[:, None]).bfloat16()
    assert torch.equal(out.cpu().float(), want.float())


# -- 4: ops.linear_w8 dispatch -----------------------------------------------


def _spy(monkeypatch):
    from kserve_amd import ops

    calls = {"skinny_gemm_w8": 0, "dequant_fp8_rows": 0}

    class Spy:
        def __getattr__(self, name):
            fn = getattr(ops._C, name)
            if name in calls:
                def wrapped(*a):
                    calls[name] += 1
                    return fn(*a)
                return wrapped
            return fn

    monkeypatch.setattr(ops, "_native", lambda op: Spy())
    return calls


@pytest.mark.parametrize(
    "N,K,M,path",
    [
        (16, 128, 128, "skinny_gemm_w8"),
        (300, 128, 128, "dequant_fp8_rows"),  # N above the kernel's limit
        (16, 128, 96, "dequant_fp8_rows"),    # M % 64 != 0
    ],
)
def test_linear_w8_dispatch(dev, monkeypatch, N, K, M, path):
    from kserve_amd import ops

    calls = _spy(monkeypatch)
    x, q, scale = _w8_case(N, K, M, dev)
    bias = (torch.randn(M, generator=torch.Generator().manual_seed(1)) / 8).to(
        torch.bfloat16
    ).to(dev)
    for b in (None, bias):
        got = ops.linear_w8(x, q, scale, b)
        torch.cuda.synchronize()
        assert got.shape == (N, M) and got.dtype == torch.bfloat16
        torch.testing.assert_close(
            got.float().cpu(), _ref(x, q, scale, b), atol=0.05, rtol=0.05
        )
    other = ({"skinny_gemm_w8", "dequant_fp8_rows"} - {path}).pop()
    assert calls[path] >= 2 and calls[other] == 0, calls


def test_linear_w8_dequant_path_chunks_a_large_weight(dev):
    """The scratch holds half of the largest weight seen: that weight
    goes through the dequant path in two row chunks."""
    from kserve_amd import ops

    N, K, M = 300, 64, 192
    x, q, scale = _w8_case(N, K, M, dev)
    saved = dict(ops._W8_SCRATCH)
    ops._W8_SCRATCH.clear()
    try:
        ops.reserve_w8_scratch(dev, M, K)
        buf = ops._W8_SCRATCH[x.device]
        assert buf.numel() == (M // 2) * K
        got = ops.linear_w8(x, q, scale)
        torch.cuda.synchronize()
        assert ops._W8_SCRATCH[x.device] is buf  # forward did not allocate
    finally:
        ops._W8_SCRATCH.clear()
        ops._W8_SCRATCH.update(saved)
    torch.testing.assert_close(
        got.float().cpu(), _ref(x, q, scale), atol=0.05, rtol=0.05
    )


# -- 5: engine ---------------------------------------------------------------


def _cfg(enforce_eager=False, num_blocks=128, quantization="fp8",
         kv_cache_dtype="auto"):
    """tests/test_gpu_engine.py::_cfg with quantization"""
    from kserve_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        ModelConfig,
        SchedulerConfig,
    )

    return EngineConfig(
        model=ModelConfig(
            vocab_size=2048,
            hidden_size=512,
            intermediate_size=1024,
            num_layers=4,
            num_heads=4,
            num_kv_heads=2,
            head_dim=128,
            max_position_embeddings=1024,
            model_name="gpu-tiny",
            quantization=quantization,
        ),
        cache=CacheConfig(
            block_size=16, num_gpu_blocks=num_blocks,
            kv_cache_dtype=kv_cache_dtype,
        ),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=2048, max_model_len=512
        ),
        device="cuda",
        seed=0,
        eos_token_id=-1,
        enforce_eager=enforce_eager,
    )


def test_fp8_graph_matches_eager(dev):
    """Same prompts and lengths as test_graph_matches_eager (identical
    batch shapes on both sides, so token equality is legitimate)."""
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    prompts = [[1, 2, 3, 4, 5], [100, 200, 300], [7, 8, 9, 10]]
    sp = SamplingParams(temperature=0.0, max_tokens=16)

    engine_e = LLMEngine(_cfg(enforce_eager=True))
    assert engine_e.model.layers[0].mlp.down_proj.qweight.dtype == FP8
    out_e = engine_e.generate(prompts, sp)
    del engine_e
    torch.cuda.empty_cache()

    engine_g = LLMEngine(_cfg(enforce_eager=False))
    out_g = engine_g.generate(prompts, sp)
    toks_e = [o.output_token_ids for o in out_e.values()]
    toks_g = [o.output_token_ids for o in out_g.values()]
    assert all(len(t) == 16 for t in toks_g)
    assert toks_e == toks_g


def test_fp8_logits_match_cpu_reference(dev):
    """GPU bf16 prefill (T=33) vs a CPU fp32 model holding the same
    qweight/weight_scale; the criteria of test_logits_match_cpu_reference."""
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import AttentionMetadata, LlamaForCausalLM

    cfg = ModelConfig(
        vocab_size=512,
        hidden_size=256,
        intermediate_size=512,
        num_layers=2,
        num_heads=2,
        num_kv_heads=1,
        head_dim=128,
        max_position_embeddings=256,
        quantization="fp8",
    )
    torch.manual_seed(0)
    cpu_model = LlamaForCausalLM(cfg, dtype=torch.float32, device="cpu")
    cpu_model.random_init(seed=5)
    gpu_model = LlamaForCausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(
            gpu_model.named_parameters(), cpu_model.named_parameters()
        ):
            assert n1 == n2
            if p2.dtype == FP8 or n2.endswith("weight_scale"):
                p1.copy_(p2)  # codes and f32 scales, bit for bit
            else:
                p1.copy_(p2.to(torch.bfloat16))

    T = 33
    ids = torch.randint(0, cfg.vocab_size, (T,))
    pos = torch.arange(T)

    def run(model, device):
        meta = AttentionMetadata(
            is_prefill=True,
            slot_mapping=torch.arange(T, dtype=torch.int32, device=device),
            cu_seqlens=torch.tensor([0, T], dtype=torch.int32, device=device),
            max_seqlen=T,
        )
        caches = [
            (
                torch.zeros(8, cfg.num_kv_heads, 16, 128, dtype=model.dtype, device=device),
                torch.zeros(8, cfg.num_kv_heads, 16, 128, dtype=model.dtype, device=device),
            )
            for _ in range(cfg.num_layers)
        ]
        hidden = model(ids.to(device), pos.to(device), caches, meta)
        return model.compute_logits(hidden)

    with torch.no_grad():
        ref = run(cpu_model, "cpu")
        got = run(gpu_model, "cuda")
    agree = (got.float().cpu().argmax(-1) == ref.argmax(-1)).float().mean()
    cos = torch.nn.functional.cosine_similarity(
        got.float().cpu().flatten(), ref.flatten(), dim=0
    )
    print(f"top-1 agreement {float(agree):.3f} cosine {float(cos):.5f}")
    assert agree > 0.9, f"top-1 agreement {agree}"
    assert cos > 0.99, f"cosine {cos}"


def test_fp8_engine_dequant_path_prompt(dev):
    """A 300-token prompt prefills through the dequant path (N > 256) in
    the same engine that decodes through the skinny kernel."""
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    engine = LLMEngine(_cfg())
    prompt = [(7 * i + 3) % 2048 for i in range(300)]
    out = engine.generate(
        [prompt, [1, 2, 3]], SamplingParams(temperature=0.0, max_tokens=8)
    )
    assert len(out) == 2
    for o in out.values():
        assert len(o.output_token_ids) == 8


def test_fp8_weights_with_fp8_kv(dev):
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    prompts = [[1, 2, 3, 4, 5], [100, 200, 300]]
    sp = SamplingParams(temperature=0.0, max_tokens=8)
    runs = []
    for _ in range(2):
        engine = LLMEngine(_cfg(kv_cache_dtype="fp8"))
        out = engine.generate(prompts, sp)
        runs.append([o.output_token_ids for o in out.values()])
        del engine
        torch.cuda.empty_cache()
    assert all(len(t) == 8 for t in runs[0])
    assert runs[0] == runs[1]


def test_fp8_model_memory(dev):
    """Model build with fp8 must allocate less than the bf16 build by at
    least 40 % of the bf16 bytes of the quantized projections (1 byte +
    4/K per weight instead of 2; the margin covers the dequant scratch,
    which is counted here)."""
    from kserve_amd import ops
    from kserve_amd.models.llama import LlamaForCausalLM

    def build(quantization):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        mcfg = _cfg(quantization=quantization).model
        with torch.device("cuda"):
            model = LlamaForCausalLM(mcfg, device="cuda")
        model.random_init(seed=0)
        torch.cuda.synchronize()
        used = torch.cuda.memory_allocated() - before
        proj = sum(
            p.numel() for n, p in model.named_parameters()
            if n.endswith("qweight")
        )
        return used, proj

    saved = dict(ops._W8_SCRATCH)
    ops._W8_SCRATCH.clear()  # count the scratch against the fp8 build
    try:
        bf16_used, _ = build(None)
        fp8_used, proj_elems = build("fp8")
    finally:
        ops._W8_SCRATCH.clear()
        ops._W8_SCRATCH.update(saved)
    proj_bf16_bytes = 2 * proj_elems
    print(f"bf16 {bf16_used} B, fp8 {fp8_used} B, projections {proj_bf16_bytes} B, "
          f"saved {(bf16_used - fp8_used) / proj_bf16_bytes:.3f} of them")
    assert proj_elems > 0
    assert bf16_used - fp8_used >= 0.4 * proj_bf16_bytes
