"""Weight-only MXFP4 (E2M1 codes, E8M0 block scales) on the GPU: the
fp4-weight skinny GEMM, the row dequantizer, ops.linear_w4 dispatch and the
engine with quantization="mxfp4".

Every shape is the smallest that reaches its code path (see the table in
test_w4_gemm_matches_reference)."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    return "cuda"


# -- 1: every code converts exactly ------------------------------------------


def _all_codes_weight(M, K):
    """byte[m][j] = (m + 37 j) % 256: with M = 256 rows every byte column,
    i.e. every (K group of the lane, byte of its 16 B) position class,
    holds all 256 byte values. Scale codes 127 + ((m + g) % 16) - 12 differ
    between neighbouring rows and neighbouring blocks."""
    m = torch.arange(M, dtype=torch.int64)[:, None]
    j = torch.arange(K // 2, dtype=torch.int64)[None, :]
    q = ((m + 37 * j) % 256).to(torch.uint8)
    if M >= 256:
        assert all(len(torch.unique(q[:, c])) == 256 for c in range(K // 2))
    g = torch.arange(K // 32, dtype=torch.int64)[None, :]
    scale = (127 + ((m + g) % 16) - 12).to(torch.uint8)
    return q.contiguous(), scale.contiguous()


@pytest.mark.parametrize(
    "K",
    [
        128,   # one K step, no split
        256,   # two splits of one step each at M = 256
        1024,  # 8 splits of one step each
        2048,  # 8 splits of two steps: the other register set and X buffer
        3072,  # 8 splits of three steps: once round the pipelined loop
    ],
)
def test_every_code_converts_exactly(dev, K):
    """x selects 128 consecutive columns: out[n][m] must be the
    dequantized w[m][off + n] exactly, for every 128-column window of K.
    Catches the nibble order, the byte select of the packed convert, which
    scale goes with which lane, and any K-order disagreement between the X
    and W fragments."""
    import kserve_amd_C
    from kserve_amd.ops import quant

    N, M = 128, 256
    q, scale = _all_codes_weight(M, K)
    want = quant.dequantize_mxfp4(q, scale)  # [M, K] f32, exact
    assert torch.equal(want.bfloat16().float(), want)
    qd, sd = q.to(dev), scale.to(dev)
    x = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    rows = torch.arange(N, device=dev)
    for off in range(0, K, 128):
        x[rows, off + rows] = 1.0
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.skinny_gemm_w4(out, x, qd, sd)
        torch.cuda.synchronize()
        x[rows, off + rows] = 0.0
        assert torch.equal(
            out.float().cpu(), want[:, off:off + 128].t()
        ), f"columns {off}..{off + 127}"


_EXACT_M = 64  # one feature workgroup: the policy splits K 8 ways


@functools.lru_cache(maxsize=None)
def _exact_weight(K):
    """(q, scale, want [M, K] f32) on the CPU, shared by the cases of a K"""
    from kserve_amd.ops import quant

    q, scale = _all_codes_weight(_EXACT_M, K)
    want = quant.dequantize_mxfp4(q, scale)
    assert torch.equal(want.bfloat16().float(), want)
    return q, scale, want


@pytest.mark.parametrize(
    "NT,steps",
    # every NT the launcher can select, at 3 steps per split: once round
    # the pipelined loop, then the single-step tail
    [(nt, 3) for nt in (1, 2, 3, 4, 5, 6, 8)]
    # 2: no loop + the two-step tail; 4: loop + the two-step tail
    + [(3, 2), (3, 4)],
)
def test_every_instantiation_is_exact(dev, NT, steps):
    """One-hot x selects N = 16 NT - 3 consecutive columns (a ragged last
    token tile: the row clamp): out[n][m] must be the dequantized
    w[m][off + n] exactly, for windows that cover all of K. M = 64 and
    K = 8 * steps * 128 make every launch the 8-way split kernel plus the
    reduce; all partials but one are zero, so the sum is exact too."""
    import kserve_amd_C

    N, M, K = 16 * NT - 3, _EXACT_M, 8 * steps * 128
    q, scale, want = _exact_weight(K)
    qd, sd, want = q.to(dev), scale.to(dev), want.to(dev)
    x = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    rows = torch.arange(N, device=dev)
    for off in list(range(0, K - N, N)) + [K - N]:
        x[rows, off + rows] = 1.0
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.skinny_gemm_w4(out, x, qd, sd)
        x[rows, off + rows] = 0.0
        assert torch.equal(
            out.float(), want[:, off:off + N].t()
        ), f"columns {off}..{off + N - 1}"


# -- 2: numerics vs torch_ref.linear_w4 --------------------------------------


def _w4_case(N, K, M, dev, x_cols=None):
    """x = randn/8; codes and scales from quantizing randn/8 (the input
    scaling of test_gpu_quant_fp8._w8_case, so its tolerance carries
    over: same accumulate and split structure)."""
    from kserve_amd.ops.quant import quantize_mxfp4

    gen = torch.Generator().manual_seed(N * 7 + K + M)
    x_full = torch.randn(N, x_cols or K, generator=gen) / 8
    w = torch.randn(M, K, generator=gen) / 8
    q, scale = quantize_mxfp4(w)
    x = x_full.to(torch.bfloat16).to(dev)[:, :K]
    return x, q.to(dev), scale.to(dev)


def _ref(x, q, scale, bias=None):
    """fp32 on the GPU tensors moved to CPU"""
    from kserve_amd.ops import torch_ref

    return torch_ref.linear_w4(
        x.float().cpu(), q.cpu(), scale.cpu(),
        None if bias is None else bias.float().cpu(),
    )


@pytest.mark.parametrize(
    "N,K,M",
    [
        (1, 128, 64),       # the minimum
        (17, 1024, 128),    # ragged N, split-K
        (97, 2048, 192),    # NT=7 -> the NT=8 instantiation
        (128, 256, 64),     # NT=8, the largest N
        (64, 4096, 4096),   # a real o_proj shape
        (33, 128, 49152),   # no split at wide M
    ],
)
def test_w4_gemm_matches_reference(dev, N, K, M):
    import kserve_amd_C

    x, q, scale = _w4_case(N, K, M, dev)
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.skinny_gemm_w4(out, x, q, scale)
    torch.cuda.synchronize()
    ref = _ref(x, q, scale)
    print(f"max abs err {float((out.float().cpu() - ref).abs().max()):.5f}")
    torch.testing.assert_close(out.float().cpu(), ref, atol=0.05, rtol=0.05)


def test_w4_gemm_strided_x(dev):
    import kserve_amd_C

    N, K, M = 64, 512, 256
    x, q, scale = _w4_case(N, K, M, dev, x_cols=2 * K)
    assert x.stride(0) == 2 * K  # x_full[:, :K]
    out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.skinny_gemm_w4(out, x, q, scale)
    torch.cuda.synchronize()
    torch.testing.assert_close(
        out.float().cpu(), _ref(x, q, scale), atol=0.05, rtol=0.05
    )


# -- 3: dequant kernel -------------------------------------------------------


@pytest.mark.parametrize("M,K", [(64, 128), (192, 1088), (5, 32)])
def test_dequant_rows_exact(dev, M, K):
    """Random bytes (all 16 codes, -0 included) and scale codes in
    [115, 130] keep every product a normal bf16."""
    import kserve_amd_C
    from kserve_amd.ops import quant

    gen = torch.Generator().manual_seed(M + K)
    q = torch.randint(0, 256, (M, K // 2), generator=gen, dtype=torch.int32).to(
        torch.uint8
    )
    scale = torch.randint(115, 131, (M, K // 32), generator=gen, dtype=torch.int32).to(
        torch.uint8
    )
    out = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    kserve_amd_C.dequant_mxfp4_rows(out, q.to(dev), scale.to(dev))
    torch.cuda.synchronize()
    want = quant.dequantize_mxfp4(q, scale, torch.bfloat16)
    assert torch.equal(out.cpu().float(), want.float())


# -- 4: ops.linear_w4 dispatch -----------------------------------------------


def _spy(monkeypatch):
    from kserve_amd import ops

    calls = {"skinny_gemm_w4": 0, "dequant_mxfp4_rows": 0}

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
        (16, 128, 128, "skinny_gemm_w4"),
        (300, 128, 128, "dequant_mxfp4_rows"),  # N above the threshold
        (16, 128, 96, "dequant_mxfp4_rows"),    # M % 64 != 0
        (16, 160, 128, "dequant_mxfp4_rows"),   # K % 128 != 0, K % 32 == 0
    ],
)
def test_linear_w4_dispatch(dev, monkeypatch, N, K, M, path):
    from kserve_amd import ops

    assert N <= ops.W4_MAX_TOKENS or path == "dequant_mxfp4_rows"
    calls = _spy(monkeypatch)
    x, q, scale = _w4_case(N, K, M, dev)
    bias = (torch.randn(M, generator=torch.Generator().manual_seed(1)) / 8).to(
        torch.bfloat16
    ).to(dev)
    for b in (None, bias):
        got = ops.linear_w4(x, q, scale, b)
        torch.cuda.synchronize()
        assert got.shape == (N, M) and got.dtype == torch.bfloat16
        torch.testing.assert_close(
            got.float().cpu(), _ref(x, q, scale, b), atol=0.05, rtol=0.05
        )
    other = ({"skinny_gemm_w4", "dequant_mxfp4_rows"} - {path}).pop()
    assert calls[path] >= 2 and calls[other] == 0, calls


def test_linear_w4_threshold_boundary(dev, monkeypatch):
    """N == W4_MAX_TOKENS still runs the kernel, one more token does not."""
    from kserve_amd import ops

    calls = _spy(monkeypatch)
    K, M = 128, 64
    n = ops.W4_MAX_TOKENS
    x, q, scale = _w4_case(n + 1, K, M, dev)
    a = ops.linear_w4(x[:n], q, scale)
    assert calls == {"skinny_gemm_w4": 1, "dequant_mxfp4_rows": 0}
    b = ops.linear_w4(x, q, scale)
    torch.cuda.synchronize()
    assert calls == {"skinny_gemm_w4": 1, "dequant_mxfp4_rows": 1}
    ref = _ref(x, q, scale)
    torch.testing.assert_close(a.float().cpu(), ref[:n], atol=0.05, rtol=0.05)
    torch.testing.assert_close(b.float().cpu(), ref, atol=0.05, rtol=0.05)


def test_linear_w4_dequant_path_chunks_a_large_weight(dev):
    """The scratch (shared with fp8, sized in bf16 elements) holds half of
    the largest weight seen: that weight goes through the dequant path in
    two row chunks, and forward does not reallocate it."""
    from kserve_amd import ops

    N, K, M = 300, 64, 192
    x, q, scale = _w4_case(N, K, M, dev)
    saved = dict(ops._W8_SCRATCH)
    ops._W8_SCRATCH.clear()
    try:
        ops.reserve_w8_scratch(dev, M, K)
        buf = ops._W8_SCRATCH[x.device]
        assert buf.numel() == (M // 2) * K
        got = ops.linear_w4(x, q, scale)
        torch.cuda.synchronize()
        assert ops._W8_SCRATCH[x.device] is buf  # forward did not allocate
    finally:
        ops._W8_SCRATCH.clear()
        ops._W8_SCRATCH.update(saved)
    torch.testing.assert_close(
        got.float().cpu(), _ref(x, q, scale), atol=0.05, rtol=0.05
    )


# -- 5: engine ---------------------------------------------------------------


def _cfg(enforce_eager=False, num_blocks=128, quantization="mxfp4",
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


def test_mxfp4_graph_matches_eager(dev):
    """Same prompts and lengths as test_graph_matches_eager (identical
    batch shapes on both sides, so token equality is legitimate)."""
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    prompts = [[1, 2, 3, 4, 5], [100, 200, 300], [7, 8, 9, 10]]
    sp = SamplingParams(temperature=0.0, max_tokens=16)

    engine_e = LLMEngine(_cfg(enforce_eager=True))
    down = engine_e.model.layers[0].mlp.down_proj
    assert down.qweight.dtype == torch.uint8
    assert down.qweight.shape == (512, 1024 // 2)
    assert down.weight_scale.shape == (512, 1024 // 32)
    out_e = engine_e.generate(prompts, sp)
    del engine_e
    torch.cuda.empty_cache()

    engine_g = LLMEngine(_cfg(enforce_eager=False))
    out_g = engine_g.generate(prompts, sp)
    toks_e = [o.output_token_ids for o in out_e.values()]
    toks_g = [o.output_token_ids for o in out_g.values()]
    assert all(len(t) == 16 for t in toks_g)
    assert toks_e == toks_g


def test_mxfp4_logits_match_cpu_reference(dev):
    """GPU bf16 prefill (T=33) vs a CPU fp32 model holding the same
    qweight/weight_scale; the criteria of the fp8 test (the error source
    is bf16 compute, not the format)."""
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
        quantization="mxfp4",
    )
    torch.manual_seed(0)
    cpu_model = LlamaForCausalLM(cfg, dtype=torch.float32, device="cpu")
    cpu_model.random_init(seed=5)
    gpu_model = LlamaForCausalLM(cfg, dtype=torch.bfloat16, device="cuda")
    n_codes = 0
    with torch.no_grad():
        for (n1, p1), (n2, p2) in zip(
            gpu_model.named_parameters(), cpu_model.named_parameters()
        ):
            assert n1 == n2
            if p2.dtype == torch.uint8:
                p1.copy_(p2)  # codes and E8M0 scales, bit for bit
                n_codes += 1
            else:
                p1.copy_(p2.to(torch.bfloat16))
    assert n_codes == 2 * 4 * cfg.num_layers

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


def test_mxfp4_engine_dequant_path_prompt(dev):
    """A 300-token prompt prefills through the dequant path (N > 128) in
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


def test_mxfp4_weights_with_fp8_kv(dev):
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


def test_mxfp4_model_memory(dev):
    """The mxfp4 build must allocate less than the bf16 build by at least
    0.6 of the bf16 bytes of the quantized projections: 4.25 bits per
    weight saves 73 %, the shared scratch of half the largest weight
    (counted here) costs 5.5 % on this config, the rest is
    allocator-rounding margin."""
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
            2 * p.numel() for n, p in model.named_parameters()
            if n.endswith("qweight")
        )
        return used, proj

    saved = dict(ops._W8_SCRATCH)
    ops._W8_SCRATCH.clear()  # count the scratch against the mxfp4 build
    try:
        bf16_used, _ = build(None)
        w4_used, proj_elems = build("mxfp4")
    finally:
        ops._W8_SCRATCH.clear()
        ops._W8_SCRATCH.update(saved)
    proj_bf16_bytes = 2 * proj_elems
    print(f"bf16 {bf16_used} B, mxfp4 {w4_used} B, projections {proj_bf16_bytes} B, "
          f"saved {(bf16_used - w4_used) / proj_bf16_bytes:.3f} of them")
    assert proj_elems > 0
    assert bf16_used - w4_used >= 0.6 * proj_bf16_bytes
