"""Custom op dispatch: CDNA4 HIP kernels on GPU, torch reference on CPU.

Policy (round-end harness contract): GPU tensors MUST run the native
extension — if ``kserve_amd_C`` is missing on a CUDA/ROCm device the op
raises ``NoNativeExtension`` instead of silently falling back to eager
torch. CPU tensors use the fp32 torch reference (tests, engine logic).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from kserve_amd.errors import NoNativeExtension
from kserve_amd.ops import torch_ref

_C = None
_IMPORT_ERROR: Optional[str] = None
try:
    import kserve_amd_C as _C  # built in-tree by setup.py (travels to GPU box)
except ImportError as e:  # pragma: no cover - exercised on GPU box
    _IMPORT_ERROR = str(e)


def has_native() -> bool:
    return _C is not None


def _native(op: str):
    if _C is None:
        raise NoNativeExtension(op, f"(import error: {_IMPORT_ERROR})")
    return _C


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        out = torch.empty_like(x)
        _native("rms_norm").rms_norm(out, x, weight, eps)
        return out
    return torch_ref.rms_norm(x, weight, eps)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """In-place on GPU: x <- rmsnorm(x+residual), residual <- x+residual."""
    if x.is_cuda:
        _native("fused_add_rms_norm").fused_add_rms_norm(x, residual, weight, eps)
        return x, residual
    return torch_ref.fused_add_rms_norm(x, residual, weight, eps)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        d = x.shape[-1] // 2
        out = torch.empty(
            (*x.shape[:-1], d), dtype=x.dtype, device=x.device
        )
        _native("silu_and_mul").silu_and_mul(out, x)
        return out
    return torch_ref.silu_and_mul(x)


def rotary_embedding(
    positions: torch.Tensor,
    q: torch.Tensor,
    k: torch.Tensor,
    cos_sin_cache: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Neox-style RoPE. GPU path mutates q/k in place and returns them."""
    if q.is_cuda:
        _native("rotary_embedding").rotary_embedding(positions, q, k, cos_sin_cache)
        return q, k
    return torch_ref.rotary_embedding(positions, q, k, cos_sin_cache)


def reshape_and_cache(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    if k.is_cuda:
        _native("reshape_and_cache").reshape_and_cache(
            k, v, k_cache, v_cache, slot_mapping
        )
        return
    torch_ref.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping)


def paged_attention_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    context_lens: torch.Tensor,
    scale: float,
    out: Optional[torch.Tensor] = None,
    window: int = 0,
) -> torch.Tensor:
    """Single-token attention of each sequence against its paged context.

    block_tables [S, max_blocks] may be wider than any sequence needs; only
    the first ceil(context_lens / block_size) entries of a row select pages,
    the rest must still be valid block ids. Cache contract: the kernels load
    whole pages and give slots at or past context_lens (and before the
    window) weight 0, so the result is exact for ANY FINITE stale data in
    those slots and undefined (NaN) for non-finite data. The cache must
    never hold non-finite values the model did not write; the engine
    allocates it zero-filled (ModelRunner._kv_allocator)."""
    if q.is_cuda:
        if out is None:
            out = torch.empty_like(q)
        _native("paged_attention_decode").paged_attention_decode(
            out, q, k_cache, v_cache, block_tables, context_lens, scale,
            window,
        )
        return out
    return torch_ref.paged_attention_decode(
        q, k_cache, v_cache, block_tables, context_lens, scale,
        window=window,
    )


def flash_prefill_varlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    if q.is_cuda:
        out = torch.empty_like(q)
        _native("flash_prefill").flash_prefill_varlen(
            out, q, k, v, cu_seqlens, int(max_seqlen), scale,
            causal=True, window=window,
        )
        return out
    return torch_ref.flash_prefill_varlen(
        q, k, v, cu_seqlens, scale, causal=True, window=window
    )


def context_attention_varlen(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    context_lens: torch.Tensor,
    max_q_len: int,
    scale: float,
    window: int = 0,
) -> torch.Tensor:
    """Prefill attention against the paged cache (chunked prefill): the
    chunk's KV must already be written to the cache; queries attend causally
    to the whole per-seq context (bounded below by the sliding window when
    window > 0).

    Cache contract, as for paged_attention_decode: exact for any finite
    stale data in slots at or past context_lens and in pages behind unused
    block-table entries (which must be valid ids), undefined for non-finite
    data there; the cache must never hold non-finite values the model did
    not write."""
    if q.is_cuda:
        out = torch.empty_like(q)
        _native("context_prefill").context_prefill_varlen(
            out, q, k_cache, v_cache, block_tables, context_lens,
            cu_seqlens_q, int(max_q_len), scale, window
        )
        return out
    return torch_ref.context_attention_varlen(
        q, k_cache, v_cache, block_tables, cu_seqlens_q, context_lens, scale,
        window=window,
    )


def greedy_sample(logits: torch.Tensor) -> torch.Tensor:
    if logits.is_cuda:
        out = torch.empty(
            logits.shape[0], dtype=torch.int64, device=logits.device
        )
        _native("greedy_sample").greedy_sample(out, logits)
        return out
    return torch_ref.greedy_sample(logits)


def random_sample(
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_p: torch.Tensor,
    top_k: torch.Tensor,
    seeds: Optional[torch.Tensor] = None,
    generator: Optional[torch.Generator] = None,
    min_p: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Temperature/top-k/top-p/min-p sampling.

    GPU: one fused HIP kernel. Plain temperature sampling is Gumbel-max;
    top-k/top-p use a bf16 radix-histogram select (exact k-th value / mass
    threshold, no sort) followed by Gumbel-max over the surviving set.
    min_p (rare) routes to the fp32 sort path.
    """
    has_min_p = min_p is not None and bool((min_p > 0).any())
    if logits.is_cuda and seeds is not None and not has_min_p:
        out = torch.empty(
            logits.shape[0], dtype=torch.int64, device=logits.device
        )
        needs_trunc = bool((top_p < 1.0).any()) or bool((top_k > 0).any())
        if needs_trunc:
            _native("random_sample").topk_topp_sample(
                out, logits, temperatures, top_p, top_k.to(torch.int32), seeds
            )
        else:
            _native("random_sample").gumbel_sample(
                out, logits, temperatures, top_k.to(torch.int32), seeds
            )
        return out
    # min-p (or CPU): fp32 sort path
    return torch_ref.random_sample(
        logits, temperatures, top_p, top_k, generator=generator, min_p=min_p
    )


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GEMM dispatch: custom MFMA skinny-GEMM for decode-sized batches
    (weight-streaming regime where hipBLASLt underperforms ~4x on gfx950 —
    see tools/gemm_bench.py), hipBLASLt via F.linear otherwise."""
    import torch.nn.functional as F

    # measured crossover (tools/gemm_bench.py on MI355X): the custom kernel
    # beats hipBLASLt only for small token batches on qkv/o-sized shapes;
    # hipBLASLt keeps the wide-M / large-K / large-N shapes.
    if (
        _C is not None
        and x.is_cuda
        and bias is None
        and x.dim() == 2
        and 0 < x.shape[0] <= 64
        and weight.shape[0] % 64 == 0
        and weight.shape[0] <= 8192
        and weight.shape[1] % 64 == 0
        and weight.shape[1] <= 8192
        and x.stride(1) == 1
    ):
        out = torch.empty(
            (x.shape[0], weight.shape[0]), dtype=x.dtype, device=x.device
        )
        _C.skinny_gemm(out, x, weight)
        return out
    return F.linear(x, weight, bias)


# Largest token batch ops.linear_w8 sends to the fp8-weight skinny GEMM;
# above it the weight is dequantized into the scratch buffer and hipBLASLt
# runs the GEMM. The kernel's own limit is 256; 128 is the largest batch at
# which it beat dequant + hipBLASLt on all four Llama-3-8B projection shapes
# (A/B table: profiles/w8_gemm.md, tools/gemm_bench.py --w8).
W8_MAX_TOKENS = 128

# One bf16 dequant scratch per device, shared by every quantized layer
# (same-stream ordering: a GEMM has consumed it before the next dequant
# overwrites it). It holds HALF of the largest quantized weight: the
# dequant path runs that weight in two row chunks, every smaller one in one
# or two, so the scratch costs a quarter of the bytes the largest weight
# saved instead of all of them.
_W8_SCRATCH: dict = {}


def w8_scratch_numel(out_features: int, in_features: int) -> int:
    return -(-out_features // 2) * in_features


def reserve_w8_scratch(device, out_features: int, in_features: int) -> None:
    """Make the per-device dequant scratch large enough for a quantized
    [out_features, in_features] weight. Layers call this when they
    quantize/load a weight, so forward (and with it hipGraph capture) never
    allocates."""
    device = torch.device(device)
    if device.type != "cuda":
        return
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    numel = w8_scratch_numel(out_features, in_features)
    buf = _W8_SCRATCH.get(device)
    if buf is None or buf.numel() < numel:
        _W8_SCRATCH[device] = None  # drop the old one before growing
        _W8_SCRATCH[device] = torch.empty(
            numel, dtype=torch.bfloat16, device=device
        )


def _w8_scratch(device, out_features: int, in_features: int) -> torch.Tensor:
    buf = _W8_SCRATCH.get(device)
    if buf is None or buf.numel() < w8_scratch_numel(out_features, in_features):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "dequant scratch too small during graph capture; "
                "call ops.reserve_w8_scratch when the weight is quantized"
            )
        reserve_w8_scratch(device, out_features, in_features)
        buf = _W8_SCRATCH[device]
    return buf


def _linear_wq(
    name: str,
    x: torch.Tensor,
    qweight: torch.Tensor,
    scale: torch.Tensor,
    bias: Optional[torch.Tensor],
    *,
    K: int,  # logical in_features of qweight
    k_multiple: int,  # the kernel's K step
    max_tokens: int,
    gemm: str,  # binding names
    dequant: str,
    reference,  # CPU path
) -> torch.Tensor:
    """What linear_w8 and linear_w4 share. GPU: decode-sized batches run the
    format's MFMA skinny GEMM (weights cross HBM once, as codes); everything
    else (prefill, large batches, odd shapes) dequantizes into the shared
    scratch, in row chunks, and runs hipBLASLt."""
    if not x.is_cuda:
        return reference(x, qweight, scale, bias)
    C = _native(name)
    import torch.nn.functional as F

    M = qweight.shape[0]
    if (
        x.dim() == 2
        and 0 < x.shape[0] <= max_tokens
        and M % 64 == 0
        and K % k_multiple == 0
        and x.dtype == torch.bfloat16
        and x.stride(1) == 1
        and x.stride(0) % 8 == 0
        and x.data_ptr() % 16 == 0
    ):
        out = torch.empty((x.shape[0], M), dtype=x.dtype, device=x.device)
        getattr(C, gemm)(out, x, qweight, scale)
        if bias is not None:
            out += bias
        return out
    if x.dtype != torch.bfloat16:
        raise TypeError(f"{name} on GPU needs bf16 activations, got {x.dtype}")
    buf = _w8_scratch(x.device, M, K)
    rows = min(M, buf.numel() // K)
    parts = []
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        w = buf[: (r1 - r0) * K].view(r1 - r0, K)
        getattr(C, dequant)(w, qweight[r0:r1], scale[r0:r1])
        parts.append(
            F.linear(x, w, None if bias is None else bias[r0:r1])
        )
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)


def linear_w8(
    x: torch.Tensor,
    qweight: torch.Tensor,
    scale: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Weight-only fp8 linear: (x @ qweight^T) * scale (+ bias).

    qweight [M, K] float8_e4m3fn, scale [M] f32 (kserve_amd.ops.quant).
    """
    return _linear_wq(
        "linear_w8", x, qweight, scale, bias,
        K=qweight.shape[1], k_multiple=64, max_tokens=W8_MAX_TOKENS,
        gemm="skinny_gemm_w8", dequant="dequant_fp8_rows",
        reference=torch_ref.linear_w8,
    )


# Largest token batch ops.linear_w4 sends to the MXFP4-weight skinny GEMM;
# above it the weight is dequantized into the shared scratch and hipBLASLt
# runs the GEMM. Measured at N = 1/16/64/128 on the four Llama-3-8B
# projection shapes, the kernel beat dequant + hipBLASLt in every cell
# (1.8-5.2x), so 128, the largest measured N and the kernel's own limit
# (its X tile fills 64 KB of LDS there), is the value (A/B table:
# profiles/w4_gemm.md, tools/gemm_bench.py --w4).
W4_MAX_TOKENS = 128


def linear_w4(
    x: torch.Tensor,
    qweight: torch.Tensor,
    weight_scale: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Weight-only MXFP4 linear: x @ dequant(qweight, weight_scale)^T (+ bias).

    qweight uint8 [M, K/2], weight_scale uint8 [M, K/32]
    (kserve_amd.ops.quant); the weights cross HBM as 4.25 bits each. The
    dequant scratch is the one linear_w8 uses.
    """
    return _linear_wq(
        "linear_w4", x, qweight, weight_scale, bias,
        K=qweight.shape[1] * 2, k_multiple=128, max_tokens=W4_MAX_TOKENS,
        gemm="skinny_gemm_w4", dequant="dequant_mxfp4_rows",
        reference=torch_ref.linear_w4,
    )


def layer_norm(x, weight, bias, eps: float):
    if x.is_cuda:
        out = torch.empty_like(x)
        _native("layer_norm").layer_norm(out, x, weight, bias, eps)
        return out
    return torch_ref.layer_norm(x, weight, bias, eps)


def fused_add_layer_norm(x, residual, weight, bias, eps: float):
    if x.is_cuda:
        out = torch.empty_like(x)
        _native("fused_add_layer_norm").fused_add_layer_norm(
            out, x, residual, weight, bias, eps
        )
        return out
    return torch_ref.fused_add_layer_norm(x, residual, weight, bias, eps)


def gelu(x):
    if x.is_cuda:
        out = torch.empty_like(x)
        _native("gelu").gelu(out, x)
        return out
    return torch_ref.gelu(x)


def flash_attn_varlen(q, k, v, cu_seqlens, max_seqlen, scale, causal=True):
    """Bidirectional-capable variant (encoder models)."""
    if q.is_cuda:
        out = torch.empty_like(q)
        _native("flash_prefill").flash_prefill_varlen(
            out, q, k, v, cu_seqlens, int(max_seqlen), scale, causal
        )
        return out
    return torch_ref.flash_prefill_varlen(q, k, v, cu_seqlens, scale, causal=causal)


def topk_topp_sample_into(
    out: torch.Tensor,
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_p: torch.Tensor,
    top_k: torch.Tensor,
    seeds: torch.Tensor,
) -> torch.Tensor:
    """Destination-passing form of the fused sampler for hipGraph capture
    (static out buffer, per-row device seeds; see model_runner
    _ensure_sampled_graph). GPU-only."""
    _native("random_sample").topk_topp_sample(
        out, logits, temperatures, top_p,
        top_k if top_k.dtype == torch.int32 else top_k.to(torch.int32),
        seeds,
    )
    return out


def _check_rows(name: str, t: torch.Tensor, dtype, n: int, device) -> None:
    if (
        t.dtype != dtype
        or t.dim() != 1
        or t.shape[0] != n
        or not t.is_contiguous()
        or t.device != device
    ):
        raise ValueError(
            f"{name} must be a contiguous {dtype} [{n}] tensor on {device}, "
            f"got {t.dtype} {tuple(t.shape)} on {t.device}"
        )


def topk_topp_minp_sample_into(
    out: torch.Tensor,
    logits: torch.Tensor,
    temperatures: torch.Tensor,
    top_p: torch.Tensor,
    top_k: torch.Tensor,
    min_p: torch.Tensor,
    seeds: torch.Tensor,
    generator: Optional[torch.Generator] = None,
) -> torch.Tensor:
    """``topk_topp_sample_into`` with a per-row min-p (fp32 [S], <= 0 off):
    an element is also dropped when its probability under the untruncated
    softmax(logits / T) is below ``min_p`` times the maximum's; the mask is
    OR-ed with top-k and top-p and the row maximum always survives. Device
    tensors only (runs under capture); CPU tensors take the sort reference,
    which draws from ``generator`` instead of ``seeds``."""
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous [S, V] tensor")
    s, dev = logits.shape[0], logits.device
    _check_rows("out", out, torch.int64, s, dev)
    _check_rows("temperatures", temperatures, torch.float32, s, dev)
    _check_rows("top_p", top_p, torch.float32, s, dev)
    _check_rows("top_k", top_k, torch.int32, s, dev)
    _check_rows("min_p", min_p, torch.float32, s, dev)
    _check_rows("seeds", seeds, torch.int64, s, dev)
    if logits.is_cuda:
        if logits.dtype != torch.bfloat16:
            raise TypeError(f"logits must be bf16 on GPU, got {logits.dtype}")
        _native("topk_topp_minp_sample").topk_topp_minp_sample(
            out, logits, temperatures, top_p, top_k, min_p, seeds
        )
        return out
    out.copy_(
        torch_ref.topk_topp_minp_sample(
            logits, temperatures, top_p, top_k, min_p, generator=generator
        )
    )
    return out


def logit_process(
    logits: torch.Tensor,
    counts: torch.Tensor,
    row_slot: torch.Tensor,
    presence: torch.Tensor,
    frequency: torch.Tensor,
    repetition: torch.Tensor,
    bias_ids: torch.Tensor,
    bias_vals: torch.Tensor,
    bias_len: torch.Tensor,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Apply logit_bias and then the presence / frequency / repetition
    penalties to logits [S, V], row s from slot ``row_slot[s]`` of the
    per-request state (``counts`` int32 [slots, V], ``bias_ids`` int32 /
    ``bias_vals`` fp32 [slots, max_bias] with ``bias_len`` int32 [slots]
    valid entries, ids unique within a slot).

    Per element: a bias entry gives ``x = bf16(float(x) + bias)``; then, if
    the token's count is positive, ``v = float(x)``, ``v = v / rep if v > 0
    else v * rep`` when ``rep != 1``, ``x = bf16(v - presence - frequency *
    count)``. Elements with neither and rows whose slot is outside
    [0, slots) (-1 marks rows without processors and graph padding) keep
    their bits. ``out=logits`` works in place; the default allocates.
    Device tensors only (runs under capture)."""
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous [S, V] tensor")
    s, v = logits.shape
    dev = logits.device
    if (
        counts.dtype != torch.int32
        or counts.dim() != 2
        or counts.shape[1] != v
        or not counts.is_contiguous()
        or counts.device != dev
    ):
        raise ValueError(
            f"counts must be a contiguous int32 [slots, {v}] tensor on {dev}"
        )
    slots = counts.shape[0]
    _check_rows("row_slot", row_slot, torch.int32, s, dev)
    _check_rows("presence", presence, torch.float32, s, dev)
    _check_rows("frequency", frequency, torch.float32, s, dev)
    _check_rows("repetition", repetition, torch.float32, s, dev)
    _check_rows("bias_len", bias_len, torch.int32, slots, dev)
    if (
        bias_ids.dtype != torch.int32
        or bias_vals.dtype != torch.float32
        or bias_ids.dim() != 2
        or bias_ids.shape[0] != slots
        or bias_vals.shape != bias_ids.shape
        or not bias_ids.is_contiguous()
        or not bias_vals.is_contiguous()
        or bias_ids.device != dev
        or bias_vals.device != dev
    ):
        raise ValueError(
            "bias_ids (int32) and bias_vals (fp32) must be contiguous "
            f"[{slots}, max_bias] tensors on {dev}"
        )
    if out is not None and out is not logits:
        if (
            out.shape != logits.shape
            or out.dtype != logits.dtype
            or out.device != dev
            or not out.is_contiguous()
        ):
            raise ValueError("out must match logits in shape, dtype, device")
    if not logits.is_cuda:
        return torch_ref.logit_process(
            logits, counts, row_slot, presence, frequency, repetition,
            bias_ids, bias_vals, bias_len, out=out,
        )
    if logits.dtype != torch.bfloat16:
        raise TypeError(f"logits must be bf16 on GPU, got {logits.dtype}")
    if out is None:
        out = torch.empty_like(logits)
    _native("logit_process").logit_process(
        out, logits, counts, row_slot, presence, frequency, repetition,
        bias_ids, bias_vals, bias_len,
    )
    return out


def token_count_add(
    counts: torch.Tensor, slot: torch.Tensor, token: torch.Tensor
) -> None:
    """``counts[slot[j], token[j]] += 1`` for every j (int32 slots, int64
    tokens, as the samplers return them). Pairs with a slot outside
    [0, slots) or a token outside [0, V) are skipped; duplicates all count.
    Device tensors only (runs under capture)."""
    dev = counts.device
    if counts.dtype != torch.int32 or counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 [slots, V] tensor")
    n = slot.numel()
    _check_rows("slot", slot, torch.int32, n, dev)
    _check_rows("token", token, torch.int64, n, dev)
    if counts.is_cuda:
        _native("token_count_add").token_count_add(counts, slot, token)
        return
    torch_ref.token_count_add(counts, slot, token)


def lora_shrink(
    x: torch.Tensor,
    a_stack: torch.Tensor,
    ranks: torch.Tensor,
    slot_idx: torch.Tensor,
) -> torch.Tensor:
    """Batched multi-LoRA shrink (BGMV): tmp[t, :rr] = x[t] @ A[slot_t, :rr]^T.

    x [T, K] bf16 rows (row stride allowed), a_stack [S, R, K] bf16, ranks
    [S] int32, slot_idx [T] int32 on the device; rr = round_up(ranks[slot],
    8). Returns fp32 [T, R]; on the GPU, rows whose slot is outside [0, S)
    and columns at or past rr are left unwritten (lora_expand_add reads
    neither)."""
    if x.is_cuda:
        tmp = torch.empty(
            (x.shape[0], a_stack.shape[1]), dtype=torch.float32, device=x.device
        )
        _native("lora_shrink").lora_shrink(tmp, x, a_stack, ranks, slot_idx)
        return tmp
    return torch_ref.lora_shrink(x, a_stack, ranks, slot_idx)


def lora_expand_add(
    y: torch.Tensor,
    tmp: torch.Tensor,
    b_stack: torch.Tensor,
    scale: torch.Tensor,
    ranks: torch.Tensor,
    slot_idx: torch.Tensor,
    out_offset: int = 0,
) -> torch.Tensor:
    """Batched multi-LoRA expand, in place:
    y[t, off:off+N] += scale[slot_t] * tmp[t, :rr] @ B[slot_t, :, :rr]^T,
    fp32 accumulate, rounded once. y may be a strided view of a wider row;
    columns outside [off, off+N) and rows whose slot is outside [0, S) keep
    their bits."""
    if y.is_cuda:
        _native("lora_expand_add").lora_expand_add(
            y, tmp, b_stack, scale, ranks, slot_idx, int(out_offset)
        )
        return y
    return torch_ref.lora_expand_add(
        y, tmp, b_stack, scale, ranks, slot_idx, out_offset
    )


# -- KV export / import (prefill-decode disaggregation) ----------------------

# device table of the 2L cache base pointers (K0, V0, K1, V1, ...), built the
# first time a pool is exported from or imported into, keyed by the pointers
_KV_BASES: dict = {}


def _kv_bases(kv_caches) -> torch.Tensor:
    ptrs = tuple(t.data_ptr() for kv in kv_caches for t in kv)
    table = _KV_BASES.get(ptrs)
    if table is None:
        if len(_KV_BASES) >= 8:
            _KV_BASES.clear()
        table = torch.tensor(
            ptrs, dtype=torch.int64, device=kv_caches[0][0].device
        )
        _KV_BASES[ptrs] = table
    return table


def _check_kv_transfer_args(kv_caches, block_ids, unique: bool):
    """Host-side validation shared by both devices; the kernels trust the
    ids. Returns the ids as a list of ints."""
    if not kv_caches:
        raise ValueError("kv_caches is empty")
    k0 = kv_caches[0][0]
    for k, v in kv_caches:
        for t in (k, v):
            if t.shape != k0.shape or t.dtype != k0.dtype:
                raise ValueError("all layers must share one shape and dtype")
    ids = [int(b) for b in block_ids]
    num_blocks = k0.shape[0]
    for b in ids:
        if not 0 <= b < num_blocks:
            raise ValueError(
                f"block id {b} outside [0, {num_blocks})"
            )
    if unique and len(set(ids)) != len(ids):
        raise ValueError("duplicate block id in a scatter")
    return ids


def kv_gather_pages(
    kv_caches,
    block_ids,
    num_tokens: int,
    out_dtype: Optional[torch.dtype] = None,
) -> torch.Tensor:
    """Gather pages ``block_ids`` (a host list) of every layer's K and V
    into one contiguous [L, 2, n, Hkv, block_size, D] tensor on the pool's
    device, in one launch. Slots at position ``j*block_size + s >=
    num_tokens`` are zero bytes, so nothing a previous owner of the last
    page left behind travels. ``out_dtype=torch.float8_e4m3fn`` on a bf16
    pool converts exactly as ``reshape_and_cache`` does for an fp8 pool;
    fp8 -> bf16 is refused."""
    ids = _check_kv_transfer_args(kv_caches, block_ids, unique=False)
    k0 = kv_caches[0][0]
    out_dtype = out_dtype or k0.dtype
    if out_dtype != k0.dtype and not (
        k0.dtype == torch.bfloat16 and out_dtype == torch.float8_e4m3fn
    ):
        raise ValueError(
            f"cannot export a {k0.dtype} pool as {out_dtype}: only bf16 -> "
            "fp8_e4m3 converts"
        )
    if not 0 <= num_tokens <= len(ids) * k0.shape[2]:
        raise ValueError(
            f"num_tokens {num_tokens} outside the {len(ids)} listed pages"
        )
    if not k0.is_cuda:
        return torch_ref.kv_gather_pages(kv_caches, ids, num_tokens, out_dtype)
    out = torch.empty(
        (len(kv_caches), 2, len(ids), *k0.shape[1:]),
        dtype=out_dtype, device=k0.device,
    )
    if ids:
        _native("kv_gather_pages").kv_gather_pages(
            out,
            [t for kv in kv_caches for t in kv],
            _kv_bases(kv_caches),
            torch.tensor(ids, dtype=torch.int32).to(k0.device),
            int(num_tokens),
        )
    return out


def kv_scatter_pages(kv_caches, block_ids, src: torch.Tensor) -> None:
    """Write ``src`` ([L, 2, n, Hkv, block_size, D] in the pool's dtype, or
    the same bytes as uint8) into pages ``block_ids`` (a host list, no
    duplicates) of every layer's K and V: whole pages, nothing else."""
    ids = _check_kv_transfer_args(kv_caches, block_ids, unique=True)
    k0 = kv_caches[0][0]
    if src.dtype != k0.dtype and src.dtype != torch.uint8:
        raise ValueError(
            f"payload dtype {src.dtype} does not match the pool's {k0.dtype}"
        )
    want = len(kv_caches) * 2 * len(ids) * k0[0].numel() * k0.element_size()
    if src.numel() * src.element_size() != want:
        raise ValueError(
            f"payload holds {src.numel() * src.element_size()} bytes, the "
            f"listed pages need {want}"
        )
    if src.device != k0.device or not src.is_contiguous():
        raise ValueError("src must be contiguous and on the pool's device")
    if not ids:
        return
    if not k0.is_cuda:
        torch_ref.kv_scatter_pages(kv_caches, ids, src)
        return
    _native("kv_scatter_pages").kv_scatter_pages(
        [t for kv in kv_caches for t in kv],
        _kv_bases(kv_caches),
        torch.tensor(ids, dtype=torch.int32).to(k0.device),
        src.view(k0.dtype),
    )
