"""Weight-only fp8 quantization (W8A16): format and host-side quantizer.

Format: OCP ``float8_e4m3fn`` codes (never ``fnuz``) with one fp32 scale per
output channel (weight row); ``w ~= float(q) * scale[row]``. Activations
stay bf16, so the only approximation is this one-time rounding of the
weights: the fp8 -> bf16 convert in the kernel is exact (E4M3 fits bf16's
mantissa) and the scale multiplies the fp32 accumulator after the K
reduction (``torch_ref.linear_w8`` / ``w8_gemm.hip``).

The quantizer is plain torch: it runs once at load, on whatever device the
shard is on.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0  # largest finite e4m3fn magnitude

QUANTIZATION_METHODS = (None, "fp8")


def check_quantization(name: Optional[str]) -> Optional[str]:
    """Validate a quantization method name (config time)."""
    if name not in QUANTIZATION_METHODS:
        raise ValueError(
            f"unknown quantization {name!r}; supported: None, 'fp8'"
        )
    return name


def quantize_fp8_per_channel(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [M, K] (bf16/f32) -> (q [M, K] float8_e4m3fn, scale [M] f32).

    scale = rowwise absmax / 448 (1.0 for an all-zero row). The clamp is
    required: casting an out-of-range value to float8_e4m3fn yields NaN,
    not the saturated 448.
    """
    assert w.dim() == 2, "quantize_fp8_per_channel expects [out, in]"
    wf = w.float()
    absmax = wf.abs().amax(dim=1)
    scale = absmax / FP8_MAX
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return q, scale


def dequantize_fp8(q: torch.Tensor, scale: torch.Tensor,
                   dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """float(q) * scale[row], rounded once to ``dtype``."""
    return (q.float() * scale.float()[:, None]).to(dtype)


def expand_scale(scale: torch.Tensor, out_features: int) -> torch.Tensor:
    """Checkpoint weight_scale (scalar, [1], [M] or [M, 1]) -> f32 [M]."""
    s = scale.float().reshape(-1)
    if s.numel() == 1:
        return s.expand(out_features).contiguous()
    if s.numel() != out_features:
        raise ValueError(
            f"weight_scale has {s.numel()} elements, expected 1 or "
            f"{out_features} (block-wise scales are not supported)"
        )
    return s.contiguous()
