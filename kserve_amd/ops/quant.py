"""Weight-only quantization (fp8 W8A16, MXFP4 W4A16): formats and
host-side quantizers.

fp8 format: OCP ``float8_e4m3fn`` codes (never ``fnuz``) with one fp32 scale per
output channel (weight row); ``w ~= float(q) * scale[row]``. Activations
stay bf16, so the only approximation is this one-time rounding of the
weights: the fp8 -> bf16 convert in the kernel is exact (E4M3 fits bf16's
mantissa) and the scale multiplies the fp32 accumulator after the K
reduction (``torch_ref.linear_w8`` / ``wq_gemm.hip``).

MXFP4 format (OCP microscaling), for a weight ``w [M, K]``, ``K % 32 == 0``:

- ``qweight``: ``uint8 [M, K/2]``. Element ``2i`` of a row is in bits 3:0 of
  byte ``i``; element ``2i+1`` is in bits 7:4.
- A 4-bit code is sign (bit 3) plus a 3-bit magnitude index into
  ``{0, 0.5, 1, 1.5, 2, 3, 4, 6}`` (E2M1; no Inf, no NaN).
- ``weight_scale``: ``uint8 [M, K/32]``, E8M0: code ``c`` means
  ``2^(c-127)``; code 255 (NaN) is invalid and refused at load.
- ``w[m][k] ~= e2m1(code[m][k]) * 2^(weight_scale[m][k/32] - 127)``.

The scale is a power of two, so applying it (in the kernel's convert,
``wq_gemm.hip``, or in ``torch_ref.linear_w4``) is exact wherever the
product is a normal bf16; as with fp8 the only approximation is the
one-time rounding of the weights.

The quantizers are plain torch: they run once at load, on whatever device
the shard is on. ``WEIGHT_FORMATS`` at the end describes both formats to the
parallel linear layers (storage shapes, shard -> codes, which op to call).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0  # largest finite e4m3fn magnitude

QUANTIZATION_METHODS = (None, "fp8", "mxfp4")


def check_quantization(name: Optional[str]) -> Optional[str]:
    """Validate a quantization method name (config time)."""
    if name not in QUANTIZATION_METHODS:
        raise ValueError(
            f"unknown quantization {name!r}; supported: None, 'fp8', 'mxfp4'"
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


# ---------------------------------------------------------------- MXFP4 --

MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MAX = 6.0
E8M0_BIAS = 127
E8M0_NAN = 255


def quantize_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [M, K] (bf16/f32), K % 32 == 0 -> (qweight uint8 [M, K/2],
    weight_scale uint8 [M, K/32]).

    Per block of 32: e = floor(log2(amax)) - 2 clamped to [-126, 127] (so
    amax / 2^e is in [4, 8): the top binade of E2M1, saturating above 6);
    an all-zero block gets scale code 127. Elements are w / 2^e clamped to
    [-6, 6] and rounded to the nearest E2M1 value, ties to the even
    mantissa. A value that rounds to zero gets code 0x0, never 0x8, which
    makes quantizing a dequantized weight the identity.
    """
    assert w.dim() == 2, "quantize_mxfp4 expects [out, in]"
    M, K = w.shape
    if K % MXFP4_BLOCK != 0:
        raise ValueError(
            f"mxfp4 needs in_features % {MXFP4_BLOCK} == 0, got {K}"
        )
    wf = w.float().reshape(M, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=2).clamp(max=torch.finfo(torch.float32).max)
    # frexp: amax = m * 2^ex with m in [0.5, 1), so floor(log2) = ex - 1
    _, ex = torch.frexp(amax)
    e = (ex.to(torch.int32) - 3).clamp(-126, 127)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    # ldexp by -e in two exact halves: 2^126 * 6 would overflow in one
    h = torch.div(e, 2, rounding_mode="floor")
    v = torch.ldexp(torch.ldexp(wf, -h[..., None]), -(e - h)[..., None])
    a = v.abs().clamp(max=E2M1_MAX)
    # thresholds are the midpoints; >= where the tie goes up to an even code
    idx = (
        (a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8)
        + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
        + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
        + (a > 5.0).to(torch.uint8)
    )
    sign = ((v < 0) & (idx > 0)).to(torch.uint8) << 3
    codes = (idx | sign).reshape(M, K // 2, 2)
    qweight = codes[..., 0] | (codes[..., 1] << 4)
    scale = (e + E8M0_BIAS).to(torch.uint8)
    return qweight.contiguous(), scale.contiguous()


def dequantize_mxfp4(qweight: torch.Tensor, weight_scale: torch.Tensor,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Table lookup times 2^(scale - 127), rounded once to ``dtype``."""
    M, K2 = qweight.shape
    lut = torch.tensor(
        E2M1_VALUES + tuple(-x for x in E2M1_VALUES),
        dtype=torch.float32, device=qweight.device,
    )
    q = qweight.to(torch.int64)
    vals = lut[torch.stack((q & 0xF, q >> 4), dim=-1)]  # [M, K/2, 2]
    vals = vals.reshape(M, K2 * 2 // MXFP4_BLOCK, MXFP4_BLOCK)
    ex = weight_scale.to(torch.int32) - E8M0_BIAS
    return torch.ldexp(vals, ex[..., None]).reshape(M, K2 * 2).to(dtype)


def check_mxfp4_scale(scale: torch.Tensor, out_features: int,
                      in_features: int, name: str = "weight_scale"
                      ) -> torch.Tensor:
    """Checkpoint E8M0 scale (uint8 or float8_e8m0fnu) -> uint8
    [out_features, in_features / 32]; refuses a wrong shape and code 255."""
    if scale.dtype != torch.uint8:
        e8m0 = getattr(torch, "float8_e8m0fnu", None)
        if e8m0 is None or scale.dtype != e8m0:
            raise ValueError(
                f"{name}: mxfp4 scales must be uint8 or float8_e8m0fnu, "
                f"got {scale.dtype}"
            )
        scale = scale.view(torch.uint8)
    want = (out_features, in_features // MXFP4_BLOCK)
    if in_features % MXFP4_BLOCK != 0 or tuple(scale.shape) != want:
        raise ValueError(
            f"{name} has shape {tuple(scale.shape)}, expected {want} "
            f"(one E8M0 scale per {MXFP4_BLOCK} input features)"
        )
    if bool((scale == E8M0_NAN).any()):
        raise ValueError(f"{name} holds the E8M0 NaN code 255")
    return scale


# ------------------------------------------- what a layer needs to know --


def _fp8_shard(w: torch.Tensor, scale: Optional[torch.Tensor], dev):
    if w.dtype == FP8_DTYPE:
        if scale is None:
            raise ValueError("fp8 checkpoint weight without weight_scale")
        return w.to(dev), scale.float().to(dev)
    if w.dtype == torch.uint8:
        raise ValueError(
            "an mxfp4 checkpoint cannot be loaded with quantization='fp8'"
        )
    return quantize_fp8_per_channel(w.to(dev))


def _mxfp4_shard(w: torch.Tensor, scale: Optional[torch.Tensor], dev):
    if w.dtype == torch.uint8:
        if scale is None:
            raise ValueError("mxfp4 checkpoint weight without weight_scale")
        scale = check_mxfp4_scale(scale, w.shape[0], w.shape[1] * 2)
        return w.to(dev), scale.to(dev)
    if w.dtype == FP8_DTYPE:
        raise ValueError(
            "an fp8 checkpoint cannot be loaded with quantization='mxfp4'"
        )
    return quantize_mxfp4(w.to(dev))


@dataclass(frozen=True)
class WeightFormat:
    """How a linear layer stores and runs one quantized format: ``qweight``
    is ``code_dtype [out, in / per_byte]``; ``weight_scale`` is
    ``scale_dtype [out]``, or ``[out, in / block]`` for a block format."""

    name: str  # the ``quantization=`` value
    code_dtype: torch.dtype
    scale_dtype: torch.dtype
    per_byte: int  # input features per qweight element
    block: Optional[int]  # input features per scale; None: one per row
    linear: str  # the ``kserve_amd.ops`` function that applies it
    # (already-sliced shard, its checkpoint scale slice or None, device) ->
    # (codes, scale) on device. A bf16/f32 shard is quantized here, after
    # slicing, so scales are per rank; a pre-quantized one is checked and
    # moved; the other format's codes are refused.
    shard_to_codes: Callable

    def storage_shapes(self, out_features: int, in_features: int):
        """Shapes of (qweight, weight_scale) for a logical [out, in]."""
        if self.block is None:
            return (out_features, in_features // self.per_byte), (out_features,)
        if in_features % self.block != 0:
            raise ValueError(
                f"{self.name} needs the per-rank in_features ({in_features}) "
                f"to be a multiple of {self.block}"
            )
        return (
            (out_features, in_features // self.per_byte),
            (out_features, in_features // self.block),
        )

    def logical_shape(self, qweight: torch.Tensor) -> Tuple[int, int]:
        """[out, in] of the weight a stored ``qweight`` stands for."""
        return qweight.shape[0], qweight.shape[1] * self.per_byte


WEIGHT_FORMATS = {
    "fp8": WeightFormat(
        "fp8", FP8_DTYPE, torch.float32, per_byte=1, block=None,
        linear="linear_w8", shard_to_codes=_fp8_shard,
    ),
    "mxfp4": WeightFormat(
        "mxfp4", torch.uint8, torch.uint8, per_byte=2, block=MXFP4_BLOCK,
        linear="linear_w4", shard_to_codes=_mxfp4_shard,
    ),
}
