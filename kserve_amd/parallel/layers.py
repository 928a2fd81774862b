"""Tensor-parallel linear layers (Megatron-style sharding, fresh code).

Column-parallel: weight rows (output features) sharded; no comm on forward.
Row-parallel: weight cols (input features) sharded; sum-all-reduce on output.
The GEMMs themselves go through torch.nn.functional.linear — on ROCm that is
hipBLASLt, the sanctioned library path for plain GEMMs; fused hot ops are the
hand-written HIP kernels in kserve_amd/ops.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from kserve_amd import ops
from kserve_amd.ops import quant
from kserve_amd.parallel import comm


def _divide(a: int, b: int) -> int:
    assert a % b == 0, f"{a} not divisible by {b}"
    return a // b


class _QuantLinearBase(nn.Module):
    """Weight storage shared by the parallel linears.

    quantization=None: a ``weight`` parameter in the model dtype.
    quantization="fp8": ``qweight`` (float8_e4m3fn) + ``weight_scale``
    (f32 [out_local]) INSTEAD of ``weight`` — the layer never holds both
    copies (kserve_amd.ops.quant has the format).
    quantization="mxfp4": ``qweight`` (uint8 [out_local, in_local/2], two
    E2M1 codes per byte) + ``weight_scale`` (uint8 [out_local,
    in_local/32], E8M0), again instead of ``weight``.
    """

    def _alloc_weight(
        self, out_local: int, in_local: int, dtype: torch.dtype,
        quantization: Optional[str],
    ) -> None:
        self.quantization = quant.check_quantization(quantization)
        # None, or the quant.WeightFormat of qweight/weight_scale
        self.weight_format = quant.WEIGHT_FORMATS.get(self.quantization)
        fmt = self.weight_format
        if fmt is not None:
            qshape, sshape = fmt.storage_shapes(out_local, in_local)
            self.qweight = nn.Parameter(
                torch.empty(qshape, dtype=fmt.code_dtype), requires_grad=False
            )
            self.weight_scale = nn.Parameter(
                torch.empty(sshape, dtype=fmt.scale_dtype), requires_grad=False
            )
        else:
            self.weight = nn.Parameter(
                torch.empty(out_local, in_local, dtype=dtype),
                requires_grad=False,
            )

    def _store_weight(self, pieces, scales=None) -> None:
        """Store this rank's shard, given as row-blocks that are
        concatenated along the output dim (fused QKV / gate+up). ``scales``
        are the matching slices of a pre-quantized checkpoint's scales."""
        scales = scales or [None] * len(pieces)
        fmt = self.weight_format
        if fmt is not None:
            dev = self.qweight.device
            qs = [fmt.shard_to_codes(w, s, dev) for w, s in zip(pieces, scales)]
            self.qweight.data.copy_(torch.cat([q for q, _ in qs], dim=0))
            self.weight_scale.data.copy_(torch.cat([s for _, s in qs], dim=0))
            # one scratch for every format, sized in bf16 elements
            ops.reserve_w8_scratch(dev, *fmt.logical_shape(self.qweight))
            return
        dt = self.weight.dtype

        def to_dt(w, s):
            if w.dtype == quant.FP8_DTYPE:
                return quant.dequantize_fp8(w, s, dt)
            if w.dtype == torch.uint8:
                if s is None:
                    raise ValueError(
                        "mxfp4 checkpoint weight without weight_scale"
                    )
                s = quant.check_mxfp4_scale(s, w.shape[0], w.shape[1] * 2)
                return quant.dequantize_mxfp4(w, s, dt)
            return w.to(dt)

        ws = [to_dt(w, s) for w, s in zip(pieces, scales)]
        self.weight.data.copy_(torch.cat(ws, dim=0))

    @torch.no_grad()
    def random_init_weight(self, std: float, generator) -> None:
        """normal_ does not exist for fp8 or packed fp4 codes: draw a
        temporary in bf16 on the layer's device and quantize it."""
        if self.weight_format is not None:
            tmp = torch.empty(
                self.weight_format.logical_shape(self.qweight),
                dtype=torch.bfloat16, device=self.qweight.device,
            ).normal_(0.0, std, generator=generator)
            self._store_weight([tmp])
        else:
            self.weight.normal_(0.0, std, generator=generator)

    def _linear(
        self, x: torch.Tensor, bias: Optional[torch.Tensor] = None,
        rows: Optional[slice] = None,
    ):
        """x @ W^T (+ bias), or x @ W[rows]^T; codes and their scales are
        sliced together."""
        pick = (lambda t: t) if rows is None else (lambda t: t[rows])
        fmt = self.weight_format
        if fmt is not None:
            return getattr(ops, fmt.linear)(
                x, pick(self.qweight), pick(self.weight_scale), bias
            )
        return ops.linear(x, pick(self.weight), bias)


class ColumnParallelLinear(_QuantLinearBase):
    """Y_shard = X @ W_shard^T; output features sharded across TP ranks."""

    def __init__(
        self,
        in_features: int,
        out_features: int,
        bias: bool = False,
        dtype: torch.dtype = torch.bfloat16,
        gather_output: bool = False,
        quantization: Optional[str] = None,
    ):
        super().__init__()
        st = comm.get_state()
        self.tp_size = st.tp_size
        self.in_features = in_features
        self.out_features = out_features
        self.out_per_rank = _divide(out_features, self.tp_size)
        self.gather_output = gather_output
        self._alloc_weight(self.out_per_rank, in_features, dtype, quantization)
        self.bias = (
            nn.Parameter(
                torch.empty(self.out_per_rank, dtype=dtype), requires_grad=False
            )
            if bias
            else None
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self._linear(x, self.bias)
        if self.gather_output and self.tp_size > 1:
            y = comm.tp_all_gather(y, dim=-1)
        return y

    def load_shard(
        self,
        full_weight: torch.Tensor,
        full_bias: Optional[torch.Tensor] = None,
        weight_scale: Optional[torch.Tensor] = None,
    ):
        """Slice the full tensor for this rank (rows = output features).
        ``weight_scale``: per-channel f32 scale of a pre-quantized (fp8)
        ``full_weight``."""
        r = comm.get_state().tp_rank
        lo, hi = r * self.out_per_rank, (r + 1) * self.out_per_rank
        self._store_weight(
            [full_weight[lo:hi]],
            [None if weight_scale is None else weight_scale[lo:hi]],
        )
        if self.bias is not None and full_bias is not None:
            self.bias.data.copy_(full_bias[lo:hi].to(self.bias.dtype))


class QKVParallelLinear(_QuantLinearBase):
    """Fused QKV projection, head-sharded. Output layout per rank:
    [q_heads_local*D | kv_heads_local*D | kv_heads_local*D]."""

    def __init__(
        self,
        hidden_size: int,
        head_dim: int,
        num_heads: int,
        num_kv_heads: int,
        bias: bool = False,
        dtype: torch.dtype = torch.bfloat16,
        quantization: Optional[str] = None,
    ):
        super().__init__()
        st = comm.get_state()
        self.tp_size = st.tp_size
        self.head_dim = head_dim
        self.num_heads = num_heads
        self.num_kv_heads = num_kv_heads
        self.heads_local = _divide(num_heads, self.tp_size)
        # kv heads replicate when tp_size > num_kv_heads
        if num_kv_heads >= self.tp_size:
            self.kv_heads_local = _divide(num_kv_heads, self.tp_size)
            self.kv_replication = 1
        else:
            self.kv_heads_local = 1
            self.kv_replication = _divide(self.tp_size, num_kv_heads)
        out_local = (self.heads_local + 2 * self.kv_heads_local) * head_dim
        self.q_size = self.heads_local * head_dim
        self.kv_size = self.kv_heads_local * head_dim
        self._alloc_weight(out_local, hidden_size, dtype, quantization)
        self.bias = (
            nn.Parameter(torch.empty(out_local, dtype=dtype), requires_grad=False)
            if bias
            else None
        )

    def forward(self, x: torch.Tensor):
        qkv = self._linear(x, self.bias)
        return qkv.split([self.q_size, self.kv_size, self.kv_size], dim=-1)

    def load_shards(
        self,
        q_weight: torch.Tensor,
        k_weight: torch.Tensor,
        v_weight: torch.Tensor,
        q_bias: Optional[torch.Tensor] = None,
        k_bias: Optional[torch.Tensor] = None,
        v_bias: Optional[torch.Tensor] = None,
        q_scale: Optional[torch.Tensor] = None,
        k_scale: Optional[torch.Tensor] = None,
        v_scale: Optional[torch.Tensor] = None,
    ):
        """``*_scale``: per-channel f32 scales of pre-quantized (fp8)
        projections; the fused layer concatenates the sliced vectors."""
        r = comm.get_state().tp_rank
        D = self.head_dim
        q_lo = r * self.heads_local * D
        q_hi = q_lo + self.heads_local * D
        kv_rank = r // self.kv_replication
        kv_lo = kv_rank * self.kv_heads_local * D
        kv_hi = kv_lo + self.kv_heads_local * D
        self._store_weight(
            [q_weight[q_lo:q_hi], k_weight[kv_lo:kv_hi], v_weight[kv_lo:kv_hi]],
            [
                None if q_scale is None else q_scale[q_lo:q_hi],
                None if k_scale is None else k_scale[kv_lo:kv_hi],
                None if v_scale is None else v_scale[kv_lo:kv_hi],
            ],
        )
        if self.bias is not None and q_bias is not None:
            b = torch.cat(
                [q_bias[q_lo:q_hi], k_bias[kv_lo:kv_hi], v_bias[kv_lo:kv_hi]], dim=0
            )
            self.bias.data.copy_(b.to(self.bias.dtype))


class RowParallelLinear(_QuantLinearBase):
    """Y = sum_ranks(X_shard @ W_shard^T); input features sharded; output
    all-reduced (the per-layer RCCL call over xGMI).

    Comm/compute overlap (north star): with ``overlap_chunks`` > 1 the GEMM
    is split along output features and each chunk's all-reduce launches
    async as soon as its GEMM is queued — the next chunk's GEMM overlaps
    the previous chunk's xGMI time (per-link-bound ring). All handles are
    waited before the concatenated result is returned, so numerics are
    identical to the synchronous path.
    """

    # overlap engages above this many output elements (small decode
    # batches are latency-bound on the collective's launch, not its bytes)
    OVERLAP_MIN_NUMEL = 1 << 20

    def __init__(
        self,
        in_features: int,
        out_features: int,
        bias: bool = False,
        dtype: torch.dtype = torch.bfloat16,
        reduce_output: bool = True,
        overlap_chunks: int = 2,
        quantization: Optional[str] = None,
    ):
        super().__init__()
        st = comm.get_state()
        self.tp_size = st.tp_size
        self.in_per_rank = _divide(in_features, self.tp_size)
        self.out_features = out_features
        self.reduce_output = reduce_output
        self._alloc_weight(out_features, self.in_per_rank, dtype, quantization)
        # bias added once (rank 0 semantics handled by adding after reduce)
        self.bias = (
            nn.Parameter(torch.empty(out_features, dtype=dtype), requires_grad=False)
            if bias
            else None
        )
        self.overlap_chunks = max(1, overlap_chunks)

    def forward(
        self, x: torch.Tensor, delta: Optional[torch.Tensor] = None
    ) -> torch.Tensor:
        use_overlap = (
            self.reduce_output
            and self.tp_size > 1
            and delta is None
            and self.overlap_chunks > 1
            and x.shape[0] * self.out_features >= self.OVERLAP_MIN_NUMEL
        )
        if use_overlap:
            n = self.overlap_chunks
            step = -(-self.out_features // n)
            parts = []
            works = []
            for c in range(n):
                rows = slice(c * step, (c + 1) * step)
                if c * step >= self.out_features:
                    break
                yc = self._linear(x, rows=rows)
                works.append(comm.tp_all_reduce_async(yc))
                parts.append(yc)
            for w in works:
                if w is not None:
                    w.wait()
            y = torch.cat(parts, dim=-1)
            if self.bias is not None:
                y = y + self.bias
            return y
        y = self._linear(x)
        if delta is not None:
            # per-rank partial (e.g. LoRA with A column-sharded): must be
            # summed by the same all-reduce as the main GEMM
            y = y + delta
        if self.reduce_output:
            y = comm.tp_all_reduce(y)
        if self.bias is not None:
            y = y + self.bias
        return y

    def load_shard(
        self,
        full_weight: torch.Tensor,
        full_bias: Optional[torch.Tensor] = None,
        weight_scale: Optional[torch.Tensor] = None,
    ):
        """Slice this rank's input features, then quantize: every rank gets
        its own per-channel scales, so its partial is correctly scaled
        before the all-reduce. A pre-quantized checkpoint's per-channel
        scale applies to every column slice unchanged. A pre-quantized
        MXFP4 weight is sliced as bytes (two features each) with the
        matching scale columns (32 features each)."""
        r = comm.get_state().tp_rank
        lo, hi = r * self.in_per_rank, (r + 1) * self.in_per_rank
        if full_weight.dtype == torch.uint8:
            if self.in_per_rank % quant.MXFP4_BLOCK != 0:
                raise ValueError(
                    f"mxfp4 row-parallel shard: per-rank in_features "
                    f"({self.in_per_rank}) must be a multiple of "
                    f"{quant.MXFP4_BLOCK} so that no scale block is split"
                )
            if weight_scale is None:
                raise ValueError("mxfp4 checkpoint weight without weight_scale")
            weight_scale = quant.check_mxfp4_scale(
                weight_scale, full_weight.shape[0], full_weight.shape[1] * 2
            )
            b = quant.MXFP4_BLOCK
            self._store_weight(
                [full_weight[:, lo // 2:hi // 2]],
                [weight_scale[:, lo // b:hi // b]],
            )
        else:
            self._store_weight([full_weight[:, lo:hi]], [weight_scale])
        if self.bias is not None and full_bias is not None:
            self.bias.data.copy_(full_bias.to(self.bias.dtype))


class MergedColumnParallelLinear(_QuantLinearBase):
    """Fused gate+up projection (SwiGLU MLP), each half column-sharded.

    Per-rank output layout: [gate_local | up_local] so silu_and_mul can
    split it locally."""

    def __init__(
        self,
        in_features: int,
        out_features_each: int,
        bias: bool = False,
        dtype: torch.dtype = torch.bfloat16,
        quantization: Optional[str] = None,
    ):
        super().__init__()
        st = comm.get_state()
        self.tp_size = st.tp_size
        self.each_per_rank = _divide(out_features_each, self.tp_size)
        self._alloc_weight(
            2 * self.each_per_rank, in_features, dtype, quantization
        )
        self.bias = (
            nn.Parameter(
                torch.empty(2 * self.each_per_rank, dtype=dtype), requires_grad=False
            )
            if bias
            else None
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._linear(x, self.bias)

    def load_shards(
        self,
        gate_weight: torch.Tensor,
        up_weight: torch.Tensor,
        gate_scale: Optional[torch.Tensor] = None,
        up_scale: Optional[torch.Tensor] = None,
    ):
        r = comm.get_state().tp_rank
        lo, hi = r * self.each_per_rank, (r + 1) * self.each_per_rank
        self._store_weight(
            [gate_weight[lo:hi], up_weight[lo:hi]],
            [
                None if gate_scale is None else gate_scale[lo:hi],
                None if up_scale is None else up_scale[lo:hi],
            ],
        )


class VocabParallelEmbedding(nn.Module):
    """Embedding table sharded over vocab; out-of-shard rows contribute 0 and
    the result is all-reduced."""

    def __init__(
        self, vocab_size: int, hidden_size: int, dtype: torch.dtype = torch.bfloat16
    ):
        super().__init__()
        st = comm.get_state()
        self.tp_size = st.tp_size
        self.vocab_per_rank = _divide(vocab_size, self.tp_size)
        self.vocab_start = st.tp_rank * self.vocab_per_rank
        self.weight = nn.Parameter(
            torch.empty(self.vocab_per_rank, hidden_size, dtype=dtype),
            requires_grad=False,
        )

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        if self.tp_size == 1:
            return F.embedding(ids, self.weight)
        local = ids - self.vocab_start
        mask = (local < 0) | (local >= self.vocab_per_rank)
        local = local.clamp(0, self.vocab_per_rank - 1)
        out = F.embedding(local, self.weight)
        out[mask] = 0
        return comm.tp_all_reduce(out)

    def load_shard(self, full_weight: torch.Tensor):
        lo = self.vocab_start
        hi = lo + self.vocab_per_rank
        self.weight.data.copy_(full_weight[lo:hi].to(self.weight.dtype))
