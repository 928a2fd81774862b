"""Multi-LoRA adapter serving for the native engine.

Reference parity: huggingfaceserver __main__.py:334-337 (--enable-lora /
--lora-modules name=path register adapter names with the model server; the
vLLM backend applies adapters per request). MI355X-native design: adapters
stay unmerged; per batch the runner records contiguous row segments per
adapter and each parallel layer adds ``(x @ A^T) @ B^T * scale`` for its
segment — two skinny hipBLASLt GEMMs per adapter per module, no sort/gather
kernels, exact under tensor parallelism (column-parallel modules shard B
rows; row-parallel modules shard A columns and add the partial delta before
the xGMI all-reduce).

Decode on the GPU does not loop over segments. The manager also keeps every
adapter in zero-filled stacks, ``a_stack[max_loras, R, in]`` and
``b_stack[max_loras, out, R]`` per (layer, module) plus one ``scale`` and one
``ranks`` vector, adapter ``id`` in slot ``id - 1``. Each token row carries a
device-side slot index (-1 = base model) and two HIP kernels per module
(``ops.lora_shrink`` / ``ops.lora_expand_add``) serve any adapter mix, with
nothing about the mix on the host, so the step is captured in a hipGraph like
the base step. The stacks are allocated once and only ever written in place:
a later registration reaches graphs captured before it. ``KS_LORA_SEGMENTS=1``
keeps decode on the segment loop (ablation). Prefill and CPU always use it.
"""

from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

# module keys the llama forward asks for
COLUMN_MODULES = ("q_proj", "k_proj", "v_proj", "gate_proj", "up_proj")
ROW_MODULES = ("o_proj", "down_proj")
ALL_MODULES = COLUMN_MODULES + ROW_MODULES


@dataclass
class LoRALayerWeights:
    a: torch.Tensor  # [r, in_local]
    b: torch.Tensor  # [out_local, r]
    scale: float

    def delta(self, x: torch.Tensor) -> torch.Tensor:
        return ((x @ self.a.t()) @ self.b.t()) * self.scale


@dataclass
class LoRAAdapter:
    adapter_id: int
    name: str
    rank: int
    # (layer_idx, module) -> weights
    weights: Dict[Tuple[int, str], LoRALayerWeights] = field(default_factory=dict)

    def get(self, layer_idx: int, module: str) -> Optional[LoRALayerWeights]:
        return self.weights.get((layer_idx, module))


def batched_decode_enabled() -> bool:
    """False under the ablation switch KS_LORA_SEGMENTS=1 (decode keeps the
    per-segment GEMM loop and, with it, the eager path)."""
    return os.environ.get("KS_LORA_SEGMENTS", "0") != "1"


@dataclass
class LoRABatchMeta:
    """Per-forward LoRA context: contiguous token-row segments per adapter,
    and for decode steps the per-row adapter slots the batched kernels read."""

    # (adapter_id, start_row, end_row) — rows with adapter_id 0 are skipped
    segments: List[Tuple[int, int, int]]
    manager: "LoRAManager"
    # [T] int32, adapter_id - 1 per row, -1 for base rows (on the forward's
    # device for decode steps)
    row_slots: Optional[torch.Tensor] = None
    decode: bool = False

    def _batched(self, x: torch.Tensor) -> bool:
        return (
            self.decode
            and x.is_cuda
            and self.row_slots is not None
            and self.manager.has_stacks
            and batched_decode_enabled()
        )

    def _apply_batched(self, layer_idx, module, x, y, out_offset) -> bool:
        """y[:, off:off+N] += delta for every row, two launches; False if no
        registered adapter targets this module."""
        from kserve_amd import ops

        st = self.manager.stacks(layer_idx, module)
        if st is None:
            return False
        a_stack, b_stack = st
        m = self.manager
        tmp = ops.lora_shrink(x, a_stack, m.ranks_stack, self.row_slots)
        ops.lora_expand_add(
            y, tmp, b_stack, m.scale_stack, m.ranks_stack, self.row_slots,
            out_offset,
        )
        return True

    def apply(
        self,
        layer_idx: int,
        module: str,
        x: torch.Tensor,   # [T, in_local] layer input
        y: torch.Tensor,   # [T, out] tensor to add the delta into (in place)
        out_offset: int = 0,
    ) -> None:
        if self._batched(x):
            self._apply_batched(layer_idx, module, x, y, out_offset)
            return
        for aid, s, e in self.segments:
            w = self.manager.layer_weights(aid, layer_idx, module)
            if w is None:
                continue
            d = w.delta(x[s:e])
            y[s:e, out_offset : out_offset + d.shape[1]] += d

    def delta_for(
        self, layer_idx: int, module: str, x: torch.Tensor
    ) -> Optional[torch.Tensor]:
        """Standalone delta tensor for row-parallel modules (added to the
        local partial before the all-reduce)."""
        if self._batched(x):
            st = self.manager.stacks(layer_idx, module)
            if st is None:
                return None
            out = torch.zeros(
                x.shape[0], st[1].shape[1], dtype=x.dtype, device=x.device
            )
            self._apply_batched(layer_idx, module, x, out, 0)
            return out
        out = None
        for aid, s, e in self.segments:
            w = self.manager.layer_weights(aid, layer_idx, module)
            if w is None:
                continue
            if out is None:
                out = torch.zeros(
                    x.shape[0], w.b.shape[0], dtype=x.dtype, device=x.device
                )
            out[s:e] = w.delta(x[s:e])
        return out


class LoRAManager:
    """Loads and holds adapters; resolves names to ids."""

    def __init__(self, device: str, dtype: torch.dtype, tp_rank: int = 0,
                 tp_size: int = 1, max_loras: int = 8,
                 max_lora_rank: int = 64):
        self.device = device
        self.dtype = dtype
        self.tp_rank = tp_rank
        self.tp_size = tp_size
        self.max_loras = max_loras
        self.max_lora_rank = max_lora_rank
        self._adapters: Dict[int, LoRAAdapter] = {}
        self._by_name: Dict[str, int] = {}
        self._next_id = 1
        # stacked storage for the batched decode kernels (CUDA devices only)
        self.stack_rank = (max_lora_rank + 7) // 8 * 8
        self._stacks: Dict[
            Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]
        ] = {}
        self.scale_stack: Optional[torch.Tensor] = None  # [max_loras] f32
        self.ranks_stack: Optional[torch.Tensor] = None  # [max_loras] int32
        self._stacks_off = False
        # bumped when a (layer, module) stack is added: decode graphs
        # captured before it hold no launches for that module
        self.stacks_version = 0

    # -- registration --------------------------------------------------------
    def register(self, name: str, path: str) -> int:
        if name in self._by_name:
            return self._by_name[name]
        if len(self._adapters) >= self.max_loras:
            raise ValueError(
                f"cannot register LoRA adapter {name!r}: all "
                f"{self.max_loras} adapter slots are in use; raise "
                "EngineConfig.lora.max_loras"
            )
        return self.install(self._load(name, path))

    def next_adapter_id(self) -> int:
        return self._next_id

    def install(self, adapter: LoRAAdapter) -> int:
        """Make a loaded adapter (weights already TP-sharded, on the device,
        id taken from ``next_adapter_id``) addressable; ``register`` ends
        here, synthetic adapters of benchmarks start here."""
        if adapter.name in self._by_name or adapter.adapter_id in self._adapters:
            raise ValueError(f"LoRA adapter {adapter.name!r} already installed")
        if len(self._adapters) >= self.max_loras:
            raise ValueError(
                f"cannot install LoRA adapter {adapter.name!r}: all "
                f"{self.max_loras} adapter slots are in use; raise "
                "EngineConfig.lora.max_loras"
            )
        if adapter.rank > self.max_lora_rank:
            raise ValueError(
                f"LoRA adapter {adapter.name!r} has rank {adapter.rank} > "
                f"max_lora_rank {self.max_lora_rank}; raise "
                "EngineConfig.lora.max_lora_rank"
            )
        self._next_id = max(self._next_id, adapter.adapter_id + 1)
        self._fill_stacks(adapter)
        self._adapters[adapter.adapter_id] = adapter
        self._by_name[adapter.name] = adapter.adapter_id
        return adapter.adapter_id

    # -- stacked storage -----------------------------------------------------
    @property
    def has_stacks(self) -> bool:
        return bool(self._stacks)

    def stacks(
        self, layer_idx: int, module: str
    ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(a_stack [S, R, in_local], b_stack [S, out_local, R]) or None if
        no registered adapter targets the module."""
        return self._stacks.get((layer_idx, module))

    def _stackable(self, adapter: LoRAAdapter) -> bool:
        """The kernels need bf16, in % 64 == 0 and out % 64 == 0."""
        return self.dtype == torch.bfloat16 and all(
            w.a.shape[1] % 64 == 0 and w.b.shape[0] % 64 == 0
            for w in adapter.weights.values()
        )

    def _fill_stacks(self, adapter: LoRAAdapter) -> None:
        """Copy the adapter's (already TP-sharded) matrices into slot
        ``adapter_id - 1``. The stacks are zero-filled, so rows [rank, R) of
        the slot's A and columns [rank, R) of its B stay zero, which is what
        lets the kernels round the rank up to a multiple of 8. Stacks are
        created the first time a (layer, module) is seen and never replaced:
        their pointers are baked into captured graphs."""
        if torch.device(self.device).type != "cuda" or self._stacks_off:
            return
        if not self._stackable(adapter):
            if self._stacks:
                raise ValueError(
                    f"LoRA adapter {adapter.name!r} has module shapes the "
                    "batched decode kernels do not take (in/out features "
                    "must be multiples of 64)"
                )
            self._stacks_off = True  # decode stays on the segment loop
            return
        S, R = self.max_loras, self.stack_rank
        slot = adapter.adapter_id - 1
        if self.scale_stack is None:
            self.scale_stack = torch.zeros(
                S, dtype=torch.float32, device=self.device
            )
            self.ranks_stack = torch.zeros(
                S, dtype=torch.int32, device=self.device
            )
        scale = 0.0
        for key, w in adapter.weights.items():
            st = self._stacks.get(key)
            if st is None:
                st = (
                    torch.zeros(S, R, w.a.shape[1], dtype=self.dtype,
                                device=self.device),
                    torch.zeros(S, w.b.shape[0], R, dtype=self.dtype,
                                device=self.device),
                )
                self._stacks[key] = st
                self.stacks_version += 1
            r = w.a.shape[0]
            st[0][slot, :r].copy_(w.a)
            st[1][slot, :, :r].copy_(w.b)
            scale = w.scale
        self.scale_stack[slot] = scale
        self.ranks_stack[slot] = adapter.rank

    def lookup(self, name: Optional[str]) -> int:
        if not name:
            return 0
        if name not in self._by_name:
            raise KeyError(f"unknown LoRA adapter: {name}")
        return self._by_name[name]

    def names(self) -> List[str]:
        return list(self._by_name)

    def layer_weights(
        self, adapter_id: int, layer_idx: int, module: str
    ) -> Optional[LoRALayerWeights]:
        a = self._adapters.get(adapter_id)
        return a.get(layer_idx, module) if a is not None else None

    # -- loading (HF PEFT format) -------------------------------------------
    def _load(self, name: str, path: str) -> LoRAAdapter:
        cfg_path = os.path.join(path, "adapter_config.json")
        with open(cfg_path) as f:
            cfg = json.load(f)
        r = int(cfg["r"])
        if r > self.max_lora_rank:
            raise ValueError(
                f"LoRA adapter {name!r} has rank {r} > max_lora_rank "
                f"{self.max_lora_rank}; raise EngineConfig.lora.max_lora_rank"
            )
        alpha = float(cfg.get("lora_alpha", r))
        scale = alpha / r
        if cfg.get("use_rslora"):
            scale = alpha / (r ** 0.5)
        tensors = self._read_tensors(path)
        adapter = LoRAAdapter(self._next_id, name, r)
        self._next_id += 1
        for key, t in tensors.items():
            parsed = self._parse_key(key)
            if parsed is None:
                continue
            layer_idx, module, which = parsed
            lw = adapter.weights.setdefault(
                (layer_idx, module), LoRALayerWeights(None, None, scale)
            )
            t = t.to(self.dtype)
            if which == "A":
                lw.a = self._shard_a(module, t)
            else:
                lw.b = self._shard_b(module, t)
        # drop incomplete pairs (e.g. modules outside the llama set)
        adapter.weights = {
            k: w
            for k, w in adapter.weights.items()
            if w.a is not None and w.b is not None
        }
        for w in adapter.weights.values():
            w.a = w.a.to(self.device).contiguous()
            w.b = w.b.to(self.device).contiguous()
        return adapter

    def _read_tensors(self, path: str) -> Dict[str, torch.Tensor]:
        st = os.path.join(path, "adapter_model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file

            return load_file(st)
        bin_path = os.path.join(path, "adapter_model.bin")
        if os.path.exists(bin_path):
            return torch.load(bin_path, map_location="cpu", weights_only=True)
        raise FileNotFoundError(f"no adapter weights under {path}")

    @staticmethod
    def _parse_key(key: str) -> Optional[Tuple[int, str, str]]:
        """'...model.layers.{i}.(self_attn|mlp).{mod}.lora_(A|B).weight'"""
        if "lora_A" in key:
            which = "A"
        elif "lora_B" in key:
            which = "B"
        else:
            return None
        parts = key.split(".")
        try:
            li = parts.index("layers")
            layer_idx = int(parts[li + 1])
        except (ValueError, IndexError):
            return None
        module = None
        for m in ALL_MODULES:
            if m in parts:
                module = m
                break
        if module is None:
            return None
        return layer_idx, module, which

    # -- TP sharding ---------------------------------------------------------
    def _shard_b(self, module: str, b: torch.Tensor) -> torch.Tensor:
        """Column-parallel modules shard the B rows (output dim)."""
        if self.tp_size == 1 or module in ROW_MODULES:
            return b
        out = b.shape[0]
        per = out // self.tp_size
        return b[self.tp_rank * per : (self.tp_rank + 1) * per]

    def _shard_a(self, module: str, a: torch.Tensor) -> torch.Tensor:
        """Row-parallel modules shard the A columns (input dim)."""
        if self.tp_size == 1 or module not in ROW_MODULES:
            return a
        inp = a.shape[1]
        per = inp // self.tp_size
        return a[:, self.tp_rank * per : (self.tp_rank + 1) * per]
