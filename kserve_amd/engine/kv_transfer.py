"""KV hand-off between engines (prefill/decode disaggregation).

A prefill engine exports a request after its first sampled token: the
request's KV pages of every layer are gathered into one contiguous buffer
(``ops.kv_gather_pages``) and travel, with what the decode engine needs to
continue the request, as a ``KVPayload``. The decode engine scatters the
pages into its own pool (``ops.kv_scatter_pages``) and decodes on.

Wire format (``to_bytes`` / ``from_bytes``), no pickle:

    MAGIC (8 bytes) | header length (uint32, little endian) | JSON header |
    page bytes

The page bytes are the [L, 2, n, Hkv, block_size, D] buffer of the gather,
``n = ceil(num_tokens / block_size)`` pages per tensor, slots at or past
``num_tokens`` zero.
"""

from __future__ import annotations

import json
import struct
from dataclasses import dataclass
from typing import List, Optional

import torch

MAGIC = b"KSKVPAY\x00"
FORMAT_VERSION = 1
# largest header from_bytes will parse (a prompt's token ids dominate it)
_MAX_HEADER_BYTES = 64 << 20

_DTYPE_NAMES = {
    torch.bfloat16: "bfloat16",
    torch.float16: "float16",
    torch.float32: "float32",
    torch.float8_e4m3fn: "fp8_e4m3",
}
_DTYPES = {v: k for k, v in _DTYPE_NAMES.items()}


def dtype_name(dtype: torch.dtype) -> str:
    try:
        return _DTYPE_NAMES[dtype]
    except KeyError:
        raise ValueError(f"KV dtype {dtype} cannot travel") from None


def torch_dtype(name: str) -> torch.dtype:
    try:
        return _DTYPES[name]
    except KeyError:
        raise ValueError(f"unknown KV payload dtype {name!r}") from None


@dataclass
class KVPayload:
    num_layers: int
    num_kv_heads: int
    head_dim: int
    block_size: int
    dtype: str  # payload dtype name (see _DTYPE_NAMES)
    model_name: str
    quantization: Optional[str]
    prompt_token_ids: List[int]
    # tokens sampled so far: the first token
    output_token_ids: List[int]
    # positions whose KV is in the payload == prompt length
    num_tokens: int
    # page data, one uint8 tensor (pinned on GPU engines)
    data: torch.Tensor
    # the first token's {token_id: logprob} entry when it was requested
    first_logprobs: Optional[dict] = None
    version: int = FORMAT_VERSION

    # -- geometry ----------------------------------------------------------
    @property
    def num_pages(self) -> int:
        return -(-self.num_tokens // self.block_size)

    @property
    def torch_dtype(self) -> torch.dtype:
        return torch_dtype(self.dtype)

    @property
    def expected_data_bytes(self) -> int:
        return (
            self.num_layers * 2 * self.num_pages * self.num_kv_heads
            * self.block_size * self.head_dim * self.torch_dtype.itemsize
        )

    def validate(self) -> None:
        """Internal consistency; raises ValueError."""
        if self.version != FORMAT_VERSION:
            raise ValueError(
                f"unknown KV payload version {self.version} "
                f"(this build reads {FORMAT_VERSION})"
            )
        for name in ("num_layers", "num_kv_heads", "head_dim", "block_size"):
            v = getattr(self, name)
            if not isinstance(v, int) or v <= 0:
                raise ValueError(f"KV payload {name} must be positive, got {v!r}")
        torch_dtype(self.dtype)
        if self.num_tokens != len(self.prompt_token_ids) or self.num_tokens < 1:
            raise ValueError(
                f"KV payload num_tokens {self.num_tokens} does not equal the "
                f"prompt length {len(self.prompt_token_ids)}"
            )
        if not self.output_token_ids:
            raise ValueError("KV payload carries no sampled token")
        if self.data.dtype != torch.uint8 or self.data.dim() != 1:
            raise ValueError("KV payload data must be a flat uint8 tensor")
        if self.data.numel() != self.expected_data_bytes:
            raise ValueError(
                f"KV payload data is {self.data.numel()} bytes, geometry and "
                f"num_tokens {self.num_tokens} ({self.num_pages} pages) "
                f"imply {self.expected_data_bytes}"
            )

    # -- wire format -------------------------------------------------------
    def _header(self) -> dict:
        return {
            "version": self.version,
            "num_layers": self.num_layers,
            "num_kv_heads": self.num_kv_heads,
            "head_dim": self.head_dim,
            "block_size": self.block_size,
            "dtype": self.dtype,
            "model_name": self.model_name,
            "quantization": self.quantization,
            "prompt_token_ids": list(self.prompt_token_ids),
            "output_token_ids": list(self.output_token_ids),
            "num_tokens": self.num_tokens,
            "num_pages": self.num_pages,
            "data_bytes": int(self.data.numel()),
            "first_logprobs": (
                None
                if self.first_logprobs is None
                else {str(k): float(v) for k, v in self.first_logprobs.items()}
            ),
        }

    def to_bytes(self) -> bytes:
        header = json.dumps(self._header(), separators=(",", ":")).encode()
        # one copy of the pages: join reads the tensor's memory in place
        body = memoryview(self.data.cpu().contiguous().numpy())
        return b"".join((MAGIC, struct.pack("<I", len(header)), header, body))

    @classmethod
    def from_bytes(cls, blob, pin_memory: Optional[bool] = None) -> "KVPayload":
        """Parse and validate any bytes-like object. Refuses (ValueError) a
        wrong magic, an unknown version, a truncated or over-long body, a
        data length other than the geometry implies, and num_tokens
        inconsistent with the page count. The pages are copied once, from
        ``blob`` into the (pinned) tensor of the payload."""
        blob = memoryview(blob).cast("B")
        fixed = len(MAGIC) + 4
        if len(blob) < fixed or bytes(blob[: len(MAGIC)]) != MAGIC:
            raise ValueError("not a KV payload (bad magic)")
        (hlen,) = struct.unpack("<I", blob[len(MAGIC) : fixed])
        if hlen > _MAX_HEADER_BYTES or fixed + hlen > len(blob):
            raise ValueError("KV payload truncated inside its header")
        try:
            h = json.loads(bytes(blob[fixed : fixed + hlen]).decode())
        except (UnicodeDecodeError, json.JSONDecodeError) as e:
            raise ValueError(f"KV payload header is not JSON: {e}") from None
        if not isinstance(h, dict):
            raise ValueError("KV payload header is not an object")
        if h.get("version") != FORMAT_VERSION:
            raise ValueError(
                f"unknown KV payload version {h.get('version')!r} "
                f"(this build reads {FORMAT_VERSION})"
            )
        try:
            body_len = int(h["data_bytes"])
            num_pages = int(h["num_pages"])
            lp = h.get("first_logprobs")
            payload = cls(
                num_layers=h["num_layers"],
                num_kv_heads=h["num_kv_heads"],
                head_dim=h["head_dim"],
                block_size=h["block_size"],
                dtype=h["dtype"],
                model_name=h["model_name"],
                quantization=h["quantization"],
                prompt_token_ids=[int(t) for t in h["prompt_token_ids"]],
                output_token_ids=[int(t) for t in h["output_token_ids"]],
                num_tokens=h["num_tokens"],
                data=torch.empty(0, dtype=torch.uint8),
                first_logprobs=(
                    None if lp is None
                    else {int(k): float(v) for k, v in lp.items()}
                ),
                version=h["version"],
            )
        except (KeyError, TypeError, ValueError, AttributeError) as e:
            raise ValueError(f"KV payload header is malformed: {e!r}") from None
        body = len(blob) - fixed - hlen
        if body < body_len:
            raise ValueError(
                f"KV payload truncated: {body} of {body_len} data bytes"
            )
        if body > body_len:
            raise ValueError(
                f"KV payload over-long: {body - body_len} bytes past its data"
            )
        if not isinstance(payload.num_tokens, int) or not isinstance(
            payload.block_size, int
        ) or payload.block_size <= 0:
            raise ValueError("KV payload header is malformed: geometry")
        if num_pages != payload.num_pages:
            raise ValueError(
                f"KV payload num_tokens {payload.num_tokens} needs "
                f"{payload.num_pages} pages of {payload.block_size}, header "
                f"says {num_pages}"
            )
        if pin_memory is None:
            pin_memory = torch.cuda.is_available()
        data = torch.empty(body_len, dtype=torch.uint8, pin_memory=pin_memory)
        if body_len:
            import numpy as np

            # a view of the caller's buffer, read once by the copy
            data.numpy()[:] = np.frombuffer(
                blob, dtype=np.uint8, count=body_len, offset=fixed + hlen
            )
        payload.data = data
        payload.validate()
        return payload

    # -- compatibility -----------------------------------------------------
    def check_compatible(self, engine_config, pool_dtype=None) -> None:
        """Raise ValueError naming the first field in which this payload
        and an engine of ``engine_config`` disagree. ``pool_dtype`` is the
        engine's actual KV pool dtype; by default it follows from the
        config the way the engine derives it."""
        m = engine_config.model
        if pool_dtype is None:
            pool_dtype = engine_config.cache.cache_torch_dtype(
                torch.bfloat16 if m.dtype == "bfloat16" else torch.float32
            )
        pairs = (
            ("num_layers", self.num_layers, m.num_layers),
            ("num_kv_heads", self.num_kv_heads, m.num_kv_heads),
            ("head_dim", self.head_dim, m.head_dim),
            ("block_size", self.block_size, engine_config.cache.block_size),
            ("dtype", self.dtype, dtype_name(pool_dtype)),
            ("model_name", self.model_name, m.model_name),
            ("quantization", self.quantization, m.quantization),
        )
        for name, mine, theirs in pairs:
            if mine != theirs:
                raise ValueError(
                    f"KV payload incompatible with this engine: {name} is "
                    f"{mine!r} in the payload, {theirs!r} here"
                )
