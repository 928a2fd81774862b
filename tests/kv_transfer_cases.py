"""Cases for the KV export/import ops (ops.kv_gather_pages /
ops.kv_scatter_pages). Helper module: imported by test_kv_transfer.py (CPU)
and test_gpu_kv_transfer.py; not collected.

Everything is compared bit for bit, so there is no tolerance. The pools are
filled with random finite bit patterns in which EVERY byte is non-zero
(low seven bits in 1..126, random top bit: finite and non-zero as bf16 and as
fp8 E4M3). A wrong page, a K/V swap, a layer swap or a missed zeroing of the
tail therefore always changes bytes, and a zeroed slot can never be mistaken
for copied data. Destination pools get a different such pattern.

``expected_gather`` / ``expected_scatter`` are written as plain loops over
(layer, K/V, page), independent of the vectorised torch_ref twins they check.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Tuple

import torch

POOL_PAGES = 12
BIG_POOL_PAGES = 640
BIG_N = 600


@dataclass(frozen=True)
class Geometry:
    L: int
    Hkv: int
    bs: int
    D: int
    dtype: torch.dtype

    @property
    def tag(self) -> str:
        d = "fp8" if self.dtype == torch.float8_e4m3fn else "bf16"
        return f"L{self.L}h{self.Hkv}d{self.D}{d}"


GEOMETRIES = (
    Geometry(2, 2, 16, 128, torch.bfloat16),
    Geometry(2, 1, 16, 64, torch.bfloat16),
    # 1 KB pages: fewer 16-byte vectors than one workgroup has lanes
    Geometry(3, 1, 16, 64, torch.float8_e4m3fn),
    Geometry(2, 2, 16, 128, torch.float8_e4m3fn),
)

# (source ids, destination ids): non-monotonic, not starting at 0
ID_LISTS = (
    ([7], [4]),
    ([7, 2, 9], [10, 1, 5]),
    ([11, 3, 8, 1, 6], [2, 9, 4, 11, 7]),
)


@dataclass(frozen=True)
class Case:
    name: str
    geo: Geometry
    pool_pages: int
    block_ids: Tuple[int, ...]
    dst_ids: Tuple[int, ...]
    num_tokens: int


def _token_counts(n: int, bs: int) -> List[int]:
    counts = {n * bs, n * bs - 1, (n - 1) * bs + 1}
    if n == 1:
        counts.add(1)
    return sorted(counts)


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    out = []
    for geo in GEOMETRIES:
        for ids, dst in ID_LISTS:
            for nt in _token_counts(len(ids), geo.bs):
                out.append(
                    Case(
                        f"{geo.tag}-n{len(ids)}-t{nt}", geo, POOL_PAGES,
                        tuple(ids), tuple(dst), nt,
                    )
                )
    # more 256-lane workgroups of 16-byte vectors (4 * 600 pages * 512 =
    # 1.2M vectors = 4800) than the kernels' grid cap of 2048: the stride
    # loop runs more than once. ~20 MB per pool.
    geo = GEOMETRIES[0]
    g = torch.Generator().manual_seed(77)
    perm = torch.randperm(BIG_POOL_PAGES - 1, generator=g) + 1
    ids = tuple(int(b) for b in perm[:BIG_N])
    dst = tuple(int(b) for b in perm.flip(0)[:BIG_N])
    out.append(
        Case(f"{geo.tag}-gridcap-n{BIG_N}", geo, BIG_POOL_PAGES, ids, dst,
             BIG_N * geo.bs - 5)
    )
    return tuple(out)


def small_cases() -> Tuple[Case, ...]:
    return tuple(c for c in cases() if c.pool_pages == POOL_PAGES)


def random_pool(geo: Geometry, pages: int, seed: int, device="cpu"):
    """[(K, V)] * L of finite patterns with every byte non-zero."""
    g = torch.Generator().manual_seed(seed)
    shape = (pages, geo.Hkv, geo.bs, geo.D * geo.dtype.itemsize)
    pool = []
    for _ in range(geo.L):
        pair = []
        for _ in range(2):
            low = torch.randint(1, 127, shape, generator=g, dtype=torch.uint8)
            top = torch.randint(0, 2, shape, generator=g, dtype=torch.uint8)
            pair.append((low | (top << 7)).view(geo.dtype).to(device))
        pool.append(tuple(pair))
    return pool


def build(case: Case, device="cpu"):
    """(source pool, destination pool) of a case."""
    return (
        random_pool(case.geo, case.pool_pages, 1, device),
        random_pool(case.geo, case.pool_pages, 2, device),
    )


def clone_pool(pool):
    return [(k.clone(), v.clone()) for k, v in pool]


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8).cpu()


def pools_equal(a, b) -> bool:
    return all(
        torch.equal(as_bytes(x), as_bytes(y))
        for pa, pb in zip(a, b)
        for x, y in zip(pa, pb)
    )


def expected_gather(case: Case, src) -> torch.Tensor:
    """uint8 [L, 2, n, Hkv, bs, D*itemsize], by plain loops."""
    geo = case.geo
    n = len(case.block_ids)
    out = torch.zeros(
        geo.L, 2, n, geo.Hkv, geo.bs, geo.D * geo.dtype.itemsize,
        dtype=torch.uint8,
    )
    for layer in range(geo.L):
        for kv in range(2):
            pages = as_bytes(src[layer][kv])
            for j, b in enumerate(case.block_ids):
                valid = min(max(case.num_tokens - j * geo.bs, 0), geo.bs)
                out[layer, kv, j, :, :valid] = pages[b, :, :valid]
    return out


def expected_scatter(case: Case, dst, buf: torch.Tensor):
    """Destination pool (as uint8 tensors) after scattering ``buf`` (the
    uint8 layout of expected_gather) into ``case.dst_ids``."""
    out = []
    for layer in range(case.geo.L):
        pair = []
        for kv in range(2):
            pages = as_bytes(dst[layer][kv]).clone()
            for j, b in enumerate(case.dst_ids):
                pages[b] = buf[layer, kv, j]
            pair.append(pages)
        out.append(tuple(pair))
    return out
