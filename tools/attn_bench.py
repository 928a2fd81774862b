#!/usr/bin/env python3
"""Decode-attention kernel microbench: achieved KV-read TB/s vs the ~6.3 TB/s
HBM ceiling, across bench-relevant shapes. Run on GPU.

    python tools/attn_bench.py [--bf16-only]

A shape's context is one length for every sequence, or ``(lo, hi)`` for
lengths drawn uniformly from lo..hi with a fixed seed (the benchmark's batch
is not uniform). Bytes are the K+V of the tokens actually in context."""

import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kserve_amd import ops

assert torch.cuda.is_available()
dev = "cuda:0"
torch.manual_seed(0)

SHAPES = [
    # (S, H, Hkv, ctx)
    (256, 32, 8, 576),   # bench batch 256
    (512, 32, 8, 576),
    (1536, 32, 8, 576),  # headline batch of bench.py
    (1536, 32, 8, (512, 704)),  # headline batch, mixed lengths
    (64, 32, 8, 576),
    (8, 32, 8, 576),     # latency mode (split-context)
    (256, 32, 8, 2048),  # long context
    (64, 64, 8, 576),    # 70b-ish TP=1 heads
]
FP8_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[6]]

D, bs = 128, 16


def context_lens(S, ctx):
    if isinstance(ctx, tuple):
        g = torch.Generator().manual_seed(1234)
        return torch.randint(ctx[0], ctx[1] + 1, (S,), generator=g,
                             dtype=torch.int32)
    return torch.full((S,), ctx, dtype=torch.int32)


def run_shape(S, H, Hkv, ctx, fp8):
    lens = context_lens(S, ctx)
    nb = (int(lens.max()) + bs - 1) // bs
    B = S * nb + 1
    kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
    vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
    if fp8:
        kc = kc.to(torch.float8_e4m3fn)
        vc = vc.to(torch.float8_e4m3fn)
    bt = torch.arange(1, S * nb + 1, dtype=torch.int32, device=dev).reshape(S, nb)
    ctx_t = lens.to(dev)
    q = torch.randn(S, H, D, dtype=torch.bfloat16, device=dev)
    scale = 1.0 / math.sqrt(D)
    out = torch.empty_like(q)
    for _ in range(5):
        ops.paged_attention_decode(q, kc, vc, bt, ctx_t, scale, out=out)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    iters = 30
    for _ in range(iters):
        ops.paged_attention_decode(q, kc, vc, bt, ctx_t, scale, out=out)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / iters * 1000
    # K+V read once per kv-head group; fp8: 1 byte per element
    kv_bytes = int(lens.sum()) * Hkv * D * 2 * (1 if fp8 else 2)
    tbs = kv_bytes / (us * 1e-6) / 1e12
    label = f"{ctx[0]}-{ctx[1]}" if isinstance(ctx, tuple) else str(ctx)
    print(f"{S:4d} {H:3d} {Hkv:3d} {label:>7} {us:8.1f} {tbs:6.2f}", flush=True)


print(f"{'S':>4} {'H':>3} {'Hkv':>3} {'ctx':>7} {'us':>8} {'TB/s':>6}")
for S, H, Hkv, ctx in SHAPES:
    run_shape(S, H, Hkv, ctx, fp8=False)

if "--bf16-only" not in sys.argv[1:]:
    # fp8 KV cache variant (half the bytes; tok/s-equivalent speedup at large
    # batch where decode attention dominates)
    print("\nfp8 E4M3 KV cache:")
    print(f"{'S':>4} {'H':>3} {'Hkv':>3} {'ctx':>7} {'us':>8} {'TB/s':>6}")
    for S, H, Hkv, ctx in FP8_SHAPES:
        run_shape(S, H, Hkv, ctx, fp8=True)
