#!/usr/bin/env python3
"""Microbench the decode-path GEMM shapes: achieved TB/s (weight traffic) per
shape, to judge hipBLASLt (tuned/untuned) against the HBM roofline.

Run on GPU: python tools/gemm_bench.py [--tune]
            python tools/gemm_bench.py --w8 [--out FILE.md]
            python tools/gemm_bench.py --w4 [--out FILE.md]

--w8 is the A/B behind ops.W8_MAX_TOKENS (profiles/w8_gemm.md): per
Llama-3-8B projection shape and token batch it times, in one process and
interleaved, (a) ops.linear on bf16 weights, (b) the fp8-weight skinny GEMM
and (c) dequant + hipBLASLt, the path ops.linear_w8 takes above the
threshold.

--w4 is the same A/B behind ops.W4_MAX_TOKENS (profiles/w4_gemm.md), with
the columns (a) ops.linear on bf16 weights, (b) the fp8-weight skinny GEMM,
(c) the MXFP4-weight skinny GEMM and (d) MXFP4 dequant + hipBLASLt.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

parser = argparse.ArgumentParser()
parser.add_argument("--tune", action="store_true")
parser.add_argument("--iters", type=int, default=50)
parser.add_argument("--w8", action="store_true",
                    help="fp8-weight A/B table instead of the bf16 table")
parser.add_argument("--w4", action="store_true",
                    help="MXFP4-weight A/B table instead of the bf16 table")
parser.add_argument("--out", default=None,
                    help="--w8/--w4: also write the table as markdown here")
args = parser.parse_args()

if args.tune:
    os.environ["PYTORCH_TUNABLEOP_ENABLED"] = "1"
    os.environ["PYTORCH_TUNABLEOP_TUNING"] = "1"
    os.environ["PYTORCH_TUNABLEOP_MAX_TUNING_DURATION_MS"] = "200"
    os.environ["PYTORCH_TUNABLEOP_FILENAME"] = "gpurun_out/tunableop_decode.csv"
else:
    base = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "profiles", "tunableop_gfx950.csv")
    if os.path.exists(base.replace(".csv", "0.csv")):
        os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
        os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", base)

import torch
import torch.nn.functional as F

assert torch.cuda.is_available()
dev = "cuda:0"

# decode GEMMs for llama-3-8b at token batch N (plus prefill-ish 16384)
SHAPES = [
    # (name, N tokens, K in, M out)
    ("qkv", 256, 4096, 6144),
    ("o", 256, 4096, 4096),
    ("gate_up", 256, 4096, 28672),
    ("down", 256, 14336, 4096),
    ("lm_head", 256, 4096, 128256),
    ("qkv", 64, 4096, 6144),
    ("gate_up", 64, 4096, 28672),
    ("down", 64, 14336, 4096),
    ("lm_head", 64, 4096, 128256),
    ("qkv_prefill", 16384, 4096, 6144),
    ("gate_up_prefill", 16384, 4096, 28672),
]

import kserve_amd_C


def bench_w8():
    """One row per (shape, N): median-of-rounds us for the three variants,
    rounds interleaved so drift hits all three alike. Each call streams a
    different weight copy (the set is larger than the 256 MB Infinity
    Cache), as consecutive layers do in a model; TB/s is weight bytes of
    the variant's own format over its time."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.ops.quant import quantize_fp8_per_channel

    shapes = [  # (name, K in, M out): Llama-3-8B projections
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
    ]
    batches = [1, 16, 64, 128, 256]
    rounds = 5
    for _, K, M in shapes:
        ops.reserve_w8_scratch(dev, M, K)

    def timed(fn, copies, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(iters):
            fn(i % copies)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1000

    lines = [
        "| shape | K | M | N | (a) bf16 us | (a) TB/s | (b) w8 us | (b) TB/s "
        "| (c) dequant+GEMM us | (b)/(a) | (b)<=(c) |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    print(lines[0]); print(lines[1])
    worst = {n: True for n in batches}
    for name, K, M in shapes:
        copies = max(2, -(-(768 << 20) // (M * K)))
        gen = torch.Generator(device=dev).manual_seed(0)
        ws, qs, ss = [], [], []
        for _ in range(copies):
            w = torch.randn(M, K, dtype=torch.bfloat16, device=dev,
                            generator=gen) * 0.02
            q, s = quantize_fp8_per_channel(w)
            ws.append(w); qs.append(q); ss.append(s)
        for N in batches:
            x = torch.randn(N, K, dtype=torch.bfloat16, device=dev,
                            generator=gen) / 8
            out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)

            def fa(i):
                return ops.linear(x, ws[i])

            def fb(i):
                kserve_amd_C.skinny_gemm_w8(out, x, qs[i], ss[i])

            def fc(i):
                return ops.linear_w8(x, qs[i], ss[i])

            iters = max(args.iters, 2 * copies)
            res = {"a": [], "b": [], "c": []}
            keep = ops.W8_MAX_TOKENS
            try:
                for r in range(rounds + 1):  # round 0 is warm-up
                    for key, fn in (("a", fa), ("b", fb), ("c", fc)):
                        ops.W8_MAX_TOKENS = 0 if key == "c" else keep
                        t = timed(fn, copies, iters)
                        if r:
                            res[key].append(t)
            finally:
                ops.W8_MAX_TOKENS = keep
            a, b, c = (statistics.median(res[k]) for k in "abc")
            spread = max(
                (max(res[k]) - min(res[k])) / statistics.median(res[k])
                for k in "abc"
            )
            ok = b <= c
            worst[N] = worst[N] and ok
            line = (
                f"| {name} | {K} | {M} | {N} | {a:.1f} | "
                f"{M * K * 2 / a / 1e6:.2f} | {b:.1f} | {M * K / b / 1e6:.2f} "
                f"| {c:.1f} | {b / a:.2f} | {'yes' if ok else 'no'} |"
            )
            print(line + f"  spread {spread:.0%}", flush=True)
            lines.append(line)
        del ws, qs, ss
        torch.cuda.empty_cache()
    # largest N such that (b) <= (c) on all four shapes (0 if none)
    chosen = max([n for n in batches if worst[n]], default=0)
    tail = f"\nW8_MAX_TOKENS by this table: {chosen}"
    print(tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + tail + "\n")


def bench_w4():
    """bench_w8's method (interleaved rounds, a weight set larger than the
    256 MB Infinity Cache even at 4.25 bits per weight) with the MXFP4
    kernel and its dequant path beside the bf16 and fp8 kernels. TB/s is
    weight bytes of the variant's own format (scales included) over its
    time."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.ops.quant import quantize_fp8_per_channel, quantize_mxfp4

    shapes = [  # (name, K in, M out): Llama-3-8B projections
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
    ]
    batches = [1, 16, 64, 128]
    rounds = 5
    for _, K, M in shapes:
        ops.reserve_w8_scratch(dev, M, K)

    def timed(fn, copies, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(iters):
            fn(i % copies)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1000

    lines = [
        "| shape | K | M | N | (a) bf16 us | (a) TB/s | (b) w8 us | (b) TB/s "
        "| (c) w4 us | (c) TB/s | (d) dequant+GEMM us | (c)/(b) | (c)/(a) "
        "| (c)<=(d) |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    print(lines[0]); print(lines[1])
    worst = {n: True for n in batches}
    for name, K, M in shapes:
        copies = max(2, -(-(768 << 20) // (M * K)))
        gen = torch.Generator(device=dev).manual_seed(0)
        ws, q8, s8, q4, s4 = [], [], [], [], []
        for _ in range(copies):
            w = torch.randn(M, K, dtype=torch.bfloat16, device=dev,
                            generator=gen) * 0.02
            q, s = quantize_fp8_per_channel(w)
            ws.append(w); q8.append(q); s8.append(s)
            q, s = quantize_mxfp4(w)
            q4.append(q); s4.append(s)
        torch.cuda.empty_cache()
        for N in batches:
            x = torch.randn(N, K, dtype=torch.bfloat16, device=dev,
                            generator=gen) / 8
            out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)

            def fa(i):
                return ops.linear(x, ws[i])

            def fb(i):
                kserve_amd_C.skinny_gemm_w8(out, x, q8[i], s8[i])

            def fc(i):
                kserve_amd_C.skinny_gemm_w4(out, x, q4[i], s4[i])

            def fd(i):
                return ops.linear_w4(x, q4[i], s4[i])

            iters = max(args.iters, 2 * copies)
            res = {"a": [], "b": [], "c": [], "d": []}
            keep = ops.W4_MAX_TOKENS
            try:
                for r in range(rounds + 1):  # round 0 is warm-up
                    for key, fn in (("a", fa), ("b", fb), ("c", fc), ("d", fd)):
                        ops.W4_MAX_TOKENS = 0 if key == "d" else keep
                        t = timed(fn, copies, iters)
                        if r:
                            res[key].append(t)
            finally:
                ops.W4_MAX_TOKENS = keep
            a, b, c, d = (statistics.median(res[k]) for k in "abcd")
            spread = max(
                (max(res[k]) - min(res[k])) / statistics.median(res[k])
                for k in "abcd"
            )
            ok = c <= d
            worst[N] = worst[N] and ok
            w4_bytes = M * K // 2 + M * K // 32
            line = (
                f"| {name} | {K} | {M} | {N} | {a:.1f} | "
                f"{M * K * 2 / a / 1e6:.2f} | {b:.1f} | {M * K / b / 1e6:.2f} "
                f"| {c:.1f} | {w4_bytes / c / 1e6:.2f} | {d:.1f} "
                f"| {c / b:.2f} | {c / a:.2f} | {'yes' if ok else 'no'} |"
            )
            print(line + f"  spread {spread:.0%}", flush=True)
            lines.append(line)
        del ws, q8, s8, q4, s4
        torch.cuda.empty_cache()
    # largest N such that (c) <= (d) on all four shapes and every smaller
    # measured N (0 if none)
    chosen = 0
    for n in batches:
        if not worst[n]:
            break
        chosen = n
    tail = f"\nW4_MAX_TOKENS by this table: {chosen}"
    print(tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + tail + "\n")


if args.w8:
    bench_w8()
    sys.exit(0)
if args.w4:
    bench_w4()
    sys.exit(0)


def bench_custom(x, w, iters):
    out = torch.empty(x.shape[0], w.shape[0], dtype=torch.bfloat16, device=dev)
    for _ in range(10):
        kserve_amd_C.skinny_gemm(out, x, w)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        kserve_amd_C.skinny_gemm(out, x, w)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1000

print(f"{'shape':18s} {'N':>6s} {'K':>6s} {'M':>7s} {'us':>9s} {'TB/s(w)':>8s} {'TFLOP/s':>8s} {'cust_us':>8s} {'cust_TB/s':>9s}")
for name, N, K, M in SHAPES:
    x = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
    w = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
    for _ in range(10):
        y = F.linear(x, w)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        y = F.linear(x, w)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / args.iters * 1000
    wbytes = M * K * 2
    tbs = wbytes / (us * 1e-6) / 1e12
    tf = 2 * N * K * M / (us * 1e-6) / 1e12
    cus, ctbs = float("nan"), float("nan")
    if N <= 256 and M % 64 == 0 and K % 64 == 0:
        cus = bench_custom(x, w, args.iters)
        ctbs = wbytes / (cus * 1e-6) / 1e12
    print(f"{name:18s} {N:6d} {K:6d} {M:7d} {us:9.1f} {tbs:8.2f} {tf:8.1f} {cus:8.1f} {ctbs:9.2f}")
