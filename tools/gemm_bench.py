#!/usr/bin/env python3
"""Microbench the decode-path GEMM shapes: achieved TB/s (weight traffic) per
shape, to judge hipBLASLt (tuned/untuned) against the HBM roofline.

Run on GPU: python tools/gemm_bench.py [--tune]
            python tools/gemm_bench.py --w8 [--out FILE.md]
            python tools/gemm_bench.py --w4 [--out FILE.md]
            python tools/gemm_bench.py --wq-tile [--out FILE.md]
            python tools/gemm_bench.py --moe [--out FILE.md]
            python tools/gemm_bench.py --moe-prefill [--out FILE.md]

--w8 is the A/B behind ops.W8_MAX_TOKENS (profiles/w8_gemm.md): per
Llama-3-8B projection shape and token batch it times, in one process and
interleaved, (a) ops.linear on bf16 weights, (b) the fp8-weight skinny GEMM
and (c) dequant + hipBLASLt, the path ops.linear_w8 takes above the
threshold.

--w4 is the same A/B behind ops.W4_MAX_TOKENS (profiles/w4_gemm.md), with
the columns (a) ops.linear on bf16 weights, (b) the fp8-weight skinny GEMM,
(c) the MXFP4-weight skinny GEMM and (d) MXFP4 dequant + hipBLASLt.

--wq-tile is the A/B behind ops.WQ_TILE_MAX_TOKENS (profiles/
wq_tile_gemm.md), same method, for both formats at N = 129..4096: (a)
ops.linear on bf16 weights, (c) dequant + hipBLASLt and (d) the fused-dequant
tile GEMM, in its remapped and its plain grid order, then forced K splits on
the shapes the (M, K) policy splits.

--moe is the A/B behind MixtralMoE.ROUTED_MAX_TOKENS (profiles/
moe_routed.md): one Mixtral-8x7B MoE layer per token batch, the routed
grouped kernels (ops.moe_routed_mlp) against the dense-bmm path.

--moe-prefill is the A/B behind MixtralMoE.ROUTED_PREFILL_MAX_TOKENS (same
profile, "Prefill"): the same layer at prefill batches, the routed prefill
kernels (ops.moe_routed_prefill_mlp) against the sparse per-expert loop.
With --quantization both sides run fp8 / MXFP4 experts and the bf16 prefill
kernels are timed alongside for orientation.
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
parser.add_argument("--wq-tile", action="store_true",
                    help="fused-dequant tile GEMM A/B table, fp8 and MXFP4 "
                         "(profiles/wq_tile_gemm.md)")
parser.add_argument("--moe", action="store_true",
                    help="routed MoE MLP against the dense-bmm path, one "
                         "Mixtral-8x7B layer (profiles/moe_routed.md)")
parser.add_argument("--moe-prefill", action="store_true",
                    help="routed MoE prefill MLP against the sparse loop, "
                         "one Mixtral-8x7B layer (profiles/moe_routed.md)")
parser.add_argument("--quantization", choices=("fp8", "mxfp4"), default=None,
                    help="--moe: the routed layer with experts in this "
                         "format against the routed bf16 layer; "
                         "--moe-prefill: both sides of the A/B with experts "
                         "in this format")
parser.add_argument("--out", default=None,
                    help="--w8/--w4/--moe: also write the table as markdown "
                         "here")
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


def bench_wq_tile():
    """bench_w8's method (interleaved rounds, a weight set larger than the
    Infinity Cache) above the skinny GEMMs' range. (d) is the tile GEMM with
    the policy's split in the remapped grid order, (d plain) the same in the
    plain order. The second table forces the split count where the policy
    splits."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.ops.quant import quantize_fp8_per_channel, quantize_mxfp4

    shapes = [  # (name, K in, M out): Llama-3-8B projections
        ("qkv", 4096, 6144),
        ("o", 4096, 4096),
        ("gate_up", 4096, 28672),
        ("down", 14336, 4096),
    ]
    batches = [129, 256, 512, 1024, 1536, 2048, 4096]
    split_batches = [256, 1536]
    rounds = 5
    formats = {
        "fp8": (quantize_fp8_per_channel, ops.linear_w8,
                kserve_amd_C.wq_tile_gemm_w8),
        "mxfp4": (quantize_mxfp4, ops.linear_w4, kserve_amd_C.wq_tile_gemm_w4),
    }
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

    def medians(fns, copies, iters):
        res = {k: [] for k in fns}
        for r in range(rounds + 1):  # round 0 is warm-up
            for key, fn in fns.items():
                t = timed(fn, copies, iters)
                if r:
                    res[key].append(t)
        spread = max(
            (max(v) - min(v)) / statistics.median(v) for v in res.values()
        )
        return {k: statistics.median(v) for k, v in res.items()}, spread

    out_lines = []

    def emit(line, note=""):
        print(line + note, flush=True)
        out_lines.append(line)

    for fmt, (quantize, linear_wq, tile) in formats.items():
        emit(f"\n## {fmt}\n")
        emit("| shape | K | M | S | N | (a) bf16 us | (c) dequant+GEMM us "
             "| (d) tile us | (d plain) us | (c)/(a) | (d)/(a) | (d)<=(c) |")
        emit("|---|---|---|---|---|---|---|---|---|---|---|---|")
        wins = {n: True for n in batches}
        sweep = []
        for name, K, M in shapes:
            copies = max(2, -(-(768 << 20) // (M * K)))
            gen = torch.Generator(device=dev).manual_seed(0)
            ws, qs, ss = [], [], []
            for _ in range(copies):
                w = torch.randn(M, K, dtype=torch.bfloat16, device=dev,
                                generator=gen) * 0.02
                q, sc = quantize(w)
                ws.append(w); qs.append(q); ss.append(sc)
            S = kserve_amd_C.wq_tile_nsplit(M, K)
            for N in batches:
                x = torch.randn(N, K, dtype=torch.bfloat16, device=dev,
                                generator=gen) / 8
                out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
                iters = max(min(args.iters, 20), 2 * copies)
                fns = {
                    "a": lambda i: ops.linear(x, ws[i]),
                    "c": lambda i: linear_wq(x, qs[i], ss[i]),
                    "d": lambda i: tile(out, x, qs[i], ss[i], None, 0, False),
                    "p": lambda i: tile(out, x, qs[i], ss[i], None, 0, True),
                }
                t, spread = medians(fns, copies, iters)
                # (d), the order ops dispatches, decides; (d plain) is
                # recorded beside it
                wins[N] = wins[N] and t["d"] <= t["c"]
                emit(f"| {name} | {K} | {M} | {S} | {N} | {t['a']:.1f} | "
                     f"{t['c']:.1f} | {t['d']:.1f} | {t['p']:.1f} | "
                     f"{t['c'] / t['a']:.2f} | {t['d'] / t['a']:.2f} | "
                     f"{'yes' if t['d'] <= t['c'] else 'no'} |",
                     f"  spread {spread:.0%}")
                if S > 1 and N in split_batches:
                    forced = {
                        s_: (lambda i, s_=s_: tile(out, x, qs[i], ss[i], None,
                                                   s_, False))
                        for s_ in (1, 2, 4, 8)
                    }
                    ts, _ = medians(forced, copies, iters)
                    sweep.append(
                        f"| {name} | {K} | {M} | {N} | "
                        + " | ".join(f"{ts[s_]:.1f}" for s_ in (1, 2, 4, 8))
                        + " |"
                    )
            del ws, qs, ss
            torch.cuda.empty_cache()
        emit("\nForced K splits (us), remapped order:\n")
        emit("| shape | K | M | N | S=1 | S=2 | S=4 | S=8 |")
        emit("|---|---|---|---|---|---|---|---|")
        for line in sweep:
            emit(line)
        # largest measured N up to which (d) <= (c) on all four shapes
        chosen = 0
        for n in batches:
            if not wins[n]:
                break
            chosen = n
        emit(f"\nWQ_TILE_MAX_TOKENS[{fmt!r}] by this table: {chosen}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")


def bench_moe():
    """One Mixtral-8x7B MoE layer (H 4096, I 14336, E 8, k 2), uniform
    random routing: ops.moe_routed_mlp against MixtralMoE._forward_dense on
    the same inputs, rounds interleaved, device-event timed, median and
    spread of the rounds. Bytes are the weights of the experts the batch
    routes to (what the routed path has to read), FLOPs those of the routed
    pairs (2 * T*k * 3*H*I); the bound is the larger of bytes / 8 TB/s and
    FLOPs / 2.5 PFLOP/s (MI355X HBM3E and dense bf16 MFMA peaks). The output
    check is the allowance of tests/test_gpu_moe_routed.py, computed here
    around the dense result."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    H, I, E, k = 4096, 14336, 8, 2
    PEAK_BW, PEAK_FLOPS = 8.0e12, 2.5e15
    rounds = 5
    cfg = ModelConfig.mixtral_8x7b()
    with torch.device(dev):
        moe = MixtralMoE(cfg, dtype=torch.bfloat16)
    gen = torch.Generator(device=dev).manual_seed(0)
    moe.w_gate_up.data.normal_(0, H ** -0.5, generator=gen)
    moe.w_down.data.normal_(0, I ** -0.5, generator=gen)

    def timed(fn, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1000

    lines = [
        "| T | experts routed | dense us | spread | routed us | spread "
        "| dense/routed | routed TB/s | routed TFLOP/s | bound | % of bound "
        "| max diff / allowance |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    print(lines[0]); print(lines[1])
    for T in (1, 4, 16, 64, 128, 256, 384):
        x = torch.randn(T, H, dtype=torch.bfloat16, device=dev, generator=gen)
        logits = torch.randn(T, E, device=dev, generator=gen)
        topw, topi = torch.softmax(logits, -1).topk(k, -1)
        topw = topw / topw.sum(-1, keepdim=True)

        def fd():
            return moe._forward_dense(x, topi, topw)

        def fr():
            return ops.moe_routed_mlp(
                x, topi, topw, moe.w_gate_up, moe.w_down, 0
            )

        iters = max(args.iters // 2, 10)
        res = {"d": [], "r": []}
        for r in range(rounds + 1):  # round 0 is warm-up
            for key, fn in (("d", fd), ("r", fr)):
                t = timed(fn, iters)
                if r:
                    res[key].append(t)
        d, rt = (statistics.median(res[key]) for key in "dr")
        sd, sr = (
            (max(res[key]) - min(res[key])) / statistics.median(res[key])
            for key in "dr"
        )
        routed = int(topi.unique().numel())
        wbytes = routed * 3 * H * I * 2
        flops = 2 * T * k * 3 * H * I
        t_bw, t_fl = wbytes / PEAK_BW * 1e6, flops / PEAK_FLOPS * 1e6
        bound = "bytes" if t_bw >= t_fl else "FLOPs"
        # allowance around the dense result (it is exact up to its own bf16
        # roundings): |act| @ |w_down| per routed pair, in f32
        ref = fd().float()
        allow = torch.zeros_like(ref)
        for e in range(E):
            t_idx, j_idx = (topi == e).nonzero(as_tuple=True)
            if t_idx.numel() == 0:
                continue
            act = ops.silu_and_mul(x[t_idx] @ moe.w_gate_up[e].t()).float()
            allow.index_add_(
                0, t_idx,
                (act.abs() @ moe.w_down[e].float().abs().t())
                * topw[t_idx, j_idx].unsqueeze(1),
            )
        allow = 2.0 ** -8 * ref.abs() + (2.0 ** -8 + (H + I) * 2.0 ** -23) * allow
        ratio = ((fr().float() - ref).abs() / allow).max().item()
        line = (
            f"| {T} | {routed} | {d:.1f} | {sd:.1%} | {rt:.1f} | {sr:.1%} "
            f"| {d / rt:.2f} | {wbytes / rt / 1e6:.2f} "
            f"| {flops / rt / 1e6:.1f} | {bound} "
            f"| {max(t_bw, t_fl) / rt:.0%} | {ratio:.3f} |"
        )
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def bench_moe_quant(q):
    """--moe --quantization q: the routed layer with fp8 / MXFP4 experts
    against the routed bf16 layer at the same T and routing, same process,
    rounds interleaved as in bench_moe. The quantized weights are the bf16
    layer's, quantized per expert. Bytes are what the routed experts occupy in
    the format (codes and scales); the bound is bytes at 8 TB/s or the routed
    FLOPs at 2.5 PFLOP/s, whichever is larger. Times are whole calls of
    ops.moe_routed_mlp (align, two GEMMs, combine and the workspace
    allocations), so TB/s and % of bound are layer figures, not kernel ones."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    H, I, E, k = 4096, 14336, 8, 2
    PEAK_BW, PEAK_FLOPS = 8.0e12, 2.5e15
    rounds = 5
    gen = torch.Generator(device=dev).manual_seed(0)
    qcfg = ModelConfig.mixtral_8x7b()
    qcfg.quantization, qcfg.moe_kernel = q, "routed"
    with torch.device(dev):
        ref = MixtralMoE(ModelConfig.mixtral_8x7b(), dtype=torch.bfloat16)
        moe = MixtralMoE(qcfg, dtype=torch.bfloat16)
    ref.w_gate_up.data.normal_(0, H ** -0.5, generator=gen)
    ref.w_down.data.normal_(0, I ** -0.5, generator=gen)
    fmt = moe.weight_format
    for e in range(E):
        for name in ("w_gate_up", "w_down"):
            codes, scale = fmt.shard_to_codes(getattr(ref, name)[e], None, dev)
            getattr(moe, name).data[e].copy_(codes)
            getattr(moe, name + "_scale").data[e].copy_(scale)
    per_expert = sum(
        t[0].numel() * t.element_size()
        for t in (moe.w_gate_up, moe.w_down, moe.w_gate_up_scale,
                  moe.w_down_scale)
    )

    def timed(fn, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1000

    lines = [
        f"| T | experts routed | bf16 us | spread | {q} us | spread "
        f"| bf16/{q} | {q} MB read | {q} TB/s | bound | % of bound |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    print(lines[0]); print(lines[1])
    for T in (1, 4, 16, 64, 128, 384):
        x = torch.randn(T, H, dtype=torch.bfloat16, device=dev, generator=gen)
        logits = torch.randn(T, E, device=dev, generator=gen)
        topw, topi = torch.softmax(logits, -1).topk(k, -1)
        topw = topw / topw.sum(-1, keepdim=True)

        def fb():
            return ops.moe_routed_mlp(
                x, topi, topw, ref.w_gate_up, ref.w_down, 0
            )

        def fq():
            return ops.moe_routed_mlp(
                x, topi, topw, moe.w_gate_up, moe.w_down, 0,
                gate_up_scale=moe.w_gate_up_scale,
                down_scale=moe.w_down_scale, quantization=q,
            )

        iters = max(args.iters, 10) * 4  # 200 calls: >= 15 ms per window
        res = {"b": [], "q": []}
        for r in range(rounds + 1):  # round 0 is warm-up
            for key, fn in (("b", fb), ("q", fq)):
                t = timed(fn, iters)
                if r:
                    res[key].append(t)
        b, qt = (statistics.median(res[key]) for key in "bq")
        sb, sq = (
            (max(res[key]) - min(res[key])) / statistics.median(res[key])
            for key in "bq"
        )
        routed = int(topi.unique().numel())
        wbytes = routed * per_expert
        flops = 2 * T * k * 3 * H * I
        t_bw, t_fl = wbytes / PEAK_BW * 1e6, flops / PEAK_FLOPS * 1e6
        line = (
            f"| {T} | {routed} | {b:.1f} | {sb:.1%} | {qt:.1f} | {sq:.1%} "
            f"| {b / qt:.2f} | {wbytes / 1e6:.0f} | {wbytes / qt / 1e6:.2f} "
            f"| {'bytes' if t_bw >= t_fl else 'FLOPs'} "
            f"| {max(t_bw, t_fl) / qt:.0%} |"
        )
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def bench_moe_prefill():
    """One Mixtral-8x7B MoE layer (H 4096, I 14336, E 8, k 2) at prefill
    batches: ops.moe_routed_prefill_mlp, in both grid orders, against
    MixtralMoE._forward_sparse on the same inputs. The method is bench_moe's:
    the variants alternate inside every round, device events around calls
    that end in a synchronise, median and spread of 5 rounds after a warm-up
    round. TFLOP/s from the routed pairs' 2 * T*k * 3*H*I, share of the
    2.5 PFLOP/s dense bf16 peak; times are whole calls (align, GEMMs,
    combine, workspace allocations; for the sparse loop its host
    synchronisations too). The check is the test allowance around the sparse
    result. The last row routes every token to the same two experts.

    --quantization q: both sides run the layer's weights quantized per expert
    to q (the sparse loop then dequantizes every expert it visits into the
    bf16 scratch, which is what MixtralMoE ran above 384 tokens before the
    kernels took these formats), and a last column times the bf16 prefill
    kernels on the same routing. The check column is then only orientation:
    the sparse side is the looser one (bf16 GEMM outputs and sums)."""
    import statistics

    from kserve_amd import ops
    from kserve_amd.engine.config import ModelConfig
    from kserve_amd.models.llama import MixtralMoE

    H, I, E, k = 4096, 14336, 8, 2
    PEAK_FLOPS = 2.5e15
    rounds = 5
    with torch.device(dev):
        moe = MixtralMoE(ModelConfig.mixtral_8x7b(), dtype=torch.bfloat16)
    gen = torch.Generator(device=dev).manual_seed(0)
    moe.w_gate_up.data.normal_(0, H ** -0.5, generator=gen)
    moe.w_down.data.normal_(0, I ** -0.5, generator=gen)
    q = args.quantization
    run, scales = moe, {}
    if q:
        qcfg = ModelConfig.mixtral_8x7b()
        qcfg.quantization, qcfg.moe_kernel = q, "routed"
        with torch.device(dev):
            run = MixtralMoE(qcfg, dtype=torch.bfloat16)
        for e in range(E):
            for name in ("w_gate_up", "w_down"):
                codes, scale = run.weight_format.shard_to_codes(
                    getattr(moe, name)[e], None, dev
                )
                getattr(run, name).data[e].copy_(codes)
                getattr(run, name + "_scale").data[e].copy_(scale)
        scales = dict(gate_up_scale=run.w_gate_up_scale,
                      down_scale=run.w_down_scale, quantization=q)

    def timed(fn, iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1000

    lines = [
        "| T | routing | sparse us | spread | feature-fastest us | spread "
        "| row-fastest us | spread | sparse/best | best TFLOP/s | % of peak "
        "| max diff / allowance |" + (" bf16 kernels us | spread |" if q else ""),
        "|---|---|---|---|---|---|---|---|---|---|---|---|"
        + ("---|---|" if q else ""),
    ]
    print(lines[0]); print(lines[1])
    cases = [(T, "uniform") for T in (512, 1024, 2048, 4096, 8192)]
    for T, mode in cases + [(2048, "two experts")]:
        x = torch.randn(T, H, dtype=torch.bfloat16, device=dev, generator=gen)
        logits = torch.randn(T, E, device=dev, generator=gen)
        topw, topi = torch.softmax(logits, -1).topk(k, -1)
        topw = topw / topw.sum(-1, keepdim=True)
        if mode != "uniform":
            topi = topi[:1].expand(T, k).contiguous()

        def fs():
            return run._forward_sparse(x, topi, topw)

        def fr(row_fast):
            ops.MOE_PREFILL_ROW_FAST = row_fast
            return ops.moe_routed_prefill_mlp(
                x, topi, topw, run.w_gate_up, run.w_down, 0, **scales
            )

        def fb():  # orientation: the bf16 kernels, default grid order
            ops.MOE_PREFILL_ROW_FAST = False
            return ops.moe_routed_prefill_mlp(
                x, topi, topw, moe.w_gate_up, moe.w_down, 0
            )

        variants = (("s", fs), ("f", lambda: fr(False)), ("r", lambda: fr(True)))
        if q:
            variants += (("b", fb),)
        iters = max(2, min(20, 16384 // T))  # >= 40 ms per window
        res = {key: [] for key, _ in variants}
        for r in range(rounds + 1):  # round 0 is warm-up
            for key, fn in variants:
                t = timed(fn, iters)
                if r:
                    res[key].append(t)
        med = {key: statistics.median(v) for key, v in res.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in res.items()}
        best = min(med["f"], med["r"])
        flops = 2 * T * k * 3 * H * I
        # allowance around the sparse result, |act| @ |w_down| per routed pair
        ref = fs().float()
        allow = torch.zeros_like(ref)
        for e in range(E):
            t_idx, j_idx = (topi == e).nonzero(as_tuple=True)
            if t_idx.numel() == 0:
                continue
            act = ops.silu_and_mul(x[t_idx] @ moe.w_gate_up[e].t()).float()
            allow.index_add_(
                0, t_idx,
                (act.abs() @ moe.w_down[e].float().abs().t())
                * topw[t_idx, j_idx].unsqueeze(1),
            )
        allow = 2.0 ** -8 * ref.abs() + (2.0 ** -8 + (H + I) * 2.0 ** -23) * allow
        ratio = ((fr(False).float() - ref).abs() / allow).max().item()
        line = (
            f"| {T} | {mode} | {med['s']:.0f} | {spread['s']:.1%} "
            f"| {med['f']:.0f} | {spread['f']:.1%} | {med['r']:.0f} "
            f"| {spread['r']:.1%} | {med['s'] / best:.2f} "
            f"| {flops / best / 1e6:.0f} | {flops / PEAK_FLOPS * 1e6 / best:.0%} "
            f"| {ratio:.3f} |"
        )
        if q:
            line += f" {med['b']:.0f} | {spread['b']:.1%} |"
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if args.moe_prefill:
    bench_moe_prefill()
    sys.exit(0)
if args.moe:
    if args.quantization:
        bench_moe_quant(args.quantization)
    else:
        bench_moe()
    sys.exit(0)
if args.wq_tile:
    bench_wq_tile()
    sys.exit(0)
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
