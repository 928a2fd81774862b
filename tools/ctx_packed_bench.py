#!/usr/bin/env python3
"""Paged-context attention for short query runs: the tiled kernel against the
GQA-packed split-KV kernel, per shape, with a sweep over forced split counts
next to the host rule's choice. Prints a markdown table: medians of REPS
device-event windows of at least WINDOW_MS each (the iteration count is scaled
to the cell), the kernels alternating within a repetition, the spread
(max - min) / median of the repetitions, GB/s of unique KV for the packed
kernel.

  python tools/ctx_packed_bench.py [--quick] [--out FILE]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kserve_amd import ops

MODELS = {"8b": (32, 8, (2, 4, 8, 16)), "70b-tp8": (8, 1, (8,))}
CONTEXTS = (512, 2048, 8192)
SEQS = (1, 16, 64, 256)
SWEEP = (1, 2, 4, 8, 16, 32)
D = 128


def inputs(S, Hq, Hkv, q_len, ctx, fp8, dev):
    g = torch.Generator(device=dev).manual_seed(S * 131 + ctx + q_len)
    nb = -(-ctx // 16)
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc = torch.randn(S * nb + 1, Hkv, 16, D, device=dev, generator=g,
                     dtype=torch.bfloat16).to(cdt)
    vc = torch.randn(S * nb + 1, Hkv, 16, D, device=dev, generator=g,
                     dtype=torch.bfloat16).to(cdt)
    perm = torch.randperm(S * nb, device=dev, generator=g) + 1
    bt = perm.view(S, nb).to(torch.int32).contiguous()
    q = torch.randn(S * q_len, Hq, D, device=dev, generator=g,
                    dtype=torch.bfloat16)
    cu = torch.arange(0, (S + 1) * q_len, q_len, device=dev, dtype=torch.int32)
    cl = torch.full((S,), ctx, device=dev, dtype=torch.int32)
    return q, kc, vc, bt, cu, cl


def window_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def time_all(fns, window, reps):
    """{name: (median ms, spread)} of the callables in ``fns``: each is
    warmed up, its iteration count sized so a window lasts ``window`` ms, and
    the callables alternate within each of ``reps`` repetitions."""
    iters = {}
    for name, fn in fns.items():
        fn()
        fn()
        torch.cuda.synchronize()
        est = max(window_ms(fn, 5), 1e-3)
        iters[name] = max(5, min(20000, int(window / est) + 1))
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(window_ms(fn, iters[name]))
    out = {}
    for name, t in times.items():
        med = statistics.median(t)
        out[name] = (med, (max(t) - min(t)) / med)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="one small shape per model, for a rehearsal")
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    scale = D ** -0.5
    lines = [
        "| model | cache | q_len | ctx | seqs | tiled ms | packed ms (rule n) |"
        " spread t/p | speedup | packed GB/s | best forced n: ms |"
        " rule / best | max abs diff |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for name, (Hq, Hkv, q_lens) in MODELS.items():
        for fp8 in (False, True):
            for q_len in (q_lens[:1] if args.quick else q_lens):
                for ctx in (CONTEXTS[:1] if args.quick else CONTEXTS):
                    for S in (SEQS[1:2] if args.quick else SEQS):
                        q, kc, vc, bt, cu, cl = inputs(
                            S, Hq, Hkv, q_len, ctx, fp8, dev)

                        def run(kernel, splits=0):
                            return ops.context_attention_varlen(
                                q, kc, vc, bt, cu, cl, q_len, scale,
                                kernel=kernel, splits=splits)

                        ref = run("tiled")
                        diff = (run("packed").float() - ref.float()).abs().max()
                        pairs = max(1, (bt.shape[1] + 1) // 2)
                        n_rule = ops.ctx_packed_splits(S, Hkv, pairs)
                        fns = {"tiled": lambda: run("tiled"),
                               "rule": lambda: run("packed")}
                        for n in SWEEP:   # sets the rule's constants
                            if n <= pairs:
                                fns[n] = lambda n=n: run("packed", n)
                        res = time_all(fns, args.window_ms, args.reps)
                        (t_tiled, s_tiled), (t_rule, s_rule) = (
                            res["tiled"], res["rule"])
                        best = min((res[n][0], n) for n in fns
                                   if isinstance(n, int))[::-1]
                        kv_bytes = 2 * S * ctx * Hkv * D * (1 if fp8 else 2)
                        lines.append(
                            f"| {name} | {'fp8' if fp8 else 'bf16'} | {q_len} "
                            f"| {ctx} | {S} | {t_tiled:.4f} "
                            f"| {t_rule:.4f} ({n_rule}) "
                            f"| {s_tiled:.0%} / {s_rule:.0%} "
                            f"| {t_tiled / t_rule:.2f}x "
                            f"| {kv_bytes / t_rule / 1e6:.0f} "
                            f"| {best[0]}: {best[1]:.4f} "
                            f"| {t_rule / best[1]:.2f} | {diff:.4f} |")
                        print(lines[-1], flush=True)
                        del q, kc, vc, bt, cu, cl, ref
                        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
