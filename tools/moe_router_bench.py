#!/usr/bin/env python3
"""Microbench the MoE router (profiles/moe_routed.md, "Router"): the fused
HIP router (ops.moe_route) against the four torch lines of
MixtralMoE.forward, per token batch, eagerly and as a captured-graph replay.

Run on GPU: python tools/moe_router_bench.py [--out FILE.md]

Each call takes another copy of x and of the gate (8 of each), as consecutive
layers do. Times are medians of interleaved rounds in microseconds per call;
"spread" is (max - min) / median over the rounds of the fused column. A graph
holds 32 calls (one per layer of a Mixtral-8x7B) and its time is per call.
"rows !=" counts rows whose expert ids differ between the two (near-ties that
the fp32 library GEMM's summation order decides differently).
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kserve_amd import ops

parser = argparse.ArgumentParser()
parser.add_argument("--out", default=None, help="also write the table here")
parser.add_argument("--rounds", type=int, default=5)
args = parser.parse_args()

assert torch.cuda.is_available()
dev = "cuda:0"
COPIES, LAYERS, GRAPH_MAX_T = 8, 32, 384
CELLS = [  # (E, k, H, token batches)
    (8, 2, 4096, [1, 16, 64, 256, 384, 2048, 8192]),
    (128, 8, 2048, [1, 64, 384, 2048, 8192]),
]


def torch_router(x, gate, k):
    logits = torch.nn.functional.linear(x.float(), gate.float())
    probs = torch.softmax(logits, dim=-1)
    topw, topi = probs.topk(k, dim=-1)
    return topi, topw / topw.sum(dim=-1, keepdim=True)


def timed(fn, iters):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1000


def ab(fns, iters):
    """Median us per variant and the spread of the last, rounds interleaved."""
    for fn in fns:
        timed(fn, 3)
    runs = [[timed(fn, iters) for fn in fns] for _ in range(args.rounds)]
    cols = list(zip(*runs))
    med = [statistics.median(c) for c in cols]
    return med, (max(cols[-1]) - min(cols[-1])) / med[-1]


def graphed(router, xs, gates, k):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [router(xs[i % COPIES], gates[i % COPIES], k)
                for i in range(LAYERS)]
    return graph, keep


lines = [
    "| E | k | H | T | torch us | fused us | speed-up | spread | "
    "graph torch us | graph fused us | speed-up | rows != |",
    "|---|---|---|---|---|---|---|---|---|---|---|---|",
]
for E, k, H, batches in CELLS:
    g = torch.Generator().manual_seed(E)
    gates = [(torch.randn(E, H, generator=g) / H ** 0.5).bfloat16().to(dev)
             for _ in range(COPIES)]
    for T in batches:
        xs = [torch.randn(T, H, generator=g).bfloat16().to(dev)
              for _ in range(COPIES)]
        fns = [
            lambda i, r=r: r(xs[i % COPIES], gates[i % COPIES], k)
            for r in (torch_router, ops.moe_route)
        ]
        iters = 200 if T <= 2048 else 50
        (t_us, f_us), spread = ab(fns, iters)
        ti, _ = torch_router(xs[0], gates[0], k)
        fi, _ = ops.moe_route(xs[0], gates[0], k)
        differ = int((ti != fi).any(-1).sum())
        cells = ["-", "-", "-"]
        if T <= GRAPH_MAX_T:
            graphs = [graphed(r, xs, gates, k)
                      for r in (torch_router, ops.moe_route)]
            (gt, gf), _ = ab([lambda i, gr=gr: gr[0].replay() for gr in graphs],
                             20)
            cells = [f"{gt / LAYERS:.1f}", f"{gf / LAYERS:.1f}",
                     f"{gt / gf:.2f}x"]
        lines.append(
            f"| {E} | {k} | {H} | {T} | {t_us:.1f} | {f_us:.1f} | "
            f"{t_us / f_us:.2f}x | {spread:.1%} | " + " | ".join(cells)
            + f" | {differ} |"
        )
        print(lines[-1], flush=True)

table = "\n".join(lines)
print(table)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(table + "\n")
