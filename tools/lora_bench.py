#!/usr/bin/env python3
"""Multi-LoRA decode-step time on a Llama-3-8B-shaped layer stack (random
weights, synthetic rank-16 adapters on all seven modules of every layer).

For batch sizes 8/64/256 and 1/4/8 distinct adapters interleaved round-robin
over the rows, one decode step (ModelRunner.execute_decode: host staging,
forward, logits) is timed on three paths:

  (a) segments  KS_LORA_SEGMENTS=1, eager: the per-segment GEMM loop
  (b) batched   ops.lora_shrink / ops.lora_expand_add, eager
  (c) graph     the batched kernels replayed from the LoRA decode hipGraph

plus the base-model graph step at the same batch (no adapter rows). Each
figure is the median over rounds of a host clock around `steps` steps that
end in a device synchronise; the paths alternate within a round, after a
warm-up of every path. Prints a markdown table and one JSON line.

Run (GPU box): python tools/lora_bench.py [--layers 8] [--out DIR]
"""

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH_SIZES = (8, 64, 256)
ADAPTERS = (1, 4, 8)
RANK = 16
CTX = 128  # tokens already in the KV cache of every request


class _Blocks:
    """The two BlockManager calls ModelRunner's decode staging makes."""

    def __init__(self, per_req):
        self.per_req = per_req

    def get_block_table(self, req):
        return req.blocks

    def table_seq(self, request_id):
        return 0


def _batch(n, n_adapters, block_size):
    nb = CTX // block_size + 1
    reqs = []
    for i in range(n):
        reqs.append(SimpleNamespace(
            request_id=f"r{i}",
            lora_id=(i % n_adapters) + 1 if n_adapters else 0,
            num_computed_tokens=CTX,
            all_token_ids=[(7 * i + j) % 100 for j in range(CTX + 1)],
            blocks=list(range(1 + i * nb, 1 + (i + 1) * nb)),
        ))
    return SimpleNamespace(requests=reqs), _Blocks(nb)


def _install_adapters(engine, n, seed=0):
    import torch

    from kserve_amd.engine.lora import (
        ALL_MODULES, LoRAAdapter, LoRALayerWeights,
    )

    m = engine.config.model
    qd, kvd = m.num_heads * m.head_dim, m.num_kv_heads * m.head_dim
    dims = {  # module -> (out, in)
        "q_proj": (qd, m.hidden_size), "k_proj": (kvd, m.hidden_size),
        "v_proj": (kvd, m.hidden_size), "o_proj": (m.hidden_size, qd),
        "gate_proj": (m.intermediate_size, m.hidden_size),
        "up_proj": (m.intermediate_size, m.hidden_size),
        "down_proj": (m.hidden_size, m.intermediate_size),
    }
    mgr = engine.get_lora_manager()
    g = torch.Generator(device="cpu").manual_seed(seed)
    for i in range(n):
        ad = LoRAAdapter(mgr.next_adapter_id(), f"bench-{i}", RANK)
        for layer in range(m.num_layers):
            for mod in ALL_MODULES:
                out, inp = dims[mod]
                a = torch.randn(RANK, inp, generator=g) * 0.02
                b = torch.randn(out, RANK, generator=g) * 0.02
                ad.weights[(layer, mod)] = LoRALayerWeights(
                    a.to(engine.model.dtype).to(engine.device),
                    b.to(engine.model.dtype).to(engine.device), 2.0)
        mgr.install(ad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8,
                    help="decoder layers of Llama-3-8B shape (the model has 32)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--segment-steps", type=int, default=2,
                    help="steps per round of path (a), which is far slower")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for lora_bench.json")
    args = ap.parse_args()

    import torch

    assert torch.cuda.is_available(), "lora_bench needs a GPU"
    from kserve_amd import ops
    from kserve_amd.engine.config import (
        CacheConfig, EngineConfig, ModelConfig, SchedulerConfig,
    )
    from kserve_amd.engine.engine import LLMEngine

    assert ops.has_native()
    model = ModelConfig.llama3_8b()
    model.num_layers = args.layers
    bs = 16
    max_bs = max(BATCH_SIZES)
    cfg = EngineConfig(
        model=model,
        cache=CacheConfig(block_size=bs,
                          num_gpu_blocks=1 + max_bs * (CTX // bs + 1)),
        scheduler=SchedulerConfig(max_num_seqs=max_bs,
                                  max_num_batched_tokens=8192,
                                  max_model_len=1024),
        device="cuda", eos_token_id=-1, enforce_eager=False,
    )
    engine = LLMEngine(cfg)
    _install_adapters(engine, max(ADAPTERS))
    runner = engine.runner
    assert engine.lora_manager.has_stacks

    def step(batch, blocks):
        return runner.execute_decode(batch, blocks)

    def set_path(path):
        os.environ["KS_LORA_SEGMENTS"] = "1" if path == "segments" else "0"
        runner.config.enforce_eager = path in ("segments", "batched")

    def timed(path, batch, blocks, steps):
        set_path(path)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(batch, blocks)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    rows = []
    print(f"# {args.layers} layers, rank {RANK}, ctx {CTX}; ms per decode step")
    print("| batch | adapters | (a) segments | (b) batched | (c) graph "
          "| base graph | a/b | b/c | c/base |")
    print("|---|---|---|---|---|---|---|---|---|", flush=True)
    for n in BATCH_SIZES:
        base_batch = _batch(n, 0, bs)
        for na in ADAPTERS:
            batch, blocks = _batch(n, na, bs)
            paths = {
                "segments": (batch, args.segment_steps),
                "batched": (batch, args.steps),
                "graph": (batch, args.steps),
                "base_graph": (base_batch[0], args.steps),
            }
            ms = {p: [] for p in paths}
            for p, (b, _) in paths.items():      # warm-up (and graph capture)
                timed(p, b, blocks, 2 if p != "segments" else 1)
            if na == ADAPTERS[0]:
                # same tokens from the three paths' first row, as a sanity
                # check that they compute the same step
                tops = {}
                for p in ("segments", "batched", "graph"):
                    set_path(p)
                    tops[p] = step(batch, blocks).float().argmax(-1).tolist()
                agree = sum(a == b for a, b in zip(tops["batched"], tops["graph"]))
                agree_seg = sum(a == b for a, b in zip(tops["batched"], tops["segments"]))
                print(f"# bs={n}: argmax agreement batched/graph {agree}/{n}, "
                      f"batched/segments {agree_seg}/{n}", flush=True)
            for _ in range(args.rounds):
                for p, (b, steps) in paths.items():
                    ms[p].append(timed(p, b, blocks, steps))
            med = {p: statistics.median(v) for p, v in ms.items()}
            spread = {p: (min(v), max(v)) for p, v in ms.items()}
            rows.append(dict(batch=n, adapters=na, ms=med, spread=spread))
            print(f"| {n} | {na} | {med['segments']:.2f} | {med['batched']:.2f} "
                  f"| {med['graph']:.2f} | {med['base_graph']:.2f} "
                  f"| {med['segments'] / med['batched']:.1f}x "
                  f"| {med['batched'] / med['graph']:.2f}x "
                  f"| {med['graph'] / med['base_graph']:.2f} |", flush=True)
    set_path("graph")
    result = dict(bench="lora_decode", layers=args.layers, rank=RANK, ctx=CTX,
                  steps=args.steps, segment_steps=args.segment_steps,
                  rounds=args.rounds, rows=rows)
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "lora_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
