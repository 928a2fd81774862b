#!/usr/bin/env python3
"""In-graph logit processors on a Llama-3-8B-shaped model (V = 128256, random
weights), batch sizes 8/64/256:

  (a) replay   ms per replay of the processed graph (logit_process +
               min-p sampler + token_count_add inside) against the sampled
               graph, both through ModelRunner.multi_step_decode, every row
               holding a state slot: the cost of the in-graph processors
  (b) tok/s    output tokens per second of a batch in which every request
               sets repetition_penalty=1.1, frequency_penalty=0.2 (greedy),
               on an engine with logit_processor_slots=0 (single steps, host
               Sampler: the path without this feature) and on one with
               slots = 256 (processed windows)

Each figure is the median over rounds, min-max beside it; the two sides
alternate within a round after a warm-up of both; every clock brackets a
device synchronise. Prints markdown tables and one JSON line.

Run (GPU box): python tools/logit_process_bench.py [--layers 8] [--out DIR]
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
CTX = 128      # (a): tokens already in the KV cache of every request
HISTORY = 64   # (a): output tokens already counted per request
PROMPT = 32    # (b): prompt tokens per request


class _Blocks:
    """The two BlockManager calls ModelRunner's decode staging makes."""

    def get_block_table(self, req):
        return req.blocks

    def table_seq(self, request_id):
        return 0


def _batch(n, block_size, k_steps, sp):
    nb = (CTX + k_steps) // block_size + 1
    reqs = []
    for i in range(n):
        toks = [(7 * i + j) % 1000 for j in range(CTX + 1)]
        reqs.append(SimpleNamespace(
            request_id=f"r{i}", lora_id=0, sampling_params=sp,
            num_computed_tokens=CTX, all_token_ids=toks,
            output_token_ids=toks[-HISTORY:],
            blocks=list(range(1 + i * nb, 1 + (i + 1) * nb)),
        ))
    return SimpleNamespace(requests=reqs), _Blocks()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8,
                    help="decoder layers of Llama-3-8B shape (the model has 32)")
    ap.add_argument("--steps", type=int, default=16,
                    help="(a): replays per timed window")
    ap.add_argument("--max-tokens", type=int, default=33,
                    help="(b): output tokens per request (1 + windows of 8)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None,
                    help="directory for logit_process_bench.json")
    args = ap.parse_args()

    import torch

    assert torch.cuda.is_available(), "logit_process_bench needs a GPU"
    from kserve_amd import ops
    from kserve_amd.engine.config import (
        CacheConfig, EngineConfig, ModelConfig, SchedulerConfig,
    )
    from kserve_amd.engine.engine import LLMEngine
    from kserve_amd.engine.sampling_params import SamplingParams

    assert ops.has_native()
    bs = 16
    max_bs = max(BATCH_SIZES)
    per_req = max((CTX + args.steps) // bs + 1,
                  (PROMPT + args.max_tokens + 8) // bs + 1)

    def make_engine(slots):
        model = ModelConfig.llama3_8b()
        model.num_layers = args.layers
        return LLMEngine(EngineConfig(
            model=model,
            cache=CacheConfig(block_size=bs,
                              num_gpu_blocks=2 + max_bs * (per_req + 1)),
            scheduler=SchedulerConfig(
                max_num_seqs=max_bs, max_num_batched_tokens=8192,
                max_model_len=1024, logit_processor_slots=slots),
            device="cuda", eos_token_id=-1, enforce_eager=False,
        ))

    host = make_engine(0)
    dev = make_engine(max_bs)
    runner = dev.runner
    state = runner.logit_state
    vocab = dev.config.model.vocab_size

    # ---- (a) one replay, processed against sampled -------------------------
    sp_a = SamplingParams(temperature=0.8, top_p=0.95, top_k=40,
                          repetition_penalty=1.1, frequency_penalty=0.2)
    rows_a = []
    print(f"# (a) {args.layers} layers, V={vocab}, ctx {CTX}, {HISTORY} counted "
          f"tokens per row; ms per replay, median (min-max) of {args.rounds}")
    print("| batch | sampled graph | processed graph | difference | "
          "bytes/step at 8 B x V x rows | implied GB/s |")
    print("|---|---|---|---|---|---|", flush=True)
    for n in BATCH_SIZES:
        batch, blocks = _batch(n, bs, args.steps, sp_a)
        for r in batch.requests:
            assert state.acquire(r) is not None
        state.catch_up(batch.requests)

        def timed(processed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.multi_step_decode(batch, blocks, args.steps,
                                     sampled=True, processed=processed)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        ms = {False: [], True: []}
        for p in (False, True):      # warm-up (and graph capture)
            timed(p)
        for _ in range(args.rounds):
            for p in (False, True):
                ms[p].append(timed(p))
        for r in batch.requests:
            state.release(r.request_id)
        med = {p: statistics.median(v) for p, v in ms.items()}
        diff = med[True] - med[False]
        nbytes = 8 * vocab * n
        rows_a.append(dict(batch=n, sampled_ms=ms[False], processed_ms=ms[True]))
        fmt = lambda v: (f"{statistics.median(v):.3f} "
                         f"({min(v):.3f}-{max(v):.3f})")
        gbs = nbytes / (diff * 1e-3) / 1e9 if diff > 0 else float("nan")
        print(f"| {n} | {fmt(ms[False])} | {fmt(ms[True])} | {diff:+.3f} "
              f"| {nbytes / 1e6:.0f} MB | {gbs:.0f} |", flush=True)

    # ---- (b) end to end, slots = 0 against slots = batch ---------------------
    sp_b = SamplingParams(temperature=0.0, max_tokens=args.max_tokens,
                          ignore_eos=True, repetition_penalty=1.1,
                          frequency_penalty=0.2)

    def run(engine, n):
        prompts = [[(11 * i + j) % 1000 + 1 for j in range(PROMPT)]
                   for i in range(n)]
        for i, p in enumerate(prompts):
            engine.add_request(p, sp_b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        while engine.has_unfinished():
            for o in engine.step():
                if o.finished:
                    done += len(o.output_token_ids)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert done == n * args.max_tokens, (done, n)
        return done / dt

    rows_b = []
    print(f"\n# (b) {args.layers} layers, {PROMPT}-token prompts, "
          f"{args.max_tokens} output tokens, greedy + repetition_penalty=1.1 "
          f"+ frequency_penalty=0.2 on every request; output tok/s incl. "
          f"prefill, median (min-max) of {args.rounds}")
    print("| batch | slots=0 (host path) | slots=256 (processed windows) "
          "| ratio of medians |")
    print("|---|---|---|---|", flush=True)
    for n in BATCH_SIZES:
        tps = {"host": [], "dev": []}
        run(host, n)
        run(dev, n)
        for _ in range(args.rounds):
            tps["host"].append(run(host, n))
            tps["dev"].append(run(dev, n))
        rows_b.append(dict(batch=n, host_tok_s=tps["host"], dev_tok_s=tps["dev"]))
        fmt = lambda v: (f"{statistics.median(v):.0f} "
                         f"({min(v):.0f}-{max(v):.0f})")
        ratio = statistics.median(tps["dev"]) / statistics.median(tps["host"])
        print(f"| {n} | {fmt(tps['host'])} | {fmt(tps['dev'])} "
              f"| {ratio:.2f}x |", flush=True)

    result = dict(bench="logit_processors", layers=args.layers, vocab=vocab,
                  steps=args.steps, max_tokens=args.max_tokens,
                  rounds=args.rounds, replay=rows_a, end_to_end=rows_b)
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "logit_process_bench.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
