#!/usr/bin/env python3
"""Time KV export and import between an engine's paged pool and pinned host
memory, with the Llama-3-8B geometry (L=32, Hkv=8, block 16, D=128).

Export  = ops.kv_gather_pages + ONE device-to-host copy into pinned memory.
Import  = ONE host-to-device copy + ops.kv_scatter_pages.

Baselines, same pages and byte count:
  (a) loop  — one ``copy_`` per page per tensor between the pool and a pinned
              host pool, which is what ModelRunner.swap_blocks does today
              (reimplemented here; swap_blocks itself is not called);
  (b) floor — one pinned host<->device copy of the payload's byte count.

Every time is a host clock around work that ends in a stream synchronise,
after warm-up of the same shape; the variants of one row are alternated
inside each repetition and the median is reported with min and max.

Usage: python tools/kv_transfer_bench.py [--tokens 128 512 2048 8192]
                                         [--reps 7] [--out table.md]
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, HKV, BS, D = 32, 8, 16, 128


def make_pool(pages, dtype, device, seed):
    """[(K, V)] * L of finite, non-zero patterns (low seven bits of each byte
    in 1..126), generated on the device."""
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (pages, HKV, BS, D * dtype.itemsize)
    return [
        tuple(
            torch.randint(
                1, 127, shape, generator=g, dtype=torch.uint8, device=device
            ).view(dtype)
            for _ in range(2)
        )
        for _ in range(L)
    ]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_row(tokens, pool_dtype, out_dtype, reps, loop_reps):
    from kserve_amd import ops

    dev = torch.device("cuda")
    n = -(-tokens // BS)
    pages = max(2 * n, 64)
    pool = make_pool(pages, pool_dtype, dev, 1)
    dst_pool = make_pool(pages, out_dtype, dev, 2)
    g = torch.Generator().manual_seed(3)
    ids = torch.randperm(pages - 1, generator=g)[:n].add(1).tolist()
    nbytes = L * 2 * n * HKV * BS * D * out_dtype.itemsize
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    dev_flat = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # host pool of baseline (a): n pages per tensor, pinned
    host_pool = [
        tuple(
            torch.empty((n, HKV, BS, D), dtype=pool_dtype, pin_memory=True)
            for _ in range(2)
        )
        for _ in range(L)
    ]

    def export_new():
        buf = ops.kv_gather_pages(pool, ids, tokens, out_dtype=out_dtype)
        host.copy_(buf.view(torch.uint8).reshape(-1), non_blocking=True)

    def export_loop():
        for (gk, gv), (ck, cv) in zip(pool, host_pool):
            for j, b in enumerate(ids):
                ck[j].copy_(gk[b], non_blocking=True)
                cv[j].copy_(gv[b], non_blocking=True)

    def d2h_floor():
        host.copy_(dev_flat, non_blocking=True)

    def import_new():
        src = host.to(dev, non_blocking=True)
        ops.kv_scatter_pages(dst_pool, ids, src)

    def import_loop():
        for (gk, gv), (ck, cv) in zip(pool, host_pool):
            for j, b in enumerate(ids):
                gk[b].copy_(ck[j], non_blocking=True)
                gv[b].copy_(cv[j], non_blocking=True)

    def h2d_floor():
        dev_flat.copy_(host, non_blocking=True)

    variants = {
        "export": export_new, "d2h_floor": d2h_floor,
        "import": import_new, "h2d_floor": h2d_floor,
    }
    converting = pool_dtype != out_dtype
    if not converting:  # the loop cannot convert
        variants["export_loop"] = export_loop
        variants["import_loop"] = import_loop
    times = {k: [] for k in variants}
    for fn in variants.values():  # warm-up: every shape, twice
        timed(fn)
        timed(fn)
    for rep in range(reps):
        for name, fn in variants.items():
            if name.endswith("_loop") and rep >= loop_reps:
                continue
            times[name].append(timed(fn))
    # the export really is what the scatter then restores
    export_new()
    import_new()
    torch.cuda.synchronize()
    back = ops.kv_gather_pages(dst_pool, ids, tokens)
    assert torch.equal(back.view(torch.uint8).reshape(-1).cpu(), host)
    return nbytes, {
        k: (statistics.median(v), min(v), max(v)) for k, v in times.items()
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tokens", type=int, nargs="*",
                    default=[128, 512, 2048, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-reps", type=int, default=3,
                    help="repetitions of the per-page loop baseline")
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("kv_transfer_bench needs a GPU: nothing is measured without one")
    bf16, fp8 = torch.bfloat16, torch.float8_e4m3fn
    combos = (("bf16", bf16, bf16), ("fp8", fp8, fp8), ("bf16->fp8", bf16, fp8))
    lines = [
        "| pool->payload | tokens | MB | export ms (min-max) | loop (a) ms | "
        "D2H floor (b) ms | export GB/s | vs (a) | vs (b) | "
        "import ms (min-max) | loop (a) ms | H2D floor (b) ms | import GB/s | "
        "vs (a) | vs (b) |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]

    def ms(t):
        return f"{t[0] * 1e3:.3f} ({t[1] * 1e3:.3f}-{t[2] * 1e3:.3f})"

    def ratio(a, b):
        return f"{a[0] / b[0]:.2f}x" if a is not None else "n/a"

    for tag, pool_dtype, out_dtype in combos:
        for tokens in args.tokens:
            nbytes, t = bench_row(
                tokens, pool_dtype, out_dtype, args.reps, args.loop_reps
            )
            el, il = t.get("export_loop"), t.get("import_loop")
            lines.append(
                f"| {tag} | {tokens} | {nbytes / 1e6:.1f} | {ms(t['export'])} | "
                + (f"{el[0] * 1e3:.3f}" if el else "n/a")
                + f" | {t['d2h_floor'][0] * 1e3:.3f} | "
                f"{nbytes / t['export'][0] / 1e9:.1f} | "
                f"{ratio(el, t['export'])} | "
                f"{t['export'][0] / t['d2h_floor'][0]:.2f}x floor | "
                f"{ms(t['import'])} | "
                + (f"{il[0] * 1e3:.3f}" if il else "n/a")
                + f" | {t['h2d_floor'][0] * 1e3:.3f} | "
                f"{nbytes / t['import'][0] / 1e9:.1f} | "
                f"{ratio(il, t['import'])} | "
                f"{t['import'][0] / t['h2d_floor'][0]:.2f}x floor |"
            )
            print(lines[-1], flush=True)
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
