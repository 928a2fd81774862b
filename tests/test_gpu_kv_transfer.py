"""KV export/import on the GPU: the HIP page kernels against their torch_ref
twins on the cases of tests/kv_transfer_cases.py, the converting gather
against the fp8 cache write, and the engine life cycle. Everything is
compared bit for bit."""

import pytest
import torch

from tests import kv_transfer_cases as kc

pytestmark = pytest.mark.gpu

CASES = kc.cases()


def _to_cuda(pool):
    return [(k.cuda(), v.cuda()) for k, v in pool]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_kernels_match_reference(case):
    from kserve_amd import ops
    from kserve_amd.ops import torch_ref

    src, dst = kc.build(case)
    ids, dst_ids = list(case.block_ids), list(case.dst_ids)
    want = torch_ref.kv_gather_pages(src, ids, case.num_tokens)
    want_dst = kc.clone_pool(dst)
    torch_ref.kv_scatter_pages(want_dst, dst_ids, want)

    g_src, g_dst = _to_cuda(src), _to_cuda(dst)
    got = ops.kv_gather_pages(g_src, ids, case.num_tokens)
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(kc.as_bytes(got), kc.as_bytes(want))
    assert kc.pools_equal(g_src, src)  # the source is only read
    ops.kv_scatter_pages(g_dst, dst_ids, got)
    # listed pages written whole, every other page bitwise unchanged
    assert kc.pools_equal(g_dst, want_dst)
    listed = set(dst_ids)
    keep = [b for b in range(case.pool_pages) if b not in listed]
    for (gk, gv), (k, v) in zip(g_dst, dst):
        assert torch.equal(kc.as_bytes(gk)[keep], kc.as_bytes(k)[keep])
        assert torch.equal(kc.as_bytes(gv)[keep], kc.as_bytes(v)[keep])


def test_scatter_accepts_the_payload_bytes():
    """The engine hands the scatter a flat uint8 buffer."""
    from kserve_amd import ops

    case = kc.small_cases()[4]
    src, dst = kc.build(case)
    g_src, g_dst = _to_cuda(src), _to_cuda(dst)
    buf = ops.kv_gather_pages(g_src, list(case.block_ids), case.num_tokens)
    ops.kv_scatter_pages(
        g_dst, list(case.dst_ids), buf.view(torch.uint8).reshape(-1).clone()
    )
    again = ops.kv_gather_pages(g_dst, list(case.dst_ids), case.num_tokens)
    assert torch.equal(kc.as_bytes(again), kc.as_bytes(buf))


def test_bad_ids_raise_before_any_launch():
    from kserve_amd import ops

    case = kc.small_cases()[4]
    src, dst = kc.build(case)
    g_src, g_dst = _to_cuda(src), _to_cuda(dst)
    buf = ops.kv_gather_pages(g_src, [7, 2], 32)
    for bad in ([7, case.pool_pages], [-1, 3], [5, 5]):
        with pytest.raises(ValueError):
            ops.kv_scatter_pages(g_dst, bad, buf)
    torch.cuda.synchronize()
    assert kc.pools_equal(g_dst, dst)
    for bad in ([case.pool_pages], [-1]):
        with pytest.raises(ValueError):
            ops.kv_gather_pages(g_src, bad, 16)
    with pytest.raises(ValueError):
        ops.kv_gather_pages(g_src, [3], 17)
    # fp8 -> bf16 is refused, as is an fp8 payload into a bf16 pool
    fp8 = _to_cuda(kc.random_pool(kc.GEOMETRIES[3], 12, 3))
    with pytest.raises(ValueError):
        ops.kv_gather_pages(fp8, [3], 16, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.kv_scatter_pages(g_dst, [3], ops.kv_gather_pages(fp8, [3], 16))
    torch.cuda.synchronize()
    assert kc.pools_equal(g_dst, dst)


def _fp8_edge_rows(T, H, D):
    """Finite bf16 rows covering +-0, values below the E4M3 normal range
    (min normal 2^-6, min subnormal 2^-9), values above 448, negatives and
    ordinary values."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(T, H, D, generator=g) * 3.0
    special = torch.tensor(
        [0.0, -0.0, 2.0 ** -6, 2.0 ** -7, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9,
         2.0 ** -12, 1e-20, -1e-20, 447.0, 448.0, 449.0, 464.0, 480.0, 500.0,
         1e4, 3e38, -448.0, -464.0, -1e4, -3e38, 0.0625, -0.3, 1.0, -1.0,
         17.0, 0.1, 208.0, 240.0, 0.0175, -0.0019]
    )
    flat = x.reshape(-1)
    flat[: special.numel()] = special
    # the same specials in the odd lanes of a conversion pair
    flat[special.numel() + 1 : 2 * special.numel() + 1] = special
    sub = torch.randn(T, generator=g) * 2.0 ** -8  # E4M3 subnormal range
    x[:, 0, 3] = sub
    x[:, H - 1, D - 1] = torch.randn(T, generator=g) * 300.0
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("D", [128, 64])
def test_converting_gather_equals_fp8_cache_write(D):
    from kserve_amd import ops

    T, H, bs, pages = 45, 2, 16, 12
    k = _fp8_edge_rows(T, H, D).cuda()
    v = _fp8_edge_rows(T, H, D).flip(0).contiguous().cuda()
    assert torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all()
    ids = [9, 2, 6]
    pos = torch.arange(T)
    slots = (torch.tensor(ids)[pos // bs] * bs + pos % bs).to(torch.int32).cuda()
    pools = {}
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        layers = []
        for layer in range(2):
            kc_, vc_ = (
                torch.zeros(pages, H, bs, D, dtype=dt, device="cuda")
                for _ in range(2)
            )
            # layer 1 stores V as K and K as V: layers and tensors differ
            a, b = (k, v) if layer == 0 else (v, k)
            ops.reshape_and_cache(a, b, kc_, vc_, slots)
            layers.append((kc_, vc_))
        pools[dt] = layers
    for nt in (T, 33, 32):
        conv = ops.kv_gather_pages(
            pools[torch.bfloat16], ids, nt, out_dtype=torch.float8_e4m3fn
        )
        plain = ops.kv_gather_pages(pools[torch.float8_e4m3fn], ids, nt)
        assert conv.dtype == torch.float8_e4m3fn and conv.shape == plain.shape
        assert torch.equal(kc.as_bytes(conv), kc.as_bytes(plain))
    assert kc.as_bytes(plain)[:, :, :2].any()


# -- engine ----------------------------------------------------------------

PROMPTS = [
    [5],
    [(i * 7) % 2000 + 1 for i in range(16)],
    [(i * 3) % 2000 + 1 for i in range(17)],
    [(i * 11) % 2000 + 1 for i in range(33)],
]


def _engine(**cache):
    from kserve_amd.engine.config import (
        CacheConfig,
        EngineConfig,
        ModelConfig,
        SchedulerConfig,
    )
    from kserve_amd.engine.engine import LLMEngine

    return LLMEngine(
        EngineConfig(
            model=ModelConfig(
                vocab_size=2048,
                hidden_size=512,
                intermediate_size=1024,
                num_layers=4,
                num_heads=4,
                num_kv_heads=2,
                head_dim=128,
                max_position_embeddings=1024,
                model_name="gpu-tiny",
            ),
            cache=CacheConfig(block_size=16, num_gpu_blocks=128, **cache),
            scheduler=SchedulerConfig(
                max_num_seqs=8, max_num_batched_tokens=2048,
                max_model_len=512, multi_step=8,
            ),
            device="cuda",
            seed=0,
            eos_token_id=-1,
        )
    )


def _greedy():
    from kserve_amd.engine.sampling_params import SamplingParams

    return SamplingParams(temperature=0.0, max_tokens=12)


def _count_prefills(engine):
    calls = []
    orig = engine.runner.execute_prefill

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    engine.runner.execute_prefill = counted
    return calls


def _export_all(engine):
    from kserve_amd.engine.kv_transfer import KVPayload

    free0 = engine.scheduler.block_manager.num_free_blocks
    ids = [engine.add_request(p, _greedy(), kv_export=True) for p in PROMPTS]
    outs = {o.request_id: o for o in engine.step()}
    assert not engine.has_unfinished()
    assert engine.scheduler.block_manager.num_free_blocks == free0
    payloads = []
    for i in ids:
        assert outs[i].finish_reason == "kv_export"
        assert outs[i].kv_payload.data.is_pinned()
        payloads.append(KVPayload.from_bytes(outs[i].kv_payload.to_bytes()))
    return payloads


def _pages_of(engine, rid, num_tokens):
    from kserve_amd import ops

    req = next(r for r in engine.scheduler.running if r.request_id == rid)
    bm = engine.scheduler.block_manager
    table = bm.get_block_table(req)[: bm.blocks_needed(num_tokens)]
    return kc.as_bytes(
        ops.kv_gather_pages(engine.runner.kv_caches, table, num_tokens)
    ).reshape(-1)


def _import_and_run(engine, payloads):
    """Import all four before the first step; returns (ids, pages after the
    first step, first outputs, final outputs)."""
    prefills = _count_prefills(engine)
    ids = [
        engine.add_request(p, _greedy(), kv_import=x)
        for p, x in zip(PROMPTS, payloads)
    ]
    firsts, final = {}, {}
    pages = None
    while engine.has_unfinished():
        for o in engine.step():
            firsts.setdefault(o.request_id, o)
            if o.finished:
                final[o.request_id] = o
        if pages is None:
            pages = [
                _pages_of(engine, i, len(p)) for i, p in zip(ids, PROMPTS)
            ]
    assert not prefills
    return ids, pages, firsts, final


def test_engine_export_import_bf16():
    r = _engine()
    ref = [o.output_token_ids for o in r.generate(PROMPTS, _greedy()).values()]
    del r
    payloads = _export_all(_engine())
    assert [x.output_token_ids for x in payloads] == [t[:1] for t in ref]
    b = _engine()
    ids, pages, firsts, final = _import_and_run(b, payloads)
    assert [final[i].output_token_ids for i in ids] == ref
    for i, x, pg in zip(ids, payloads, pages):
        assert firsts[i].new_token_ids == x.output_token_ids
        assert torch.equal(pg, x.data)


def test_engine_bf16_export_feeds_fp8_pool():
    # an fp8 engine that prefills the same batch itself
    f = _engine(kv_cache_dtype="fp8")
    f_ids = [f.add_request(p, _greedy()) for p in PROMPTS]
    final_f = {}
    f_pages = None
    while f.has_unfinished():
        for o in f.step():
            if o.finished:
                final_f[o.request_id] = o
        if f_pages is None:  # right after the prefill step
            f_pages = [
                _pages_of(f, i, len(p)) for i, p in zip(f_ids, PROMPTS)
            ]
    del f
    a = _engine(kv_export_dtype="fp8")
    assert a.runner.kv_caches[0][0].dtype == torch.bfloat16
    payloads = _export_all(a)
    del a
    assert all(x.dtype == "fp8_e4m3" for x in payloads)
    b = _engine(kv_cache_dtype="fp8")
    ids, pages, _, final = _import_and_run(b, payloads)
    for pg, fp, x in zip(pages, f_pages, payloads):
        assert torch.equal(pg, x.data)
        assert torch.equal(pg, fp)
    assert [final[i].output_token_ids for i in ids] == [
        final_f[i].output_token_ids for i in f_ids
    ]
