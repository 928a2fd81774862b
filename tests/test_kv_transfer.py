"""KV export/import (prefill/decode disaggregation) on the CPU: the torch_ref
twins of the page ops against the loop oracle of tests/kv_transfer_cases.py,
mutants of the twins, the payload wire format, the engine life cycle on the
tiny model and the server roles. Everything is compared bit for bit."""

import asyncio
import dataclasses

import pytest
import torch

from kserve_amd import ops
from kserve_amd.engine.config import (
    CacheConfig,
    EngineConfig,
    ModelConfig,
    ParallelConfig,
    SchedulerConfig,
)
from kserve_amd.engine.engine import LLMEngine
from kserve_amd.engine.kv_transfer import FORMAT_VERSION, MAGIC, KVPayload
from kserve_amd.engine.sampling_params import SamplingParams
from kserve_amd.ops import torch_ref
from tests import kv_transfer_cases as kc

CASES = kc.cases()


# -- reference ops ---------------------------------------------------------


def _passes(case, gather, scatter) -> bool:
    """gather/scatter reproduce the loop oracle on this case."""
    src, dst = kc.build(case)
    src_before = kc.clone_pool(src)
    buf = gather(src, list(case.block_ids), case.num_tokens)
    want = kc.expected_gather(case, src)
    ok = tuple(buf.shape) == (
        case.geo.L, 2, len(case.block_ids), case.geo.Hkv, case.geo.bs,
        case.geo.D,
    ) and buf.dtype == case.geo.dtype
    ok = ok and torch.equal(kc.as_bytes(buf), want.view_as(kc.as_bytes(buf)))
    ok = ok and kc.pools_equal(src, src_before)
    scatter(dst, list(case.dst_ids), buf)
    want_dst = kc.expected_scatter(case, kc.build(case)[1], want)
    return ok and kc.pools_equal(dst, want_dst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_gather_scatter(case):
    assert _passes(case, torch_ref.kv_gather_pages, torch_ref.kv_scatter_pages)


@pytest.mark.parametrize("case", kc.small_cases(), ids=lambda c: c.name)
def test_roundtrip_zeroes_tail_and_spares_other_pages(case):
    src, dst = kc.build(case)
    before = kc.clone_pool(dst)
    buf = ops.kv_gather_pages(src, list(case.block_ids), case.num_tokens)
    ops.kv_scatter_pages(dst, list(case.dst_ids), buf)
    bs = case.geo.bs
    listed = set(case.dst_ids)
    for layer in range(case.geo.L):
        for kv in range(2):
            got = kc.as_bytes(dst[layer][kv])
            was = kc.as_bytes(before[layer][kv])
            orig = kc.as_bytes(src[layer][kv])
            for b in range(case.pool_pages):
                if b not in listed:
                    assert torch.equal(got[b], was[b])
            for j, (s, d) in enumerate(zip(case.block_ids, case.dst_ids)):
                valid = min(max(case.num_tokens - j * bs, 0), bs)
                assert torch.equal(got[d][:, :valid], orig[s][:, :valid])
                assert not got[d][:, valid:].any()
                # every source byte is non-zero: nothing copied looks zeroed
                assert got[d][:, :valid].all()


def _mutants():
    g, s = torch_ref.kv_gather_pages, torch_ref.kv_scatter_pages
    return {
        "zero_bound_plus_one": (lambda kv, ids, nt: g(kv, ids, nt + 1), s),
        "zero_bound_minus_one": (lambda kv, ids, nt: g(kv, ids, nt - 1), s),
        "identity_page_order": (
            lambda kv, ids, nt: g(kv, list(range(len(ids))), nt), s,
        ),
        "k_v_swapped": (
            lambda kv, ids, nt: g([(v, k) for k, v in kv], ids, nt), s,
        ),
        "layers_reversed": (lambda kv, ids, nt: g(kv[::-1], ids, nt), s),
        "scatter_page_plus_one": (
            g,
            lambda kv, ids, buf: s(
                kv, [(b + 1) % kv[0][0].shape[0] for b in ids], buf
            ),
        ),
    }


@pytest.mark.parametrize("name", sorted(_mutants()))
def test_every_mutant_is_killed(name):
    gather, scatter = _mutants()[name]
    killed = [c.name for c in kc.small_cases() if not _passes(c, gather, scatter)]
    assert killed, f"mutant {name} passes every case"


def test_ops_validate_ids_before_touching_anything():
    case = kc.small_cases()[0]
    src, dst = kc.build(case)
    before = kc.clone_pool(dst)
    buf = ops.kv_gather_pages(src, [7, 2], 32)
    for bad in ([7, 12], [-1, 3], [5, 5]):
        with pytest.raises(ValueError):
            ops.kv_scatter_pages(dst, bad, buf)
    assert kc.pools_equal(dst, before)
    for bad in ([12], [-1]):
        with pytest.raises(ValueError):
            ops.kv_gather_pages(src, bad, 16)
    with pytest.raises(ValueError):
        ops.kv_gather_pages(src, [3], 17)  # more tokens than pages
    fp8 = kc.random_pool(kc.GEOMETRIES[3], 12, 3)
    with pytest.raises(ValueError, match="bf16 -> fp8"):
        ops.kv_gather_pages(fp8, [3], 16, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):  # fp8 payload into a bf16 pool
        ops.kv_scatter_pages(
            dst, [3], ops.kv_gather_pages(fp8, [3], 16)
        )


def test_converting_gather_matches_fp8_cache_write_on_cpu():
    """The torch_ref converting gather is the cast torch_ref.reshape_and_cache
    applies when the pool is fp8."""
    torch.manual_seed(3)
    T, H, D, bs = 40, 2, 128, 16
    k = (torch.randn(T, H, D) * 4).to(torch.bfloat16)
    v = (torch.randn(T, H, D) * 4).to(torch.bfloat16)
    slots = torch.arange(T, dtype=torch.int32) + 2 * bs
    pools = {}
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        kc_, vc_ = (torch.zeros(8, H, bs, D, dtype=dt) for _ in range(2))
        torch_ref.reshape_and_cache(k, v, kc_, vc_, slots)
        pools[dt] = [(kc_, vc_)]
    ids = [2, 3, 4]
    conv = ops.kv_gather_pages(
        pools[torch.bfloat16], ids, T, out_dtype=torch.float8_e4m3fn
    )
    plain = ops.kv_gather_pages(pools[torch.float8_e4m3fn], ids, T)
    assert conv.dtype == torch.float8_e4m3fn
    assert torch.equal(kc.as_bytes(conv), kc.as_bytes(plain))


# -- payload ---------------------------------------------------------------


def _payload(num_tokens=17, dtype="bfloat16", **kw) -> KVPayload:
    L, H, D, bs = 2, 2, 16, 16
    pages = -(-num_tokens // bs)
    item = 1 if dtype == "fp8_e4m3" else 2
    g = torch.Generator().manual_seed(5)
    fields = dict(
        num_layers=L, num_kv_heads=H, head_dim=D, block_size=bs, dtype=dtype,
        model_name="tiny-llama", quantization=None,
        prompt_token_ids=list(range(1, num_tokens + 1)),
        output_token_ids=[42], num_tokens=num_tokens,
        data=torch.randint(
            0, 256, (L * 2 * pages * H * bs * D * item,), generator=g,
            dtype=torch.uint8,
        ),
        first_logprobs={42: -0.25, 7: -1.5},
    )
    fields.update(kw)
    return KVPayload(**fields)


def _reheader(blob: bytes, **changes) -> bytes:
    """The same payload bytes with header fields replaced."""
    import json
    import struct

    fixed = len(MAGIC) + 4
    (hlen,) = struct.unpack("<I", blob[len(MAGIC):fixed])
    h = json.loads(blob[fixed:fixed + hlen])
    h.update(changes)
    header = json.dumps(h).encode()
    return MAGIC + struct.pack("<I", len(header)) + header + blob[fixed + hlen:]


def test_payload_roundtrip():
    p = _payload()
    q = KVPayload.from_bytes(p.to_bytes())
    for f in dataclasses.fields(KVPayload):
        if f.name != "data":
            assert getattr(q, f.name) == getattr(p, f.name), f.name
    assert torch.equal(q.data, p.data)
    assert q.first_logprobs == {42: -0.25, 7: -1.5}
    assert b"pickle" not in p.to_bytes()[:64] and p.to_bytes().startswith(MAGIC)


def test_payload_refusals():
    blob = _payload().to_bytes()
    bad = {
        "unknown version": _reheader(blob, version=FORMAT_VERSION + 1),
        "truncated body": blob[:-1],
        "over-long body": blob + b"\x00",
        "truncated header": blob[:20],
        "bad magic": b"X" + blob[1:],
        # data length other than the geometry implies
        "data vs geometry": _reheader(blob, num_layers=3),
        # num_tokens inconsistent with the page count
        "tokens vs pages": _reheader(
            blob, num_tokens=16, prompt_token_ids=list(range(16))
        ),
        "tokens vs prompt": _reheader(blob, num_tokens=18),
    }
    for what, b in bad.items():
        with pytest.raises(ValueError):
            KVPayload.from_bytes(b)
            pytest.fail(f"{what} accepted")
    # consistent header, short data: geometry check, not only the length field
    short = _payload()
    short.data = short.data[:-32]
    with pytest.raises(ValueError, match="imply"):
        KVPayload.from_bytes(short.to_bytes())


def _engine_cfg(**cache) -> EngineConfig:
    cache.setdefault("block_size", 16)
    cache.setdefault("num_gpu_blocks", 64)
    return EngineConfig(
        model=ModelConfig.tiny(vocab_size=128),
        cache=CacheConfig(**cache),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=256, max_model_len=128,
            multi_step=8,
        ),
        device="cpu",
        eos_token_id=-1,
    )


@pytest.mark.parametrize(
    "field,change",
    [
        ("num_layers", dict(num_layers=3)),
        ("num_kv_heads", dict(num_kv_heads=1)),
        ("head_dim", dict(head_dim=32)),
        ("block_size", dict(block_size=8)),
        ("dtype", dict(dtype="fp8_e4m3")),  # fp8 payload, bf16 engine
        ("model_name", dict(model_name="other")),
        ("quantization", dict(quantization="fp8")),
    ],
)
def test_check_compatible_names_the_field(field, change):
    cfg = _engine_cfg()
    _payload().check_compatible(cfg)
    p = dataclasses.replace(_payload(), **change)
    with pytest.raises(ValueError, match=field):
        p.check_compatible(cfg)


def test_fp8_payload_fits_fp8_engine_only():
    p = _payload(dtype="fp8_e4m3")
    p.check_compatible(_engine_cfg(kv_cache_dtype="fp8"))
    with pytest.raises(ValueError, match="dtype"):
        p.check_compatible(_engine_cfg())


# -- engine ----------------------------------------------------------------

PROMPTS = [
    [5],
    [(i * 7) % 100 + 1 for i in range(16)],
    [(i * 3) % 100 + 1 for i in range(17)],
    [(i * 11) % 100 + 1 for i in range(33)],
]
GREEDY = SamplingParams(temperature=0.0, max_tokens=12)


def _engine(**cache) -> LLMEngine:
    torch.manual_seed(0)
    return LLMEngine(_engine_cfg(**cache))


def _count_prefills(engine):
    calls = []
    orig = engine.runner.execute_prefill

    def counted(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    engine.runner.execute_prefill = counted
    return calls


def _export_all(engine, prompts, sp=GREEDY):
    ids = [engine.add_request(p, sp, kv_export=True) for p in prompts]
    outs = {o.request_id: o for o in engine.step()}
    return [outs[i] for i in ids]


def _drain(engine):
    firsts, final = {}, {}
    while engine.has_unfinished():
        for o in engine.step():
            firsts.setdefault(o.request_id, o)
            if o.finished:
                final[o.request_id] = o
    return firsts, final


@pytest.fixture(scope="module")
def reference_tokens():
    out = _engine().generate(PROMPTS, GREEDY)
    return [o.output_token_ids for o in out.values()]


@pytest.fixture(scope="module")
def exported():
    """Engine A's four payloads, through the wire format."""
    a = _engine()
    free0 = a.scheduler.block_manager.num_free_blocks
    outs = _export_all(a, PROMPTS)
    assert not a.has_unfinished()
    # nothing is held after the export step
    assert a.scheduler.block_manager.num_free_blocks == free0
    for o, p in zip(outs, PROMPTS):
        assert o.finished and o.finish_reason == "kv_export"
        assert len(o.new_token_ids) == 1
        assert o.kv_payload.num_tokens == len(p)
    return [KVPayload.from_bytes(o.kv_payload.to_bytes()) for o in outs]


def test_import_continues_without_prefill(reference_tokens, exported):
    b = _engine()
    prefills = _count_prefills(b)
    ids = [
        b.add_request(p, GREEDY, kv_import=x) for p, x in zip(PROMPTS, exported)
    ]
    firsts, final = _drain(b)
    assert [final[i].output_token_ids for i in ids] == reference_tokens
    assert not prefills
    for i, x in zip(ids, exported):
        assert firsts[i].new_token_ids == x.output_token_ids
    assert all(final[i].finish_reason == "length" for i in ids)
    assert all(final[i].kv_payload is None for i in ids)


def test_export_carries_first_token_of_reference(reference_tokens, exported):
    assert [x.output_token_ids for x in exported] == [
        t[:1] for t in reference_tokens
    ]


def test_import_max_tokens_one_finishes_at_once(exported):
    b = _engine()
    free0 = b.scheduler.block_manager.num_free_blocks
    sp = SamplingParams(temperature=0.0, max_tokens=1)
    rid = b.add_request(PROMPTS[2], sp, kv_import=exported[2])
    outs = b.step()
    assert [o.request_id for o in outs] == [rid]
    assert outs[0].finished and outs[0].finish_reason == "length"
    assert outs[0].output_token_ids == exported[2].output_token_ids
    assert not b.has_unfinished()
    assert b.scheduler.block_manager.num_free_blocks == free0


def test_imported_request_survives_recompute_preemption(
    reference_tokens, exported
):
    b = _engine()
    prefills = _count_prefills(b)
    ids = [
        b.add_request(p, GREEDY, kv_import=x) for p, x in zip(PROMPTS, exported)
    ]
    final = {}
    for o in b.step():  # import + first decode window
        if o.finished:
            final[o.request_id] = o
    victim = next(r for r in b.scheduler.running if r.request_id == ids[3])
    b.scheduler.running.remove(victim)
    b.scheduler._preempt(victim)
    final.update(_drain(b)[1])
    assert prefills  # the preempted request was recomputed by prefill
    assert [final[i].output_token_ids for i in ids] == reference_tokens


def test_import_waits_for_a_seat(exported, reference_tokens):
    """max_num_seqs bounds imported requests like any other."""
    torch.manual_seed(0)
    cfg = _engine_cfg()
    cfg.scheduler.max_num_seqs = 2
    b = LLMEngine(cfg)
    ids = [
        b.add_request(p, GREEDY, kv_import=x) for p, x in zip(PROMPTS, exported)
    ]
    b.step()
    assert len(b.scheduler.running) == 2 and len(b.scheduler.waiting) == 2
    _, final = _drain(b)
    assert sorted(final) == sorted(ids)
    assert all(len(final[i].output_token_ids) == 12 for i in ids)


def test_export_with_prefix_cache_keeps_refcounts():
    a = _engine(enable_prefix_caching=True)
    bm = a.scheduler.block_manager
    free0 = bm.num_free_blocks
    shared = [(i * 5) % 90 + 1 for i in range(32)]
    first = _export_all(a, [shared + [3, 4, 5]])
    second = _export_all(a, [shared + [9, 8]])  # hits the 32-token prefix
    assert bm.cache_hit_tokens == 32
    assert not a.has_unfinished()
    assert not bm._refcount and not bm._tables
    assert bm.num_free_blocks == free0
    # the shared pages travel identically in both payloads
    d1 = first[0].kv_payload.data.view(2, 2, 3, -1)
    d2 = second[0].kv_payload.data.view(2, 2, 3, -1)
    assert torch.equal(d1[:, :, :2], d2[:, :, :2])
    # and the cache-hit export matches a cold engine's
    cold = _export_all(_engine(), [shared + [9, 8]])
    assert torch.equal(cold[0].kv_payload.data, second[0].kv_payload.data)
    assert cold[0].new_token_ids == second[0].new_token_ids


def test_export_with_chunked_prefill(exported):
    torch.manual_seed(0)
    cfg = _engine_cfg()
    cfg.scheduler.enable_chunked_prefill = True
    cfg.scheduler.max_num_batched_tokens = 16
    a = LLMEngine(cfg)
    rid = a.add_request(PROMPTS[3], GREEDY, kv_export=True)
    _, final = _drain(a)
    assert final[rid].finish_reason == "kv_export"
    assert final[rid].kv_payload.num_tokens == 33
    assert final[rid].new_token_ids == exported[3].output_token_ids


def test_refusals(exported):
    b = _engine()
    with pytest.raises(ValueError, match="LoRA"):
        b.add_request(
            PROMPTS[1], SamplingParams(lora_name="x"), kv_export=True
        )
    with pytest.raises(ValueError, match="guided"):
        b.add_request(
            PROMPTS[1], SamplingParams(response_format="json_object"),
            kv_import=exported[1],
        )
    with pytest.raises(ValueError, match="guided"):
        b.add_request(
            PROMPTS[1], SamplingParams(guided_choice=["a", "b"]),
            kv_export=True,
        )
    with pytest.raises(ValueError, match="different prompt"):
        b.add_request(PROMPTS[2], GREEDY, kv_import=exported[1])
    with pytest.raises(ValueError, match="dtype"):
        _engine(kv_cache_dtype="fp8").add_request(
            PROMPTS[1], GREEDY, kv_import=exported[1]
        )
    # a payload the pool could never hold would wait forever: 33 tokens + 1
    # need 3 blocks, a 4-block pool gives a request 2 (block 0, watermark)
    with pytest.raises(ValueError, match="blocks"):
        _engine(num_gpu_blocks=4).add_request(
            PROMPTS[3], GREEDY, kv_import=exported[3]
        )
    # the draft model of draft-model speculation never saw the prompt
    b.draft = object()
    with pytest.raises(ValueError, match="draft"):
        b.add_request(PROMPTS[1], GREEDY, kv_import=exported[1])
    b.draft = None
    b.config.parallel = ParallelConfig(tensor_parallel_size=2)
    with pytest.raises(ValueError, match="parallel"):
        b.add_request(PROMPTS[1], GREEDY, kv_export=True)
    with pytest.raises(ValueError, match="parallel"):
        b.add_request(PROMPTS[1], GREEDY, kv_import=exported[1])
    assert not b.has_unfinished()


# -- server ----------------------------------------------------------------


def test_role_arguments_parse():
    from kserve_amd.controlplane.llmisvc_config import PRESETS
    from kserve_amd.runtimes.huggingfaceserver import build_parser

    p = build_parser()
    assert p.parse_args([]).role == "both"
    assert p.parse_args(["--role=prefill"]).role == "prefill"
    a = p.parse_args(["--role=decode", "--prefill-endpoint=http://pre:8080"])
    assert (a.role, a.prefill_endpoint) == ("decode", "http://pre:8080")
    with pytest.raises(SystemExit):
        p.parse_args(["--role=nonsense"])
    preset = PRESETS["kserve-config-llm-prefill-template"]["prefill"]["args"]
    assert "--role=prefill" in preset
    rendered = [
        "--model_dir=/mnt/models", "--model_name=m", "--backend=engine",
        "--tensor-parallel-size=1", "--max_model_len=8192",
        "--max_num_seqs=256",
    ]
    assert p.parse_args(rendered + preset).role == "prefill"


def test_rendered_prefill_workload_arguments_parse():
    from kserve_amd.controlplane import llmisvc
    from kserve_amd.controlplane.llmisvc_config import PRESETS
    from kserve_amd.runtimes.huggingfaceserver import build_parser

    spec = llmisvc.LLMInferenceServiceSpec(
        model=llmisvc.LLMModelSpec(uri="hf://x", name="m"),
        workload=llmisvc.WorkloadSpec(),
        prefill=llmisvc.WorkloadSpec(),
    )
    manifest = llmisvc.render_workload(
        llmisvc.LLMInferenceService("llama", spec=spec), "prefill"
    )
    args = manifest["spec"]["template"]["spec"]["containers"][0]["args"]
    args = args + PRESETS["kserve-config-llm-prefill-template"]["prefill"]["args"]
    assert build_parser().parse_args(args).role == "prefill"


def test_main_mounts_the_prefill_route(monkeypatch):
    """main() with the preset's arguments builds a server whose app has
    the KV route; with the default role it has not."""
    from kserve_amd.controlplane.llmisvc_config import PRESETS
    from kserve_amd.model_server import ModelServer
    from kserve_amd.runtimes import huggingfaceserver as hfs
    from kserve_amd.runtimes.llm_model import LLMModel

    from kserve_amd import model_server

    started = []
    # main() and ModelServer configure process-wide logging; leave the test
    # session's loggers as they are
    monkeypatch.setattr(hfs, "configure_logging", lambda *a, **k: None)
    monkeypatch.setattr(model_server, "configure_logging", lambda *a, **k: None)
    monkeypatch.setattr(
        hfs, "build_model",
        lambda args: LLMModel(
            args.model_name, _engine_cfg(), role=args.role,
            prefill_endpoint=args.prefill_endpoint,
        ),
    )
    monkeypatch.setattr(
        ModelServer, "start", lambda self, models: started.append((self, models))
    )
    base = ["--model_name=m", "--backend=engine"]
    hfs.main(base + PRESETS["kserve-config-llm-prefill-template"]["prefill"]["args"])
    hfs.main(base)
    hfs.main(base + ["--role=decode", "--prefill-endpoint=http://pre:8080"])

    def has_route(server):
        return any(
            getattr(r, "path", None) == "/v1/kv/prefill"
            and "POST" in getattr(r, "methods", ())
            for r in server.app.routes
        )

    assert [has_route(srv) for srv, _ in started] == [True, False, False]
    assert [m[0].role for _, m in started] == ["prefill", "both", "decode"]
    assert started[2][1][0].prefill_endpoint == "http://pre:8080"


@pytest.mark.parametrize(
    "error", [RuntimeError("stream broke"), KeyError("header"), OSError("down")]
)
def test_any_peer_failure_falls_back(error):
    """Whatever the peer path raises, the request is prefilled locally."""
    from kserve_amd.runtimes.llm_model import LLMModel

    class Client:
        async def post(self, *a, **k):
            raise error

    model = LLMModel(
        "m", _engine_cfg(), role="decode", prefill_endpoint="http://pre",
        http_client=Client(),
    )
    before = _fallbacks()
    got = asyncio.new_event_loop().run_until_complete(
        model._remote_prefill([1, 2, 3], GREEDY)
    )
    assert got is None
    assert _fallbacks() == before + 1


def _app(name, role="both", prefill_endpoint=None, http_client=None):
    from kserve_amd.model_repository import ModelRepository
    from kserve_amd.protocol.dataplane import DataPlane
    from kserve_amd.protocol.rest.openai.endpoints import (
        register_openai_endpoints,
    )
    from kserve_amd.protocol.rest.server import create_app
    from kserve_amd.runtimes.llm_model import (
        LLMModel,
        register_kv_prefill_route,
    )

    torch.manual_seed(0)
    cfg = _engine_cfg(block_size=4, num_gpu_blocks=128)
    model = LLMModel(
        name, cfg, role=role, prefill_endpoint=prefill_endpoint,
        http_client=http_client,
    )
    repo = ModelRepository()
    repo.update(model)
    dp = DataPlane(repo)
    app = create_app(dp)
    register_openai_endpoints(app, dp, [model])
    if role == "prefill":
        register_kv_prefill_route(app, model)
    return app, model


def _fallbacks() -> float:
    from kserve_amd.metrics import KV_TRANSFER_FALLBACK

    return KV_TRANSFER_FALLBACK._value.get()


REQ = {"model": "m", "prompt": [3, 1, 4, 1, 5, 9, 2, 6, 5], "max_tokens": 6,
       "temperature": 0.0}


@pytest.fixture(scope="module")
def servers():
    """A `both` app, a prefill app, and decode apps pointed at the prefill
    app, at a peer that errors and at one that truncates the payload."""
    import httpx
    from fastapi import FastAPI
    from fastapi.responses import Response
    from fastapi.testclient import TestClient

    both_app, both = _app("m")
    pre_app, pre = _app("m", role="prefill")

    def client_for(app):
        return httpx.AsyncClient(
            transport=httpx.ASGITransport(app=app), base_url="http://pre"
        )

    broken = FastAPI()

    @broken.post("/v1/kv/prefill")
    async def _err():
        return Response(status_code=503)

    truncating = FastAPI()

    @truncating.post("/v1/kv/prefill")
    async def _cut():
        blob = await pre.kv_prefill(
            {"prompt_token_ids": REQ["prompt"],
             "sampling": {"temperature": 0.0}}
        )
        return Response(content=blob[:-7],
                        media_type="application/octet-stream")

    built = {"both": (both_app, both), "prefill": (pre_app, pre)}
    for key, peer in (("decode", pre_app), ("decode_503", broken),
                      ("decode_cut", truncating)):
        built[key] = _app(
            "m", role="decode", prefill_endpoint="http://pre",
            http_client=client_for(peer),
        )
    clients = {}
    stack = []
    for key, (app, model) in built.items():
        c = TestClient(app)
        c.__enter__()
        stack.append(c)
        asyncio.new_event_loop().run_until_complete(model.start_engine())
        clients[key] = (c, model)
    yield clients
    for c in stack:
        c.__exit__(None, None, None)
    for _, model in clients.values():
        model.stop()


def _complete(servers, key):
    c, model = servers[key]
    r = c.post("/openai/v1/completions", json=REQ)
    assert r.status_code == 200, r.text
    return r.json()["choices"][0]


def test_prefill_route_returns_a_payload(servers):
    c, _ = servers["prefill"]
    r = c.post(
        "/v1/kv/prefill",
        json={"prompt_token_ids": REQ["prompt"],
              "sampling": {"temperature": 0.0}},
    )
    assert r.status_code == 200, r.text
    assert r.headers["content-type"] == "application/octet-stream"
    p = KVPayload.from_bytes(r.content)
    assert p.prompt_token_ids == REQ["prompt"] and len(p.output_token_ids) == 1
    assert c.post("/v1/kv/prefill", json={"prompt_token_ids": []}).status_code == 400
    # only prefill-role servers have the route
    assert servers["both"][0].post(
        "/v1/kv/prefill", json={"prompt_token_ids": [1]}
    ).status_code in (404, 405)


def test_decode_server_imports_from_prefill_server(servers):
    want = _complete(servers, "both")
    _, decode_model = servers["decode"]
    prefills = _count_prefills(decode_model.async_engine.engine)
    before = _fallbacks()
    got = _complete(servers, "decode")
    assert got["text"] == want["text"]
    assert got["finish_reason"] == want["finish_reason"] == "length"
    assert not prefills
    assert _fallbacks() == before


@pytest.mark.parametrize("key", ["decode_503", "decode_cut"])
def test_decode_server_falls_back_to_local_prefill(servers, key):
    want = _complete(servers, "both")
    _, model = servers[key]
    prefills = _count_prefills(model.async_engine.engine)
    before = _fallbacks()
    got = _complete(servers, key)
    assert got["text"] == want["text"]
    assert len(prefills) == 1
    assert _fallbacks() == before + 1


def test_transfer_counters_are_exported(servers):
    c, _ = servers["both"]
    body = c.get("/metrics").content
    for name in (b"kv_transfer_fallback_total",
                 b"kv_transfer_exported_requests_total",
                 b"kv_transfer_exported_bytes_total",
                 b"kv_transfer_imported_requests_total",
                 b"kv_transfer_imported_bytes_total"):
        assert name in body
