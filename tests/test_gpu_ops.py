"""GPU numerics: each CDNA4 HIP kernel vs the plain-PyTorch fp32 reference.

All tests are @pytest.mark.gpu and run on a real MI355X via gpurun.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from kserve_amd.ops import torch_ref


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    torch.manual_seed(0)
    return torch.device("cuda:0")


def bf16_close(got, ref_f32, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(
        got.float().cpu(), ref_f32.float().cpu(), atol=atol, rtol=rtol
    )


class TestMfmaProbe:
    def test_mfma_probe(self, dev):
        """Verifies the A/B fragment layout assumptions in mfma_layouts.h."""
        import kserve_amd_C

        a = torch.randn(16, 32, dtype=torch.bfloat16, device=dev)
        b = torch.randn(32, 16, dtype=torch.bfloat16, device=dev)
        c = torch.zeros(16, 16, dtype=torch.float32, device=dev)
        kserve_amd_C.mfma_probe(c, a.view(torch.int16), b.view(torch.int16))
        torch.cuda.synchronize()
        ref = a.float() @ b.float()
        torch.testing.assert_close(c.cpu(), ref.cpu(), atol=1e-2, rtol=1e-2)


class TestRMSNorm:
    @pytest.mark.parametrize("rows,hidden", [(1, 4096), (64, 4096), (333, 8192), (7, 64)])
    def test_rms_norm(self, dev, rows, hidden):
        from kserve_amd import ops

        x = torch.randn(rows, hidden, dtype=torch.bfloat16, device=dev)
        w = torch.randn(hidden, dtype=torch.bfloat16, device=dev)
        got = ops.rms_norm(x, w, 1e-5)
        ref = torch_ref.rms_norm(x.float().cpu(), w.float().cpu(), 1e-5)
        bf16_close(got, ref)

    def test_fused_add_rms_norm(self, dev):
        from kserve_amd import ops

        rows, hidden = 96, 4096
        x = torch.randn(rows, hidden, dtype=torch.bfloat16, device=dev)
        res = torch.randn(rows, hidden, dtype=torch.bfloat16, device=dev)
        w = torch.randn(hidden, dtype=torch.bfloat16, device=dev)
        x_ref, res_ref = torch_ref.fused_add_rms_norm(
            x.float().cpu(), res.float().cpu(), w.float().cpu(), 1e-5
        )
        got_x, got_res = ops.fused_add_rms_norm(x, res, w, 1e-5)
        bf16_close(got_res, res_ref)
        bf16_close(got_x, x_ref)


class TestActivation:
    @pytest.mark.parametrize("rows,d", [(16, 14336), (257, 128)])
    def test_silu_and_mul(self, dev, rows, d):
        from kserve_amd import ops

        x = torch.randn(rows, 2 * d, dtype=torch.bfloat16, device=dev)
        got = ops.silu_and_mul(x)
        ref = torch_ref.silu_and_mul(x.float().cpu())
        bf16_close(got, ref)


class TestRope:
    def test_rotary_embedding(self, dev):
        from kserve_amd import ops

        T, Hq, Hk, D = 77, 8, 2, 128
        cache = torch_ref.make_cos_sin_cache(D, 512, 500000.0).to(dev)
        q = torch.randn(T, Hq, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(T, Hk, D, dtype=torch.bfloat16, device=dev)
        pos = torch.randint(0, 512, (T,), device=dev)
        q_ref, k_ref = torch_ref.rotary_embedding(
            pos.cpu(), q.float().cpu(), k.float().cpu(), cache.cpu()
        )
        got_q, got_k = ops.rotary_embedding(pos, q, k, cache)
        bf16_close(got_q, q_ref)
        bf16_close(got_k, k_ref)


class TestKVCache:
    def test_reshape_and_cache(self, dev):
        from kserve_amd import ops

        T, Hkv, D, bs, B = 50, 8, 128, 16, 32
        k = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        slots = torch.randperm(B * bs, device=dev)[:T].to(torch.int32)
        kc_ref = torch.zeros(B, Hkv, bs, D).float()
        vc_ref = torch.zeros_like(kc_ref)
        torch_ref.reshape_and_cache(
            k.float().cpu(), v.float().cpu(), kc_ref, vc_ref, slots.cpu()
        )
        ops.reshape_and_cache(k, v, kc, vc, slots)
        bf16_close(kc, kc_ref)
        bf16_close(vc, vc_ref)


class TestDecodeAttention:
    @pytest.mark.parametrize(
        "S,H,Hkv,ctx_max",
        [
            (4, 32, 8, 100),    # llama-8b shape, small batch (split-context)
            (64, 32, 8, 500),   # moderate batch
            (2, 8, 2, 17),      # ragged boundary
            (8, 4, 4, 64),      # group=1 (MHA)
            (4, 8, 1, 100),     # group=8 (llama-70b TP=8 shape)
            (16, 64, 8, 200),   # full 70b head config
        ],
    )
    def test_paged_decode(self, dev, S, H, Hkv, ctx_max):
        from kserve_amd import ops

        D, bs = 128, 16
        torch.manual_seed(S)
        ctx = torch.randint(1, ctx_max + 1, (S,), dtype=torch.int32)
        max_blocks = int((int(ctx.max()) + bs - 1) // bs)
        B = S * max_blocks + 1
        kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        # disjoint block tables
        bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
            S, max_blocks
        )
        q = torch.randn(S, H, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.paged_attention_decode(
            q, kc, vc, bt.to(dev), ctx.to(dev), scale
        )
        ref = torch_ref.paged_attention_decode(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, ctx, scale
        )
        bf16_close(got, ref)


class TestPrefillAttention:
    @pytest.mark.parametrize(
        "lens,H,Hkv",
        [
            ([128], 32, 8),
            ([64, 200, 13], 32, 8),
            ([1, 511], 8, 8),
            ([65], 16, 4),
        ],
    )
    def test_flash_prefill(self, dev, lens, H, Hkv):
        from kserve_amd import ops

        D = 128
        torch.manual_seed(sum(lens))
        total = sum(lens)
        cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
        q = torch.randn(total, H, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(total, Hkv, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(total, Hkv, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.flash_prefill_varlen(q, k, v, cu.to(dev), max(lens), scale)
        ref = torch_ref.flash_prefill_varlen(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu, scale
        )
        bf16_close(got, ref, atol=3e-2, rtol=3e-2)

    def test_full_gpu_grid_repeatable_and_accurate(self, dev):
        """One prefill wave of the serving benchmark's shape (32 prompts x
        512 tokens, 32/8 heads: 4096 workgroups, many per CU in turn). The
        kernel was once exact on small grids but changed ~0.25% of its
        outputs from call to call at this size (see mul_f32_unpacked in
        attention_prefill.hip), so check here that identical inputs give
        identical bits and that they match fp32."""
        from kserve_amd import ops

        S, L, H, Hkv, D = 32, 512, 32, 8, 128
        torch.manual_seed(7)
        # q/k/v as the model passes them: strided views of one qkv buffer
        qkv = torch.randn(S * L, (H + 2 * Hkv) * D, dtype=torch.bfloat16,
                          device=dev)
        q = qkv[:, : H * D].view(S * L, H, D)
        k = qkv[:, H * D : (H + Hkv) * D].view(S * L, Hkv, D)
        v = qkv[:, (H + Hkv) * D :].view(S * L, Hkv, D)
        cu = torch.arange(0, S * L + 1, L, dtype=torch.int32, device=dev)
        scale = 1.0 / math.sqrt(D)
        outs = [ops.flash_prefill_varlen(q, k, v, cu, L, scale)
                for _ in range(3)]
        torch.cuda.synchronize()
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        # fp32 reference for the first and last sequence
        for s in (0, S - 1):
            sl = slice(s * L, (s + 1) * L)
            ref = torch_ref.flash_prefill_varlen(
                q[sl].float(), k[sl].float(), v[sl].float(),
                cu[:2], scale,
            )
            bf16_close(outs[0][sl], ref, atol=3e-2, rtol=3e-2)

    @pytest.mark.parametrize(
        "qlens,ctx_extra,H,Hkv",
        [
            ([64], [128], 32, 8),       # single resumed chunk
            ([128, 32, 5], [0, 64, 200], 32, 8),  # mixed fresh+resumed
            ([1, 300], [500, 17], 8, 8),          # MHA, long context
            ([256], [0], 16, 4),                  # fresh chunk (ctx==qlen)
        ],
    )
    def test_context_prefill(self, dev, qlens, ctx_extra, H, Hkv):
        """Chunked-prefill paged-context attention vs fp32 torch ref."""
        from kserve_amd import ops

        D, bs = 128, 16
        torch.manual_seed(sum(qlens))
        S = len(qlens)
        ctx = [q_ + e for q_, e in zip(qlens, ctx_extra)]
        max_blocks = max((c + bs - 1) // bs for c in ctx)
        B = S * max_blocks + 1
        kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
            S, max_blocks
        )
        total_q = sum(qlens)
        cu = torch.tensor(
            [0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32
        )
        ctx_t = torch.tensor(ctx, dtype=torch.int32)
        q = torch.randn(total_q, H, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.context_attention_varlen(
            q, kc, vc, bt.to(dev), cu.to(dev), ctx_t.to(dev), max(qlens), scale
        )
        ref = torch_ref.context_attention_varlen(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, cu,
            ctx_t, scale
        )
        bf16_close(got, ref, atol=3e-2, rtol=3e-2)


    def test_paged_decode_fp8(self, dev):
        """fp8 E4M3 KV cache decode vs fp32 ref reading the SAME quantized
        cache (so only the kernel's conversion/accumulation is under test)."""
        from kserve_amd import ops

        S, H, Hkv, ctx_max, D, bs = 32, 32, 8, 300, 128, 16
        torch.manual_seed(99)
        ctx = torch.randint(1, ctx_max + 1, (S,), dtype=torch.int32)
        max_blocks = int((int(ctx.max()) + bs - 1) // bs)
        B = S * max_blocks + 1
        kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev).to(
            torch.float8_e4m3fn
        )
        vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev).to(
            torch.float8_e4m3fn
        )
        bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
            S, max_blocks
        )
        q = torch.randn(S, H, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.paged_attention_decode(q, kc, vc, bt.to(dev), ctx.to(dev), scale)
        ref = torch_ref.paged_attention_decode(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, ctx, scale
        )
        bf16_close(got, ref)

    def test_reshape_and_cache_fp8(self, dev):
        from kserve_amd import ops

        T, Hkv, D, bs, B = 50, 8, 128, 16, 32
        torch.manual_seed(1)
        k = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(B, Hkv, bs, D, dtype=torch.float8_e4m3fn, device=dev)
        vc = torch.zeros_like(kc)
        slots = torch.randperm(B * bs, device=dev)[:T].to(torch.int32)
        ops.reshape_and_cache(k, v, kc, vc, slots)
        torch.cuda.synchronize()
        kc_ref = torch.zeros(B, Hkv, bs, D, dtype=torch.float8_e4m3fn)
        vc_ref = torch.zeros_like(kc_ref)
        torch_ref.reshape_and_cache(k.cpu(), v.cpu(), kc_ref, vc_ref, slots.cpu())
        # both sides quantize bf16 -> E4M3 round-to-nearest: bit comparable
        torch.testing.assert_close(
            kc.float().cpu(), kc_ref.float(), atol=0.08, rtol=0.08
        )
        torch.testing.assert_close(
            vc.float().cpu(), vc_ref.float(), atol=0.08, rtol=0.08
        )

    def test_context_prefill_fp8(self, dev):
        from kserve_amd import ops

        D, bs = 128, 16
        torch.manual_seed(5)
        qlens, ctx_extra, H, Hkv = [48, 7], [100, 30], 32, 8
        S = len(qlens)
        ctx = [a + b for a, b in zip(qlens, ctx_extra)]
        max_blocks = max((c + bs - 1) // bs for c in ctx)
        B = S * max_blocks + 1
        kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev).to(
            torch.float8_e4m3fn
        )
        vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev).to(
            torch.float8_e4m3fn
        )
        bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
            S, max_blocks
        )
        cu = torch.tensor([0] + list(torch.tensor(qlens).cumsum(0)), dtype=torch.int32)
        ctx_t = torch.tensor(ctx, dtype=torch.int32)
        q = torch.randn(sum(qlens), H, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.context_attention_varlen(
            q, kc, vc, bt.to(dev), cu.to(dev), ctx_t.to(dev), max(qlens), scale
        )
        ref = torch_ref.context_attention_varlen(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, cu,
            ctx_t, scale
        )
        bf16_close(got, ref, atol=3e-2, rtol=3e-2)


class TestSampling:
    def test_greedy(self, dev):
        from kserve_amd import ops

        logits = torch.randn(32, 128256, dtype=torch.bfloat16, device=dev)
        got = ops.greedy_sample(logits)
        ref = logits.float().argmax(dim=-1).cpu()
        assert (got.cpu() == ref).all()

    def test_gumbel_distribution(self, dev):
        """Gumbel-max sampling matches softmax probabilities statistically."""
        import kserve_amd_C

        vocab = 8
        probs = torch.tensor([0.4, 0.2, 0.15, 0.1, 0.05, 0.05, 0.03, 0.02])
        logits_row = probs.log().to(torch.bfloat16)
        n = 4096
        logits = logits_row.repeat(n, 1).to(dev)
        temps = torch.ones(n, dtype=torch.float32, device=dev)
        top_k = torch.full((n,), -1, dtype=torch.int32, device=dev)
        seeds = torch.arange(n, dtype=torch.int64, device=dev) * 7919
        out = torch.empty(n, dtype=torch.int64, device=dev)
        kserve_amd_C.gumbel_sample(out, logits, temps, top_k, seeds)
        torch.cuda.synchronize()
        counts = torch.bincount(out.cpu(), minlength=vocab).float() / n
        assert torch.allclose(counts, probs, atol=0.05), counts

    def test_gumbel_determinism(self, dev):
        import kserve_amd_C

        logits = torch.randn(16, 1000, dtype=torch.bfloat16, device=dev)
        temps = torch.full((16,), 0.8, dtype=torch.float32, device=dev)
        top_k = torch.full((16,), -1, dtype=torch.int32, device=dev)
        seeds = torch.arange(16, dtype=torch.int64, device=dev)
        out1 = torch.empty(16, dtype=torch.int64, device=dev)
        out2 = torch.empty(16, dtype=torch.int64, device=dev)
        kserve_amd_C.gumbel_sample(out1, logits, temps, top_k, seeds)
        kserve_amd_C.gumbel_sample(out2, logits, temps, top_k, seeds)
        torch.cuda.synchronize()
        assert (out1 == out2).all()


    def test_topk_support_and_distribution(self, dev):
        """top-k sampler: support is EXACTLY the top-k set; frequencies match
        the renormalized softmax."""
        import kserve_amd_C

        vocab = 1024
        torch.manual_seed(3)
        logits_row = torch.randn(vocab, dtype=torch.bfloat16)
        k = 8
        # bf16 rounding can tie values at the k-th rank; the kernel includes
        # all ties of the k-th value (sorted-cumsum semantics do too)
        kth = logits_row.float().topk(k).values.min()
        topk_idx = set(
            torch.nonzero(logits_row.float() >= kth).flatten().tolist()
        )
        n = 8192
        logits = logits_row.repeat(n, 1).to(dev)
        temps = torch.ones(n, dtype=torch.float32, device=dev)
        top_p = torch.ones(n, dtype=torch.float32, device=dev)
        top_k = torch.full((n,), k, dtype=torch.int32, device=dev)
        seeds = torch.arange(n, dtype=torch.int64, device=dev) * 104729
        out = torch.empty(n, dtype=torch.int64, device=dev)
        kserve_amd_C.topk_topp_sample(out, logits, temps, top_p, top_k, seeds)
        torch.cuda.synchronize()
        got = out.cpu()
        assert set(got.tolist()) <= topk_idx, set(got.tolist()) - topk_idx
        # renormalized probabilities over the (tie-widened) top-k set
        idx = torch.tensor(sorted(topk_idx))
        p_ref = torch.softmax(logits_row.float()[idx], dim=-1)
        counts = torch.zeros(len(idx))
        for j, i in enumerate(idx.tolist()):
            counts[j] = (got == i).sum()
        assert torch.allclose(counts / n, p_ref, atol=0.04), (counts / n, p_ref)

    def test_topp_support(self, dev):
        """top-p sampler: support equals the sorted-cumsum top-p set."""
        import kserve_amd_C

        vocab = 4096
        torch.manual_seed(7)
        logits_row = (torch.randn(vocab) * 3).to(torch.bfloat16)
        p = 0.85
        # reference top-p set: sorted desc, include until cumsum >= p
        pr = torch.softmax(logits_row.float(), dim=-1)
        vals, order = pr.sort(descending=True)
        keep = int((vals.cumsum(0) < p).sum()) + 1
        allowed = set(order[:keep].tolist())
        n = 8192
        logits = logits_row.repeat(n, 1).to(dev)
        temps = torch.ones(n, dtype=torch.float32, device=dev)
        top_p = torch.full((n,), p, dtype=torch.float32, device=dev)
        top_k = torch.full((n,), -1, dtype=torch.int32, device=dev)
        seeds = torch.arange(n, dtype=torch.int64, device=dev) * 7919 + 13
        out = torch.empty(n, dtype=torch.int64, device=dev)
        kserve_amd_C.topk_topp_sample(out, logits, temps, top_p, top_k, seeds)
        torch.cuda.synchronize()
        got = set(out.cpu().tolist())
        # bf16 ties at the boundary value may widen the set by equal-valued
        # tokens; anything sampled outside must have the boundary value
        boundary = logits_row[order[keep - 1]]
        extra = got - allowed
        for e in extra:
            assert logits_row[e] == boundary, (e, float(logits_row[e]))

    def test_topk_topp_determinism(self, dev):
        import kserve_amd_C

        torch.manual_seed(11)
        logits = torch.randn(32, 128256, dtype=torch.bfloat16, device=dev)
        temps = torch.full((32,), 0.7, dtype=torch.float32, device=dev)
        # top_p left at 1.0: the mass histogram uses float atomics, whose
        # ordering can flip an exact-boundary token between runs; the top-k
        # threshold is integer-exact and must be bit-deterministic
        top_p = torch.ones(32, dtype=torch.float32, device=dev)
        top_k = torch.full((32,), 50, dtype=torch.int32, device=dev)
        seeds = torch.arange(32, dtype=torch.int64, device=dev)
        out1 = torch.empty(32, dtype=torch.int64, device=dev)
        out2 = torch.empty(32, dtype=torch.int64, device=dev)
        kserve_amd_C.topk_topp_sample(out1, logits, temps, top_p, top_k, seeds)
        kserve_amd_C.topk_topp_sample(out2, logits, temps, top_p, top_k, seeds)
        torch.cuda.synchronize()
        assert (out1 == out2).all()

    def test_topk1_is_argmax_with_ties(self, dev):
        """top_k=1 must give greedy's token for every seed, also when several
        logits tie for the maximum in bf16 (random small models do this): the
        lowest index wins, as in greedy_sample."""
        import kserve_amd_C

        from kserve_amd import ops

        S, V = 64, 2051  # V not a multiple of 8 or 256
        torch.manual_seed(12)
        logits = torch.randn(S, V, dtype=torch.bfloat16, device=dev)
        top = logits.float().max(dim=-1).values.to(torch.bfloat16)
        # 1-4 extra copies of each row's maximum at random places
        g = torch.Generator().manual_seed(3)
        for s in range(S):
            idx = torch.randint(0, V, (1 + s % 4,), generator=g)
            logits[s, idx.to(dev)] = top[s]
        want = ops.greedy_sample(logits)
        ref = (logits.float() == logits.float().max(-1, keepdim=True).values)
        assert torch.equal(want.cpu(), ref.cpu().float().argmax(-1))
        assert int(ref.sum(-1).min()) >= 2
        temps = torch.full((S,), 0.7, dtype=torch.float32, device=dev)
        top_p = torch.ones(S, dtype=torch.float32, device=dev)
        top_k = torch.ones(S, dtype=torch.int32, device=dev)
        for base in (0, 5, 1 << 20):
            seeds = torch.arange(S, dtype=torch.int64, device=dev) * 7919 + base
            out = torch.empty(S, dtype=torch.int64, device=dev)
            kserve_amd_C.topk_topp_sample(out, logits, temps, top_p, top_k, seeds)
            assert torch.equal(out, want)


class TestSkinnyGemm:
    @pytest.mark.parametrize(
        "N,K,M",
        [
            (256, 4096, 6144),   # qkv
            (256, 14336, 4096),  # down (split-K path)
            (64, 4096, 4096),    # o_proj small batch
            (1, 4096, 6144),     # single-token decode
            (17, 512, 128),      # ragged N, tiny
            (256, 4096, 128256), # lm_head (no split)
        ],
    )
    def test_skinny_gemm_matches_matmul(self, dev, N, K, M):
        import kserve_amd_C

        torch.manual_seed(N + K)
        x = torch.randn(N, K, dtype=torch.bfloat16, device=dev) / 8
        w = torch.randn(M, K, dtype=torch.bfloat16, device=dev) / 8
        out = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.skinny_gemm(out, x, w)
        torch.cuda.synchronize()
        ref = (x.float() @ w.float().t())
        torch.testing.assert_close(
            out.float(), ref, atol=0.05, rtol=0.05
        )

    def test_skinny_gemm_strided_x(self, dev):
        import kserve_amd_C

        x_full = torch.randn(64, 8192, dtype=torch.bfloat16, device=dev) / 8
        x = x_full[:, :4096]  # strided rows
        w = torch.randn(1024, 4096, dtype=torch.bfloat16, device=dev) / 8
        out = torch.empty(64, 1024, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.skinny_gemm(out, x, w)
        torch.cuda.synchronize()
        ref = x.float() @ w.float().t()
        torch.testing.assert_close(out.float(), ref, atol=0.05, rtol=0.05)


class TestGemm8Experimental:
    """8-phase MFMA GEMM (experimental; not in the serving path).
    GPU-validated round 2 across the full SW x SCHED matrix — runs by
    default now; KS_GEMM8=0 skips."""

    @pytest.mark.skipif(
        __import__("os").environ.get("KS_GEMM8") == "0",
        reason="disabled with KS_GEMM8=0",
    )
    @pytest.mark.parametrize("M,N,K", [(256, 256, 64), (256, 256, 256),
                                       (512, 512, 512), (512, 256, 4096)])
    @pytest.mark.parametrize("swizzle", [0, 1, 2])
    def test_gemm8_matches_matmul(self, dev, M, N, K, swizzle):
        import kserve_amd_C

        torch.manual_seed(M + K)
        a = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
        d = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        kserve_amd_C.gemm8(d, a, w, swizzle)
        torch.cuda.synchronize()
        # random (non-symmetric) inputs: transpose bugs cannot hide
        ref = (a.float() @ w.float().t())
        torch.testing.assert_close(
            d.float(), ref, atol=K * 2e-3, rtol=3e-2
        )


class TestSlidingWindowKernels:
    """Window-bounded attention vs fp32 torch references (Mistral-family):
    the HIP kernels take a `window` arg and must match the masked refs for
    contexts beyond the window, across split-context and variant dispatch.

    Inputs are unscaled randn: with q/k/v scaled by 1/4 attention is almost
    uniform and a window of W+1 or W-1 moved the prefill outputs by less
    than the 2e-2 allowance; unscaled, the fp32 reference with W+-1 misses
    it by 0.08-0.7 (wherever T > W). tests/test_gpu_attention.py holds the
    cases built to catch off-by-one masks."""

    @pytest.mark.parametrize(
        "S,H,Hkv,ctx_max,W",
        [
            (4, 32, 8, 300, 64),    # llama-8b shape, window < ctx
            (2, 8, 2, 700, 128),    # long ctx, deep split
            (8, 4, 4, 50, 64),      # window > ctx (no-op)
            (200, 32, 8, 400, 96),  # V4 large-batch variant
        ],
    )
    def test_decode_window(self, dev, S, H, Hkv, ctx_max, W):
        from kserve_amd import ops

        D, bs = 128, 16
        torch.manual_seed(S + W)
        ctx = torch.randint(max(1, ctx_max // 2), ctx_max + 1, (S,),
                            dtype=torch.int32)
        max_blocks = int((int(ctx.max()) + bs - 1) // bs)
        B = S * max_blocks + 1
        kc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(B, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        bt = torch.arange(1, S * max_blocks + 1, dtype=torch.int32).reshape(
            S, max_blocks
        )
        q = torch.randn(S, H, D, dtype=torch.bfloat16, device=dev)
        scale = 1.0 / math.sqrt(D)
        got = ops.paged_attention_decode(
            q, kc, vc, bt.to(dev), ctx.to(dev), scale, window=W
        )
        ref = torch_ref.paged_attention_decode(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, ctx,
            scale, window=W,
        )
        bf16_close(got, ref)

    @pytest.mark.parametrize("T,W", [(200, 64), (64, 64), (333, 100)])
    def test_flash_prefill_window(self, dev, T, W):
        from kserve_amd import ops

        H, Hkv, D = 8, 2, 128
        torch.manual_seed(T)
        q = torch.randn(T, H, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(T, Hkv, D, dtype=torch.bfloat16, device=dev)
        cu = torch.tensor([0, T], dtype=torch.int32)
        scale = 1.0 / math.sqrt(D)
        got = ops.flash_prefill_varlen(
            q, k, v, cu.to(dev), T, scale, window=W
        )
        ref = torch_ref.flash_prefill_varlen(
            q.float().cpu(), k.float().cpu(), v.float().cpu(), cu, scale,
            causal=True, window=W,
        )
        bf16_close(got, ref)

    def test_context_prefill_window(self, dev):
        from kserve_amd import ops

        H, Hkv, D, bs = 8, 2, 128, 16
        ctx, n_new, W = 150, 30, 48
        torch.manual_seed(7)
        nb = -(-ctx // bs)
        kc = torch.randn(nb + 1, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        vc = torch.randn(nb + 1, Hkv, bs, D, dtype=torch.bfloat16, device=dev)
        bt = torch.arange(1, nb + 1, dtype=torch.int32).unsqueeze(0)
        q = torch.randn(n_new, H, D, dtype=torch.bfloat16, device=dev)
        cu_q = torch.tensor([0, n_new], dtype=torch.int32)
        cl = torch.tensor([ctx], dtype=torch.int32)
        scale = 1.0 / math.sqrt(D)
        got = ops.context_attention_varlen(
            q, kc, vc, bt.to(dev), cu_q.to(dev), cl.to(dev), n_new, scale,
            window=W,
        )
        ref = torch_ref.context_attention_varlen(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt, cu_q,
            cl, scale, window=W,
        )
        bf16_close(got, ref)
