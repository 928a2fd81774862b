"""GPU: the attention kernels, reshape_and_cache and RoPE on the adversarial
cases of tests/attention_cases.py (needles, poison, permuted wide block
tables, shared prefixes, strided q/k/v), against the fp64 reference and its
derived elementwise allowance. tests/test_attention_cases.py shows on the CPU
that every near-miss of the reference fails this same comparison by >= 10x.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from kserve_amd.ops import torch_ref
from tests import attention_cases as ac


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from kserve_amd import ops

    assert ops.has_native(), "native extension must be present on the GPU box"
    return torch.device("cuda:0")


def _check(case, dev):
    ratio = ac.gpu_ratio(case, dev)
    print(f"{case.name}: worst err/allowance = {ratio:.3f}")
    assert ratio <= 1.0, (
        f"{case.name}: worst |got-ref| is {ratio:.2f}x the allowance "
        f"(eps_P = 2^{int(round(torch.log2(torch.tensor(case.eps_p)).item()))})"
    )


@pytest.mark.parametrize("name", [c.name for c in ac.DECODE_CASES])
def test_decode(dev, name):
    _check(ac.CASES_BY_NAME[name], dev)


@pytest.mark.parametrize("name", [c.name for c in ac.DECODE_FP8_CASES])
def test_decode_fp8(dev, name):
    _check(ac.CASES_BY_NAME[name], dev)


@pytest.mark.parametrize("name", [c.name for c in ac.FLASH_CASES])
def test_flash_prefill(dev, name):
    _check(ac.CASES_BY_NAME[name], dev)


@pytest.mark.parametrize("name", [c.name for c in ac.CONTEXT_CASES])
def test_context_prefill(dev, name):
    _check(ac.CASES_BY_NAME[name], dev)


# ---------------------------------------------------------------------------
# reshape_and_cache: strided k/v, padding slots, page-edge slots, bit-exact
# untouched cache
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hkv,D", [(2, 128), (3, 64)])
def test_reshape_and_cache_padding_and_edges(dev, fp8, Hkv, D):
    from kserve_amd import ops

    bs, B = ac.PAGE, 5
    g = torch.Generator().manual_seed(11 + Hkv)
    # first and last slot of a page, a page in the middle, and -1 padding
    slots = torch.tensor([0, -1, bs - 1, 2 * bs, -1, 3 * bs + 7, 5 * bs - 1,
                          -1, bs], dtype=torch.int32)
    T = slots.numel()
    kv = (torch.rand(T, 2 * Hkv * D + 16, generator=g) * 4 - 2).to(torch.bfloat16)
    kv = kv.to(dev)
    k = kv[:, 8:8 + Hkv * D].view(T, Hkv, D)
    v = kv[:, 8 + Hkv * D:8 + 2 * Hkv * D].view(T, Hkv, D)
    assert not k.is_contiguous() and not v.is_contiguous()
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    # sentinel: a bit pattern no conversion of the inputs (|x| <= 2) gives
    sent_k = torch.full((B, Hkv, bs, D), 96.0).to(cdt).to(dev)
    sent_v = torch.full((B, Hkv, bs, D), -80.0).to(cdt).to(dev)
    kc, vc = sent_k.clone(), sent_v.clone()
    ops.reshape_and_cache(k, v, kc, vc, slots.to(dev))
    torch.cuda.synchronize()

    exp_k, exp_v = sent_k.cpu().clone(), sent_v.cpu().clone()
    keep = slots >= 0
    torch_ref.reshape_and_cache(
        k.cpu()[keep].contiguous(), v.cpu()[keep].contiguous(), exp_k, exp_v,
        slots[keep])
    def by_token(t, bits):
        t = t.cpu()
        t = t.view(torch.uint8 if fp8 else torch.int16) if bits else t.float()
        return t.permute(0, 2, 1, 3).reshape(B * bs, Hkv * D)

    written = torch.zeros(B * bs, dtype=torch.bool)
    written[slots[keep].long()] = True
    for got, exp, sent in ((kc, exp_k, sent_k), (vc, exp_v, sent_v)):
        # untouched slots (padding rows write nothing): bit for bit
        assert torch.equal(by_token(got, True)[~written],
                           by_token(sent, True)[~written])
        # written slots: the same value (bf16 copy, or E4M3 round-to-nearest
        # of a bf16 value, is unique up to the sign of zero)
        assert torch.equal(by_token(got, False)[written],
                           by_token(exp, False)[written])
        assert bool((by_token(got, True)[written]
                     != by_token(sent, True)[written]).any(dim=1).all())


# ---------------------------------------------------------------------------
# RoPE on strided q/k at D=64, positions 0 and max_pos - 1
# ---------------------------------------------------------------------------
def test_rotary_embedding_d64_strided(dev):
    from kserve_amd import ops

    T, H, Hkv, D, max_pos = 9, 6, 2, 64, 4096
    g = torch.Generator().manual_seed(5)
    cs = torch_ref.make_cos_sin_cache(D, max_pos)
    pos = torch.tensor([0, max_pos - 1, 1, 17, 0, 2048, max_pos - 1, 63, 64],
                       dtype=torch.int64)
    qkv = torch.randn(T, (H + 2 * Hkv) * D + 8, generator=g).to(torch.bfloat16)
    qkv_dev = qkv.to(dev)
    q = qkv_dev[:, :H * D].view(T, H, D)
    k = qkv_dev[:, H * D:(H + Hkv) * D].view(T, Hkv, D)
    assert not q.is_contiguous() and not k.is_contiguous()
    q_ref, k_ref = torch_ref.rotary_embedding(
        pos, qkv[:, :H * D].view(T, H, D).double(),
        qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D).double(), cs.double())
    ops.rotary_embedding(pos.to(dev), q, k, cs.to(dev))
    torch.cuda.synchronize()
    got = qkv_dev.cpu()
    # fp32 math on bf16 inputs, one bf16 rounding on store: within one ulp
    # (2^-8 relative) of the exact value, plus fp32 noise of the two-term sum
    for got_x, ref_x in ((got[:, :H * D].view(T, H, D), q_ref),
                         (got[:, H * D:(H + Hkv) * D].view(T, Hkv, D), k_ref)):
        err = (got_x.double() - ref_x).abs()
        assert bool((err <= 2.0 ** -8 * ref_x.abs() + 1e-6).all()), float(err.max())
    # position 0 is the identity; v and the pad columns are untouched
    assert torch.equal(got[0, :(H + Hkv) * D], qkv[0, :(H + Hkv) * D])
    assert torch.equal(got[:, (H + Hkv) * D:], qkv[:, (H + Hkv) * D:])
