"""Adversarial attention cases, an fp64 reference of its own and a derived
comparator. Helper module: imported by test_attention_cases.py (CPU),
test_gpu_attention.py and attention_variant_child.py; not collected.

Why this exists: random dense inputs with an identity block table and a flat
2e-2 tolerance accept a window that is off by one, a kernel that never reads
the block table, and one that reads a slot past ``context_lens``. The cases
here are built so that each of those mistakes moves some output by O(1):

* **Needles.** A needle is a key whose score is well above the rest (q has a
  common positive offset in every dim, the needle key is a positive constant
  in every dim) and whose value has a spike of magnitude 8-24 in a dim of its
  own. Dropping a visible needle removes ``p * spike`` from that dim; letting
  an invisible one in adds it. Because the spike dim belongs to that needle
  alone, ``absmass`` there is dominated by the needle itself, so the change
  stays ~100x the allowance however many other needles share the softmax.
  Must-see needles sit on the last valid token, the first token inside the
  window and the first and last token of every page (split boundaries are
  page boundaries). Must-ignore needles sit on the first slot after ``ctx``,
  on ``wstart - 1``, on slot 0 of every unreferenced page, and in varlen
  prefill on the row after the packed tokens; there the last key of the
  previous sequence and key ``i + 1`` are ordinary must-see needles of other
  rows.
* **Poison.** Every other slot after ``ctx`` in the last page, every page no
  valid table entry references, and block 0 hold large finite values of
  alternating sign (+-3e38 bf16, +-448 fp8). Unused table entries point at
  such a page. NaN/Inf are left out on purpose: the kernels are exact for any
  finite stale data and undefined for non-finite (see
  ``ops.paged_attention_decode``).
* **Block tables** are wider than any sequence needs, ids are permuted
  across sequences, and some cases share the first pages of two sequences.

The comparator is elementwise
``|got - ref| <= 2^-8 |ref| + eps_P * absmass + 1e-6`` with
``absmass = P @ |V|``: the rounding of the bf16 output (round-to-nearest is
off by at most half an ulp, which is 2^-8 |x| at the bottom of a binade, so a
correctly rounded output alone can use this term up) plus the kernel's
internal rounding scaled by what was actually summed. ``eps_P`` is derived,
not fitted:
2^-8 where the PV product runs on MFMA (P is rounded to bf16 once for the
product, and the normaliser sums the unrounded P), 2^-12 for the decode
kernels whose PV is fp32 FMA (bf16 x bf16 products are exact in fp32; what is
left is ``__expf`` and summation order).
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

PAGE = 16
OUT_ULP = 2.0 ** -8      # worst round-to-nearest error of a bf16 output
EPS_MFMA = 2.0 ** -8     # PV on MFMA: P rounded to bf16
EPS_FMA = 2.0 ** -12     # PV in fp32 FMA
ABS_FLOOR = 1e-6
POISON_BF16 = 3e38
POISON_FP8 = 448.0
TABLE_SLACK = 3          # table columns beyond the longest sequence's need
Q_OFFSET = 0.5           # common positive offset of every q dim
OUT_SENTINEL = 12345.0   # decode output pre-fill


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                # "decode" | "context" | "flash"
    Hkv: int
    group: int
    D: int
    ctx: Tuple[int, ...] = ()      # decode/context: context length per seq
    q_lens: Tuple[int, ...] = ()   # context: new tokens; flash: seq lengths
    window: int = 0
    causal: bool = True
    fp8: bool = False
    share_prefix: bool = False
    seed: int = 0

    @property
    def H(self) -> int:
        return self.Hkv * self.group

    @property
    def S(self) -> int:
        return len(self.ctx) if self.kind != "flash" else len(self.q_lens)

    @property
    def eps_p(self) -> float:
        return EPS_FMA if self.kind == "decode" else EPS_MFMA


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------
DECODE_CTX = (1, 15, 16, 17, 31, 32, 33, 200)
DECODE_W = 48
DECODE_WIN_CTX = (DECODE_W - 1, DECODE_W, DECODE_W + 1, DECODE_W + 15,
                  DECODE_W + 16, DECODE_W + 17, 200)
# (Hkv, group, D): groups 1, 3, 4, 5, 8; D=64 for groups 1 and 8
DECODE_HEADS = ((2, 1, 128), (2, 3, 128), (1, 4, 128), (2, 4, 128),
                (1, 5, 128), (2, 5, 128), (2, 8, 128), (1, 1, 64), (2, 8, 64))


def _v4_ctx(n: int, lo: int, hi: int, seed: int) -> Tuple[int, ...]:
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(lo, hi + 1, (n,), generator=g).tolist()
    # make sure the edges are in the batch
    c[0], c[1], c[2], c[3] = hi, lo, 16, 17
    return tuple(c)


def _decode_cases() -> List[Case]:
    out = []
    for i, (hkv, g, d) in enumerate(DECODE_HEADS):
        tag = f"kv{hkv}g{g}d{d}"
        out.append(Case(f"dec_{tag}", "decode", hkv, g, d, ctx=DECODE_CTX,
                        seed=100 + i))
        out.append(Case(f"dec_{tag}_w{DECODE_W}", "decode", hkv, g, d,
                        ctx=DECODE_WIN_CTX, window=DECODE_W, seed=200 + i))
    # two sequences sharing their first pages (prefix cache)
    out.append(Case("dec_share_kv2g4d128", "decode", 2, 4, 128,
                    ctx=(200, 100, 33, 16), share_prefix=True, seed=300))
    # S=4: the smallest batch the forced wide-V variant is run at
    out.append(Case("dec_s4_kv2g4d128", "decode", 2, 4, 128,
                    ctx=(1, 17, 33, 200), seed=301))
    out.append(Case(f"dec_s4_kv2g4d128_w{DECODE_W}", "decode", 2, 4, 128,
                    ctx=(DECODE_W - 1, DECODE_W + 1, DECODE_W + 17, 200),
                    window=DECODE_W, seed=302))
    # S=129 > 128: the auto-dispatched wide-V kernel
    out.append(Case("dec_s129_kv1g4d128", "decode", 1, 4, 128,
                    ctx=_v4_ctx(129, 1, 40, 1), seed=303))
    out.append(Case("dec_s129_kv1g4d128_w24", "decode", 1, 4, 128,
                    ctx=_v4_ctx(129, 1, 40, 2), window=24, seed=304))
    return out


def _decode_fp8_cases() -> List[Case]:
    out = []
    for i, g in enumerate((1, 2, 4)):
        out.append(Case(f"dec8_kv2g{g}", "decode", 2, g, 128, ctx=DECODE_CTX,
                        fp8=True, seed=400 + i))
        out.append(Case(f"dec8_kv2g{g}_w{DECODE_W}", "decode", 2, g, 128,
                        ctx=DECODE_WIN_CTX, window=DECODE_W, fp8=True,
                        seed=410 + i))
    return out


FLASH_HEADS = ((1, 4), (3, 1), (2, 4))   # H/Hkv = (4,1), (3,3), (8,2)
FLASH_LENS = ((1,), (63, 64, 65), (1, 129, 31))
FLASH_WINDOWS = (1, 16, 63, 64, 65)
FLASH_WIN_T = 130


def _flash_cases() -> List[Case]:
    out = []
    n = 0
    for hkv, g in FLASH_HEADS:
        for d in (128, 64):
            tag = f"kv{hkv}g{g}d{d}"
            for lens in FLASH_LENS:
                ltag = "x".join(str(x) for x in lens)
                for causal in (True, False):
                    n += 1
                    out.append(Case(
                        f"fl_{tag}_{'c' if causal else 'nc'}_{ltag}", "flash",
                        hkv, g, d, q_lens=lens, causal=causal, seed=500 + n))
            for w in FLASH_WINDOWS:
                n += 1
                out.append(Case(f"fl_{tag}_w{w}", "flash", hkv, g, d,
                                q_lens=(FLASH_WIN_T,), window=w,
                                seed=500 + n))
    return out


# (q_len, past), mixed in one batch
CONTEXT_SHAPES = ((1, 0), (1, 200), (33, 0), (33, 31), (64, 64), (5, 123))
CONTEXT_WINDOWS = (0, 16, 48, 65)


def _context_cases() -> List[Case]:
    out = []
    n = 0
    for fp8 in (False, True):
        for hkv, g in ((2, 4), (1, 3)):
            for w in CONTEXT_WINDOWS:
                n += 1
                out.append(Case(
                    f"ctx{'8' if fp8 else ''}_kv{hkv}g{g}"
                    + (f"_w{w}" if w else ""),
                    "context", hkv, g, 128,
                    ctx=tuple(q + p for q, p in CONTEXT_SHAPES),
                    q_lens=tuple(q for q, _ in CONTEXT_SHAPES),
                    window=w, fp8=fp8, share_prefix=True, seed=700 + n))
    return out


DECODE_CASES = _decode_cases()
DECODE_FP8_CASES = _decode_fp8_cases()
FLASH_CASES = _flash_cases()
CONTEXT_CASES = _context_cases()
ALL_CASES = DECODE_CASES + DECODE_FP8_CASES + FLASH_CASES + CONTEXT_CASES
CASES_BY_NAME: Dict[str, Case] = {c.name: c for c in ALL_CASES}
assert len(CASES_BY_NAME) == len(ALL_CASES)


# ---------------------------------------------------------------------------
# decode dispatch, mirrored from bindings.cpp / ks_paged_attention_decode
# ---------------------------------------------------------------------------
def decode_n_splits(S: int, H: int, Hkv: int, max_blocks: int,
                    override: int = 0) -> int:
    """The split-context heuristic of the paged_attention_decode binding."""
    base = S * Hkv
    grp = H // Hkv
    n = 1
    if override > 0:
        n = override
    elif grp <= 4 and base <= 512:
        n = min(8, max(2, 2048 // base))
    elif base < 512:
        n = min(16, (512 + base - 1) // base)
    if n > 1 and (max_blocks + n - 1) // n < 1:
        n = 1
    return n


def split_first_tokens(ctx: int, window: int, n_splits: int) -> List[int]:
    """Positions of the first token of every split but the first (the token
    right after each split boundary), as the decode kernels partition the
    window's pages."""
    nblocks = -(-ctx // PAGE)
    wstart = ctx - window if (window > 0 and ctx > window) else 0
    first_blk = wstart // PAGE
    bps = -(-(nblocks - first_blk) // n_splits)
    out = []
    for sp in range(1, n_splits):
        blk = first_blk + sp * bps
        if blk < nblocks:
            out.append(blk * PAGE)
    return out


def expected_decode_kernel(case: Case, env: Dict[str, str]) -> str:
    """Which bf16 decode kernel ks_paged_attention_decode launches for this
    case under ``env`` (fp8 caches: which QK chain). Mirrors the dispatch
    order in attention_decode.hip; a variant test asserts on this so that a
    case cannot fall through to the default kernel unnoticed."""
    def flag(name):  # "=1 enables"
        return env.get(name, "")[:1] == "1"

    def tri(name):   # -1 auto, 0 off, 1 on
        v = env.get(name)
        return -1 if v is None else (1 if v[:1] == "1" else 0)

    if case.fp8:
        return "fp8_fma" if env.get("KS_FP8_CVTB", "1")[:1] == "0" else "fp8_cvtb"
    g, d, S = case.group, case.D, case.S
    hpw = (g + 3) // 4
    fast = hpw == 1 and d == 128
    if flag("KS_ATTN_WS") and g in (1, 2, 4, 8) and d == 128:
        return "ws"
    if flag("KS_ATTN_H2") and g == 4 and d == 128:
        return "h2"
    if flag("KS_ATTN_MQ") and fast:
        return "mq"
    if flag("KS_ATTN_U2") and fast:
        return "u2"
    v4 = tri("KS_ATTN_V4")
    if (v4 == 1 or (v4 == -1 and S > 128)) and fast:
        return "v4d2" if flag("KS_ATTN_V4D2") else "v4"
    d2 = tri("KS_ATTN_D2")
    if (d2 == 1 or (d2 == -1 and S <= 128)) and fast:
        return "d2"
    if env.get("KS_ATTN_PB", "1")[:1] != "0" and fast:
        return "pb"
    occ = int(env.get("KS_ATTN_OCC", "0") or 0)
    if occ >= 5 and fast:
        return "occ6" if occ >= 6 else "occ5"
    return f"generic_d{d}_hpw{hpw}"


# ---------------------------------------------------------------------------
# input builder
# ---------------------------------------------------------------------------
def _round(x: torch.Tensor, fp8: bool) -> torch.Tensor:
    """Round to the storage format, return as float32."""
    if fp8:
        return x.to(torch.float8_e4m3fn).float()
    return x.to(torch.bfloat16).float()


def _needle_key(D: int) -> float:
    # score = scale * a * sum(q) ~ a * (Q_OFFSET * sqrt(D) + N(0, 1)):
    # 4.2 +- 0.75 at D=128, 4 +- 1 at D=64, against N(0, 1.25) for the rest.
    # Both constants are exact in bf16 and E4M3.
    return 0.75 if D == 128 else 1.0


class _NeedleWriter:
    def __init__(self, case: Case):
        self.case = case
        self.n = 0
        self.a = _needle_key(case.D)

    def put(self, krow: torch.Tensor, vrow: torch.Tensor) -> None:
        """krow/vrow: [Hkv, D] views of one token's K and V."""
        dim = (5 * self.n + 1) % self.case.D   # 5 is coprime to 64 and 128
        sign = 1.0 if self.n % 2 == 0 else -1.0
        self.n += 1
        krow[:] = self.a
        for kvh in range(self.case.Hkv):
            vrow[kvh, dim] = sign * 8.0 * (1 + kvh % 3)   # 8, 16, 24


def _poison(case: Case) -> torch.Tensor:
    """[Hkv, D] pattern of alternating sign."""
    mag = POISON_FP8 if case.fp8 else POISON_BF16
    sgn = torch.ones(case.Hkv, case.D)
    sgn[:, 1::2] = -1.0
    sgn[1::2] *= -1.0
    return _round(sgn * mag, case.fp8)


def _build_paged(case: Case, g: torch.Generator) -> SimpleNamespace:
    S, Hkv, D, H = case.S, case.Hkv, case.D, case.H
    ctx = list(case.ctx)
    nb = [-(-c // PAGE) for c in ctx]
    needed = max(nb)
    width = needed + TABLE_SLACK

    # which (seq, page) pairs alias another sequence's page
    alias: Dict[Tuple[int, int], Tuple[int, int]] = {}
    if case.share_prefix:
        order = sorted(range(S), key=lambda s: -ctx[s])
        a, b = order[0], order[1]
        n_shared = min(ctx[a], ctx[b]) // PAGE - 1
        assert n_shared >= 1, "share_prefix needs two sequences of >= 2 full pages"
        for p in range(n_shared):
            alias[(b, p)] = (a, p)

    pairs = [(s, p) for s in range(S) for p in range(nb[s])
             if (s, p) not in alias]
    n_spare = 2
    B = 1 + len(pairs) + n_spare
    ids = (torch.randperm(B - 1, generator=g) + 1).tolist()
    order = torch.randperm(len(pairs), generator=g).tolist()
    page_of: Dict[Tuple[int, int], int] = {}
    for rank, pi in enumerate(order):
        page_of[pairs[pi]] = ids[rank]
    for dst, src in alias.items():
        page_of[dst] = page_of[src]
    poison_pages = [0] + ids[len(pairs):]

    bt = torch.empty(S, width, dtype=torch.int32)
    for s in range(S):
        for p in range(width):
            bt[s, p] = (page_of[(s, p)] if p < nb[s]
                        else poison_pages[(s + p) % len(poison_pages)])

    k_cache = _round(torch.randn(B, Hkv, PAGE, D, generator=g), case.fp8)
    v_cache = _round(torch.rand(B, Hkv, PAGE, D, generator=g) * 2 - 1, case.fp8)
    pz = _poison(case)
    needles = _NeedleWriter(case)

    def slot(s, pos):
        return page_of[(s, pos // PAGE)], pos % PAGE

    # poison: whole unreferenced pages (slot 0 is a must-ignore needle: it
    # is the "first invalid slot" of a sequence whose ctx ends on a page
    # boundary), then the tail of every last page
    for pg in poison_pages:
        k_cache[pg] = pz[:, None, :]
        v_cache[pg] = pz[:, None, :]
        v_cache[pg, :, 0] = 0.0
        needles.put(k_cache[pg, :, 0], v_cache[pg, :, 0])
    for s in range(S):
        for pos in range(ctx[s], nb[s] * PAGE):
            pg, off = slot(s, pos)
            k_cache[pg, :, off] = pz
            v_cache[pg, :, off] = pz

    must_see, must_ignore = [], []
    for s in range(S):
        W = case.window
        wstart = ctx[s] - W if (W > 0 and ctx[s] > W) else 0
        see = {ctx[s] - 1, wstart}
        for p in range(wstart // PAGE, nb[s]):
            for pos in (p * PAGE, p * PAGE + PAGE - 1):
                if wstart <= pos < ctx[s]:
                    see.add(pos)
        ignore = set()
        if ctx[s] % PAGE != 0:
            ignore.add(ctx[s])
        if wstart >= 1:
            ignore.add(wstart - 1)
        for pos in sorted(ignore):
            pg, off = slot(s, pos)
            if pos >= ctx[s]:
                v_cache[pg, :, off] = 0.0
            needles.put(k_cache[pg, :, off], v_cache[pg, :, off])
            must_ignore.append((s, pos))
        for pos in sorted(see):
            pg, off = slot(s, pos)
            needles.put(k_cache[pg, :, off], v_cache[pg, :, off])
            must_see.append((s, pos))

    Tq = S if case.kind == "decode" else sum(case.q_lens)
    q = _round(torch.randn(Tq, H, D, generator=g) + Q_OFFSET, False)
    inp = SimpleNamespace(
        case=case, q=q, k_cache=k_cache, v_cache=v_cache, block_tables=bt,
        context_lens=torch.tensor(ctx, dtype=torch.int32),
        needed_blocks=needed, scale=1.0 / math.sqrt(D),
        must_see=must_see, must_ignore=must_ignore, num_blocks=B,
    )
    if case.kind == "context":
        cu = [0]
        for n in case.q_lens:
            cu.append(cu[-1] + n)
        inp.cu_seqlens_q = torch.tensor(cu, dtype=torch.int32)
        inp.max_q_len = max(case.q_lens)
    return inp


def _build_flash(case: Case, g: torch.Generator) -> SimpleNamespace:
    Hkv, D, H = case.Hkv, case.D, case.H
    lens = list(case.q_lens)
    T = sum(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    # one row past the packed tokens: the "first invalid slot" of the last
    # sequence. The ops get k[:T] / v[:T]; a stray read lands on this needle.
    k = _round(torch.randn(T + 1, Hkv, D, generator=g), False)
    v = _round(torch.rand(T + 1, Hkv, D, generator=g) * 2 - 1, False)
    needles = _NeedleWriter(case)
    must_see = []
    for s, n in enumerate(lens):
        # first/last key (the last is the next sequence's "previous key",
        # the first is row W-1's window edge and row W's must-ignore), the
        # 16/32/64 tile edges, and two interior keys
        pos = {0, n - 1}
        for e in (15, 16, 31, 32, 63, 64, 127, 128):
            if e < n:
                pos.add(e)
        for e in (n // 3, (2 * n) // 3):
            pos.add(e)
        for p in sorted(pos):
            needles.put(k[cu[s] + p], v[cu[s] + p])
            must_see.append((s, p))
    needles.put(k[T], v[T])
    q = _round(torch.randn(T, H, D, generator=g) + Q_OFFSET, False)
    return SimpleNamespace(
        case=case, q=q, k=k, v=v, T=T,
        cu_seqlens=torch.tensor(cu, dtype=torch.int32), max_seqlen=max(lens),
        scale=1.0 / math.sqrt(D), must_see=must_see, must_ignore=[(len(lens) - 1, lens[-1])],
    )


@functools.lru_cache(maxsize=None)
def build(case: Case) -> SimpleNamespace:
    """Inputs of a case as float32 CPU tensors that hold values already
    rounded to the storage format (bf16, or E4M3 for an fp8 cache). Cached:
    callers must not modify them."""
    g = torch.Generator().manual_seed(case.seed)
    if case.kind == "flash":
        return _build_flash(case, g)
    return _build_paged(case, g)


# ---------------------------------------------------------------------------
# fp64 reference with mutants
# ---------------------------------------------------------------------------
MUTANTS = (
    "drop_last",             # drop the last valid token
    "include_first_invalid",  # one key past the last visible one
    "window_plus",           # window W+1
    "window_minus",          # window W-1
    "ignore_table",          # identity block ids
    "row_stride",            # table row stride = needed blocks, not width
    "head_mod",              # h % Hkv instead of h // group
    "drop_page_first",       # drop the first token of every page
    "drop_after_split",      # drop the token after every split boundary
    "causal_strict",         # prefill causal j < i
    "ctx_offset_minus",      # context offset ctx - q_len - 1
    "ctx_offset_plus",       # context offset ctx - q_len + 1
    "prev_seq_leak",         # varlen: last key of the previous sequence
    "noncausal_as_causal",   # bidirectional run with the causal mask
)


def _visible(case: Case, ctx_or_len: int, q_len: int, row: int,
             mutate: Optional[str], seq: int,
             split_firsts: List[int]) -> List[int]:
    """Explicit list of the key positions (local to the sequence) that query
    ``row`` of a sequence sees."""
    W = case.window
    if W > 0:
        if mutate == "window_plus":
            W += 1
        elif mutate == "window_minus":
            W -= 1
    if case.kind == "decode":
        qpos = ctx_or_len - 1
        hi = qpos
    elif case.kind == "context":
        start = ctx_or_len - q_len
        if mutate == "ctx_offset_minus":
            start -= 1
        elif mutate == "ctx_offset_plus":
            start += 1
        qpos = start + row
        hi = min(qpos, ctx_or_len - 1)
    else:
        qpos = row
        causal = case.causal or mutate == "noncausal_as_causal"
        hi = qpos if causal else ctx_or_len - 1
    lo = max(0, qpos - W + 1) if case.window > 0 else 0
    vis = list(range(lo, hi + 1))
    if mutate == "causal_strict" and vis and vis[-1] == qpos:
        vis.pop()
    if mutate == "drop_last" and vis:
        vis.pop()
    if mutate == "include_first_invalid":
        vis.append(max(hi, -1) + 1)
    if mutate == "drop_page_first":
        vis = [j for j in vis if j % PAGE != 0]
    if mutate == "drop_after_split":
        vis = [j for j in vis if j not in split_firsts]
    if mutate == "prev_seq_leak" and seq > 0:
        vis = [-1] + vis
    return vis


def reference(inp: SimpleNamespace, mutate: Optional[str] = None):
    """Position-wise float64 attention. Returns ``(out, absmass, sig)``:
    out and absmass are [Tq, H, D] float64 with ``absmass = P @ |V|``; sig
    identifies, per row, which stored tokens were attended and through which
    kv head map, so a mutant that changes nothing on a case can be told from
    one that does."""
    assert mutate is None or mutate in MUTANTS, mutate
    case: Case = inp.case
    H, Hkv, D, group = case.H, case.Hkv, case.D, case.group
    if mutate == "head_mod":
        kvmap = [h % Hkv for h in range(H)]
    else:
        kvmap = [h // group for h in range(H)]
    q = inp.q.double()
    out = torch.zeros(q.shape, dtype=torch.float64)
    absmass = torch.zeros(q.shape, dtype=torch.float64)
    sig = [tuple(kvmap)]

    paged = case.kind != "flash"
    if paged:
        bt = inp.block_tables.long()
        width = bt.shape[1]
        flat = bt.flatten()
        kc, vc = inp.k_cache.double(), inp.v_cache.double()
        n_splits = decode_n_splits(case.S, H, Hkv, width)
    else:
        kf, vf = inp.k.double(), inp.v.double()

    row0 = 0
    for s in range(case.S):
        if case.kind == "decode":
            n_rows, length = 1, case.ctx[s]
        elif case.kind == "context":
            n_rows, length = case.q_lens[s], case.ctx[s]
        else:
            n_rows, length = case.q_lens[s], case.q_lens[s]
        firsts = (split_first_tokens(length, case.window, n_splits)
                  if case.kind == "decode" else [])
        vis = [_visible(case, length, n_rows, r, mutate, s, firsts)
               for r in range(n_rows)]
        cols = sorted(set(j for v_ in vis for j in v_))
        if not cols:
            sig.append(tuple(() for _ in vis))
            row0 += n_rows
            continue
        col_t = torch.tensor(cols, dtype=torch.long)
        if paged:
            blk = col_t // PAGE
            if mutate == "ignore_table":
                ids = 1 + s * width + blk
            elif mutate == "row_stride":
                ids = flat[(s * inp.needed_blocks + blk) % flat.numel()]
            else:
                ids = bt[s, blk]
            ids = ids % inp.num_blocks
            off = col_t % PAGE
            K = kc[ids, :, off]           # [n, Hkv, D]
            V = vc[ids, :, off]
            src = (ids * PAGE + off).tolist()
        else:
            gi = int(inp.cu_seqlens[s]) + col_t
            K, V = kf[gi], vf[gi]
            src = gi.tolist()
        src_of = dict(zip(cols, src))
        sig.append(tuple(tuple(src_of[j] for j in v_) for v_ in vis))
        index_of = {j: i for i, j in enumerate(cols)}
        mask = torch.zeros(n_rows, len(cols), dtype=torch.bool)
        for r, v_ in enumerate(vis):
            if v_:
                mask[r, [index_of[j] for j in v_]] = True
        Kh, Vh = K[:, kvmap], V[:, kvmap]           # [n, H, D]
        qs = q[row0:row0 + n_rows]                  # [R, H, D]
        sc = torch.einsum("rhd,nhd->hrn", qs, Kh) * inp.scale
        sc = sc.masked_fill(~mask[None], float("-inf"))
        mx = sc.max(dim=-1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        p = torch.exp(sc - mx)                      # masked -> exp(-inf) = 0
        l = p.sum(dim=-1, keepdim=True)
        p = torch.where(l > 0, p / l.clamp_min(1e-300), torch.zeros_like(p))
        out[row0:row0 + n_rows] = torch.einsum("hrn,nhd->rhd", p, Vh)
        absmass[row0:row0 + n_rows] = torch.einsum("hrn,nhd->rhd", p, Vh.abs())
        row0 += n_rows
    return out, absmass, tuple(sig)


@functools.lru_cache(maxsize=None)
def expected(case: Case):
    """(out, absmass) of the unmutated reference; cached, do not modify."""
    out, absmass, _ = reference(build(case))
    return out, absmass


# ---------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------
def allowance(ref: torch.Tensor, absmass: torch.Tensor,
              eps_p: float) -> torch.Tensor:
    return OUT_ULP * ref.abs() + eps_p * absmass + ABS_FLOOR


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, absmass: torch.Tensor,
                eps_p: float) -> float:
    """max over elements of |got - ref| / allowance; inf if anything in
    ``got`` is not finite. <= 1 passes."""
    got = got.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    r = (got - ref).abs() / allowance(ref, absmass, eps_p)
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------
# running a case on the GPU kernels
# ---------------------------------------------------------------------------
def _strided_rows(x: torch.Tensor, dev, lead: int, tail: int) -> torch.Tensor:
    """[T, heads, D] bf16 on ``dev`` as a view of a wider row buffer, the way
    the model passes slices of the fused qkv projection. lead/tail are in
    elements and multiples of 8 (the kernels load 16 B vectors)."""
    T, h, d = x.shape
    wide = torch.full((T, lead + h * d + tail), 777.0, dtype=torch.bfloat16,
                      device=dev)
    view = wide[:, lead:lead + h * d].view(T, h, d)
    view.copy_(x.to(torch.bfloat16))
    assert not view.is_contiguous() or T == 1
    return view


def _cache_to(x: torch.Tensor, case: Case, dev) -> torch.Tensor:
    dt = torch.float8_e4m3fn if case.fp8 else torch.bfloat16
    return x.to(dt).to(dev)


def run_gpu(case: Case, dev) -> torch.Tensor:
    """Run the case through kserve_amd.ops on ``dev``; returns the bf16
    output. q (and k/v for flash) are strided views; the decode output is
    pre-filled with a sentinel that must not survive."""
    from kserve_amd import ops

    inp = build(case)
    q = _strided_rows(inp.q, dev, 32, 32)
    if case.kind == "flash":
        k = _strided_rows(inp.k, dev, 8, 24)[:inp.T]
        v = _strided_rows(inp.v, dev, 16, 8)[:inp.T]
        cu = inp.cu_seqlens.to(dev)
        if case.causal:
            return ops.flash_prefill_varlen(q, k, v, cu, inp.max_seqlen,
                                            inp.scale, window=case.window)
        assert case.window == 0
        return ops.flash_attn_varlen(q, k, v, cu, inp.max_seqlen, inp.scale,
                                     causal=False)
    kc = _cache_to(inp.k_cache, case, dev)
    vc = _cache_to(inp.v_cache, case, dev)
    bt = inp.block_tables.to(dev)
    cl = inp.context_lens.to(dev)
    if case.kind == "decode":
        out = torch.full(inp.q.shape, OUT_SENTINEL, dtype=torch.bfloat16,
                         device=dev)
        got = ops.paged_attention_decode(q, kc, vc, bt, cl, inp.scale,
                                         out=out, window=case.window)
        assert got is out
        assert not bool((out == OUT_SENTINEL).any()), \
            f"{case.name}: output rows left unwritten"
        return out
    return ops.context_attention_varlen(
        q, kc, vc, bt, inp.cu_seqlens_q.to(dev), cl, inp.max_q_len,
        inp.scale, window=case.window)


def gpu_ratio(case: Case, dev, eps_p: Optional[float] = None) -> float:
    ref, absmass = expected(case)
    got = run_gpu(case, dev)
    return worst_ratio(got, ref, absmass, case.eps_p if eps_p is None else eps_p)
