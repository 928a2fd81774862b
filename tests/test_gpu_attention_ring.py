"""LDS-ring decode attention kernel (KS_ATTN_V4RING=1) against the pipelined
kernel it shares its arithmetic with (KS_ATTN_V4RING=0 KS_ATTN_V4PIPE=1).

CPU: the lane -> source-address and lane -> LDS-read-address maps of
kserve_amd/ops/csrc/attn_ring_layout.h, which the kernel is built from, are
printed by a small host program (tests/ring_layout_check.cpp) and checked
here: every byte of a slot half written once per page, every operand read
returning the bytes the pipelined kernel loads for that lane, nothing outside
the slot.

GPU: the switches are read once per process, so each side runs in a child of
its own (this file with --child), one after the other; a child that dies ends
the comparison there. Both children build the same seeded needle/poison
inputs (tests/attention_cases.py: permuted block tables wider than needed,
unused entries pointing at poison pages) and write raw output bits to an
.npz; the parent allows zero differing elements, in the bf16 outputs and in
the fp32 split partials. The ring child also reports err/allowance against
the fp64 reference at eps_P = 2^-12.

Shapes: Hkv 2, D 128, page 16, 129 sequences (the slot starts above 128).
The ring has R = 4 slots and walks page pairs with R - 2 = 2 pages fetched
ahead, so contexts 1..33 cover a prologue with fewer pages than it fetches,
16R - 1 .. 16(R + 1) + 1 every wrap phase of the ring, the odd contexts the
tail whose second page is a clamped re-read, and 1023..2049 the 64-entry
block-id chunk: its refill at page 64, a fetch that crosses into the next
chunk, and the clamp to the last entry (1025 = 65 pages, 2049 = 129 pages).
At 129 sequences x 2 kv heads the launcher's heuristic takes 7 splits
(2048 / 258); the unsplit cases therefore run under KS_ATTN_SPLIT=1, one case
runs the heuristic as it is, and one runs 3 splits through the binding that
returns the partials (short contexts give it empty splits).
"""

import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import attention_cases as ac

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "kserve_amd", "ops", "csrc")
CHILD_TIMEOUT_S = 180  # a healthy child takes ~15 s; this only bounds a hang

R = 4  # V4RING_SLOTS in attention_decode.hip
S = 129
_EDGES = (1, 15, 16, 17, 31, 32, 33,
          16 * R - 1, 16 * R, 16 * R + 1, 16 * (R + 1) + 1,
          1023, 1024, 1025, 1041, 2049)
_WIN_EDGES = (33, 100, 1025)


def _ctx(edges):
    return tuple(edges) + (1,) * (S - len(edges))


CASES = [ac.Case(f"ring_kv2g{g}", "decode", 2, g, 128, ctx=_ctx(_EDGES),
                 seed=900 + g) for g in (1, 2, 3, 4)]
CASES.append(ac.Case("ring_kv2g4_w40", "decode", 2, 4, 128,
                     ctx=_ctx(_WIN_EDGES), window=40, seed=910))
SPLIT_CASE = CASES[3]      # group 4, 3 splits through the partials binding
SPLIT_N = 3
AUTO_SPLIT_CASE = CASES[2]  # group 3 under the launcher's own split count

SIDES = {
    "ring": {"KS_ATTN_V4RING": "1"},
    "pipe": {"KS_ATTN_V4RING": "0", "KS_ATTN_V4PIPE": "1"},
}


# ---------------------------------------------------------------------------
# CPU: the layout maps
# ---------------------------------------------------------------------------
def _host_compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cc)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def _layout_maps(tmp_path, extra=()):
    exe = str(tmp_path / "ring_layout_check")
    subprocess.run(
        [_host_compiler(), "-std=c++17", "-O1", "-g", *extra, f"-I{CSRC}",
         os.path.join(REPO, "tests", "ring_layout_check.cpp"), "-o", exe],
        check=True, timeout=120)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, text=True,
                          timeout=60)
    rows = [ln.split() for ln in proc.stdout.splitlines()]
    return proc.returncode, rows


def test_ring_layout_maps(tmp_path):
    rc, rows = _layout_maps(tmp_path)
    half, chunk = 4096, 16
    for tag in ("K", "V"):
        written = np.full(half, -1, dtype=np.int64)   # LDS byte -> source byte
        for r in rows:
            if r[0] != tag:
                continue
            wave, lane, src, dst = map(int, r[1:])
            assert dst == (wave * 64 + lane) * chunk   # what the load does
            assert 0 <= src and src + chunk <= half and src % chunk == 0
            assert 0 <= dst and dst + chunk <= half
            assert (written[dst:dst + chunk] == -1).all(), "byte written twice"
            written[dst:dst + chunk] = np.arange(src, src + chunk)
        assert (written >= 0).all(), "byte of the slot never written"
        assert sorted(written.tolist()) == list(range(half))
        n = 0
        for r in rows:
            if r[0] != tag.lower():
                continue
            lane, c, rd = map(int, r[1:])
            assert 0 <= rd and rd + chunk <= half
            if tag == "K":   # kreg[c] of lane (tok, part) in the v4p layout
                want = ((lane >> 2) * 128 + (lane & 3) * 32 + c * 8) * 2
            else:            # vreg[q4]: token vtok + 4 * q4, dims 8 * (lane & 15)
                want = (((lane >> 4) + 4 * c) * 128 + (lane & 15) * 8) * 2
            assert written[rd:rd + chunk].tolist() == \
                list(range(want, want + chunk)), (tag, lane, c)
            n += 1
        assert n == 64 * 4
    assert rc == 0 and rows[-1] == ["bad", "0"]


def test_ring_layout_maps_sanitized(tmp_path):
    """The same host program under ASan + UBSan (a stand-alone binary)."""
    rc, rows = _layout_maps(
        tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert rc == 0 and rows[-1] == ["bad", "0"]


def test_cases_reach_the_slot():
    for c in CASES:
        for env in SIDES.values():
            assert ac.expected_decode_kernel(c, env) == "v4", c.name
    # the heuristic does split this slot at 129 sequences
    assert ac.decode_n_splits(S, 2 * 3, 2, 132) == 7


# ---------------------------------------------------------------------------
# GPU: child and parent
# ---------------------------------------------------------------------------
def _bits(t):
    import torch
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy()
    return t.view(torch.int32).numpy()


def _child(side, path):
    import torch
    from kserve_amd import ops
    import kserve_amd_C

    for k, v in SIDES[side].items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    assert torch.cuda.is_available() and ops.has_native()
    dev = torch.device("cuda:0")
    arrays, ratios = {}, {}

    def check(name, case, got):
        arrays[name] = _bits(got)
        if side == "ring":
            ref, absmass = ac.expected(case)
            ratios[name] = ac.worst_ratio(got, ref, absmass, ac.EPS_FMA)

    # the unsplit cases need KS_ATTN_SPLIT=1, which is read once per process:
    # this child is started with it, and the two split runs below do not
    # depend on it (an explicit count; the heuristic run is a third process)
    if os.environ.get("KS_ATTN_SPLIT") == "1":
        for case in CASES:
            check(case.name, case, ac.run_gpu(case, dev))
        inp = ac.build(SPLIT_CASE)
        q = ac._strided_rows(inp.q, dev, 32, 32)
        out = torch.full(inp.q.shape, ac.OUT_SENTINEL, dtype=torch.bfloat16,
                         device=dev)
        po, pml = kserve_amd_C.paged_attention_decode_split(
            out, q, ac._cache_to(inp.k_cache, SPLIT_CASE, dev),
            ac._cache_to(inp.v_cache, SPLIT_CASE, dev),
            inp.block_tables.to(dev), inp.context_lens.to(dev), inp.scale, 0,
            SPLIT_N)
        check("split3", SPLIT_CASE, out)
        arrays["split3_part_ml"] = _bits(pml)
        # an empty split writes its (m, l) only: mask part_out by l > 0
        live = (pml[..., 1] > 0).unsqueeze(-1)
        arrays["split3_part_out"] = _bits(torch.where(live, po,
                                                      torch.zeros_like(po)))
        arrays["split3_live"] = live.cpu().numpy()
    else:
        assert "KS_ATTN_SPLIT" not in os.environ
        check("auto_split", AUTO_SPLIT_CASE, ac.run_gpu(AUTO_SPLIT_CASE, dev))
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(json.dumps({"side": side, "ratios": ratios}))
    sys.stdout.flush()
    return 0


_runs = {"done": False, "error": None, "out": {}, "ratios": {}}


def _run_children(tmp):
    """ring and pipe, unsplit then heuristic: four children, one at a time."""
    if _runs["done"]:
        return
    _runs["done"] = True
    base = {k: v for k, v in os.environ.items()
            if not k.startswith(("KS_ATTN_", "KS_FP8_"))}
    for split in ("1", None):
        for side, env in SIDES.items():
            path = os.path.join(tmp, f"{side}_{split}.npz")
            e = dict(base, **env)
            if split:
                e["KS_ATTN_SPLIT"] = split
            try:
                proc = subprocess.run(
                    [sys.executable, "-m", "tests.test_gpu_attention_ring",
                     "--child", side, path],
                    env=e, cwd=REPO, timeout=CHILD_TIMEOUT_S,
                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                _runs["error"] = f"child {side} ran into its time limit"
                return
            if proc.returncode != 0:
                _runs["error"] = (f"child {side} (split={split}) exited "
                                  f"{proc.returncode}\n{proc.stderr[-2000:]}")
                return
            rec = json.loads([ln for ln in proc.stdout.splitlines()
                              if ln.startswith("{")][-1])
            _runs["ratios"].update(rec["ratios"])
            with np.load(path) as z:
                _runs["out"].setdefault(side, {}).update(
                    {k: z[k] for k in z.files})


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    _run_children(str(tmp_path_factory.mktemp("ring")))
    if _runs["error"]:
        pytest.fail(_runs["error"])
    return _runs


_OUTPUTS = [c.name for c in CASES] + ["split3", "auto_split"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _OUTPUTS)
def test_ring_equals_pipelined_bit_for_bit(runs, name):
    ring, pipe = runs["out"]["ring"][name], runs["out"]["pipe"][name]
    assert ring.shape == pipe.shape and ring.dtype == np.int16
    ndiff = int((ring != pipe).sum())
    print(f"{name}: {ndiff} of {ring.size} bf16 outputs differ")
    assert ndiff == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["split3_part_out", "split3_part_ml"])
def test_ring_split_partials_bit_for_bit(runs, name):
    ring, pipe = runs["out"]["ring"][name], runs["out"]["pipe"][name]
    assert ring.shape == pipe.shape and ring.dtype == np.int32
    live = runs["out"]["pipe"]["split3_live"]
    assert live.any() and not live.all()   # full and empty splits both occur
    assert (runs["out"]["ring"]["split3_live"] == live).all()
    ndiff = int((ring != pipe).sum())
    print(f"{name}: {ndiff} of {ring.size} fp32 partials differ")
    assert ndiff == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", _OUTPUTS)
def test_ring_passes_fp64_reference(runs, name):
    ratio = runs["ratios"][name]
    print(f"{name}: err/allowance = {ratio:.3f}")
    assert ratio <= 1.0


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    sys.exit(_child(sys.argv[2], sys.argv[3]))
