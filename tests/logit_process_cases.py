"""Cases and an fp64 reference for ops.logit_process, written from the
contract (docs/DESIGN.md section 11), not from the code under test.

Per element of row s with slot = row_slot[s] inside [0, slots):
  1. a bias entry (ids[slot, :len[slot]]) for the token:
        x = bf16(x + bias)                       (first rounding)
  2. counts[slot, i] > 0:
        v = x;  repetition != 1: v = v / rep if v > 0 else v * rep
        v = v - presence - frequency * count
        x = bf16(v)                              (second rounding)
  3. otherwise x keeps its bits.
Rows whose slot is outside [0, slots) keep their bits.

Tolerance (derived, not tuned): the implementations compute step 2 in fp32,
possibly with a reciprocal instead of a division and a fused multiply-add,
which is an error of a few fp32 ulps (2^-22 relative) against the 2^-9 of
half a bf16 ulp. So only a value within that distance of a rounding tie can
land on the neighbouring bf16 value: every output must be within ONE bf16
ulp (one step in the ordered bit patterns) of the reference rounded to
bf16, non-finite values must match exactly, and every element of rule 3 and
every slot-less row must be bit-identical to the input.
"""

import torch

SLOTS = 6
MAX_BIAS = 8

# values put under the first counted tokens of every slotted row: positive,
# negative, zero and -inf logits all meet a positive count
SPECIAL_LOGITS = [3.5, -2.25, 0.0, float("-inf")]
COUNT_CYCLE = [1, 2, 300, 1, 2]
PRESENCE = [0.5, 0.0, -0.75, 1.25]
FREQUENCY = [0.25, 0.125, -0.0625, 0.0]
REPETITION = [2.0, 1.0, 0.5, 1.3]
BIAS_VALS = [2.0, -3.5, 100.0]


def row_slots(S, slots=SLOTS):
    """A non-identity permutation of the slots over the rows (5s + 2 mod 6:
    2, 1, 0, 5, 4, 3), with row 1 slot-less (-1) and the last row out of
    range when there are rows to spare."""
    rs = [(5 * s + 2) % slots for s in range(S)]
    if S >= 2:
        rs[1] = -1
    if S >= 3:
        rs[S - 1] = slots + 3
    return rs


def build_case(S, V, slots=SLOTS, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + S * 1009 + V)
    logits = (torch.randn(S, V, generator=g) * 4.0).to(torch.bfloat16)
    counts = torch.zeros(slots, V, dtype=torch.int32)
    n_counted = min(V, 12) if V < 24 else 12
    if V >= 4:
        n_counted = min(n_counted, V - 2)  # leave uncounted tokens
    counted = []
    for sl in range(slots):
        toks = torch.randperm(V, generator=g)[:n_counted].tolist()
        counted.append(toks)
        for j, t in enumerate(toks):
            counts[sl, t] = COUNT_CYCLE[(j + sl) % len(COUNT_CYCLE)]
    rs = row_slots(S, slots)
    for s, sl in enumerate(rs):
        if 0 <= sl < slots:
            for j, t in enumerate(counted[sl][: len(SPECIAL_LOGITS)]):
                logits[s, t] = SPECIAL_LOGITS[(j + s) % len(SPECIAL_LOGITS)]
    # bias lists: slot 3 has none; the others one COUNTED token and then
    # uncounted ones; entries past bias_len are stale and must be ignored
    bias_ids = torch.zeros(slots, MAX_BIAS, dtype=torch.int32)
    bias_vals = torch.full((slots, MAX_BIAS), 1000.0, dtype=torch.float32)
    bias_len = torch.zeros(slots, dtype=torch.int32)
    for sl in range(slots):
        if sl == 3:
            continue
        ids = [counted[sl][min(1, len(counted[sl]) - 1)]]
        for t in range(V):
            if len(ids) == len(BIAS_VALS):
                break
            if counts[sl, t] == 0:
                ids.append(t)
        for j, t in enumerate(ids):
            bias_ids[sl, j] = t
            bias_vals[sl, j] = BIAS_VALS[j]
        bias_len[sl] = len(ids)
    pick = lambda vals: torch.tensor(
        [vals[s % len(vals)] for s in range(S)], dtype=torch.float32
    )
    return {
        "S": S, "V": V, "slots": slots,
        "logits": logits,
        "counts": counts,
        "row_slot": torch.tensor(rs, dtype=torch.int32),
        "presence": pick(PRESENCE),
        "frequency": pick(FREQUENCY),
        "repetition": pick(REPETITION),
        "bias_ids": bias_ids,
        "bias_vals": bias_vals,
        "bias_len": bias_len,
    }


# the case set of the CPU tests: every feature above meets every other
CPU_SHAPES = [(6, 64), (6, 257), (3, 40), (1, 7), (1, 1)]


def op_args(case, device="cpu"):
    """Positional arguments of ops.logit_process after `logits`."""
    return tuple(
        case[k].to(device)
        for k in (
            "counts", "row_slot", "presence", "frequency", "repetition",
            "bias_ids", "bias_vals", "bias_len",
        )
    )


def _bf16(x64):
    return x64.to(torch.float32).to(torch.bfloat16)


def reference(case, mutant=None):
    """fp64 evaluation of the contract; returns (ref, touched): the exact
    value before the final rounding as float64 [S, V], and a bool mask of
    the elements rules 1 or 2 apply to. `mutant` names one deliberate
    deviation (the CPU test shows the case set catches each)."""
    S, V, slots = case["S"], case["V"], case["slots"]
    x = case["logits"].to(torch.float64).clone()
    touched = torch.zeros(S, V, dtype=torch.bool)
    for s in range(S):
        sl = int(case["row_slot"][s])
        if mutant == "slot_is_row":
            sl = s
        if not 0 <= sl < slots:
            continue
        p = float(case["presence"][s])
        f = float(case["frequency"][s])
        r = float(case["repetition"][s])
        bias = {}
        for j in range(int(case["bias_len"][sl])):
            bias[int(case["bias_ids"][sl, j])] = float(case["bias_vals"][sl, j])
        cnt = case["counts"][sl].tolist()
        if mutant == "presence_at_zero":
            todo = range(V)
        else:
            todo = sorted(set(bias) | {i for i in range(V) if cnt[i] > 0})
        for i in todo:
            if not 0 <= i < V:
                continue
            c = cnt[i]
            v = float(x[s, i])  # Python floats are fp64 and keep +-inf
            hit = False
            if i in bias and mutant != "bias_after":
                v = float(_bf16(torch.tensor(v + bias[i], dtype=torch.float64)))
                hit = True
            if c > 0 or mutant == "presence_at_zero":
                if c > 0 and r != 1.0:
                    if v > 0 or mutant == "no_sign_branch":
                        v = v / r
                    else:
                        v = v * r
                cc = min(c, 1) if mutant == "frequency_once" else c
                v = v - p - f * cc
                hit = True
            if i in bias and mutant == "bias_after":
                v = v + bias[i]
                hit = True
            x[s, i] = v
            touched[s, i] = hit
    return x, touched


MUTANTS = [
    "no_sign_branch",
    "presence_at_zero",
    "frequency_once",
    "slot_is_row",
    "bias_after",
]


def _ordered(bits16):
    """int16 bf16 patterns -> integers that order like the values."""
    u = bits16.to(torch.int32) & 0xFFFF
    return torch.where(u >= 0x8000, 0xFFFF - u, u | 0x8000)


def violations(out, case, ref=None):
    """Elements of `out` (bf16 [S, V]) that miss the tolerance: a list of
    (row, token, got, want) with at most a few entries, empty when the
    output is right."""
    if ref is None:
        ref = reference(case)
    exact, touched = ref
    out = out.cpu()
    want = _bf16(exact)
    got_bits = out.view(torch.int16)
    want_bits = want.view(torch.int16)
    in_bits = case["logits"].view(torch.int16)
    dist = (_ordered(got_bits) - _ordered(want_bits)).abs()
    finite = torch.isfinite(exact) & torch.isfinite(out.to(torch.float64))
    bad = torch.where(finite, dist > 1, got_bits != want_bits)
    bad |= ~touched & (got_bits != in_bits)
    idx = bad.nonzero()[:5].tolist()
    return [
        (s, i, float(out[s, i]), float(exact[s, i])) for s, i in idx
    ]
