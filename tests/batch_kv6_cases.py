"""Seeded inputs of the ragged MXFP6 batch cases (tests/test_hip_batch_kv6.py, cases (b) and (c)), built on the CPU so that the GPU
test and the CPU test of its precondition (tests/test_batch_kv6_cpu.py) draw exactly the same rows, slot maps, score state and tokens.

The generator is that of tests/batch_kv8_cases.py — same draw order — over a table of its own: entries of 2, 17, 96, 300 and 2049
slots (an extent that ends right behind, inside and in front of the kv6 stream's 16-row wave-loads — head_dim 128: a row is a 4-lane
group, 4 rows in flight per lane group — a split path through several wave-loads per split, and the full north-star length) among
9, 33, 65, 130 and 1301.  Entries evict only with a budget >= 30, as there.  Both shapes are head_dim 128:
GQA x 2 in fp16 and GQA x 4 in bf16, the widest factor a kv6 step takes."""
import torch

from tests.batch_kv8_cases import STEPS, fill_entry, plan_kw      # noqa: F401  (re-exported: one way to fill a bank and to plan an entry)

RAGGED_T = (2, 9, 17, 33, 65, 96, 130, 300, 1301, 2049)
OFFS = {2: 0, 9: 0, 17: 5, 33: 0, 65: 0, 96: 3, 130: 13, 300: 21, 1301: 7, 2049: 0}      # per-entry score_off
EVICTS = {2: False, 9: False, 17: False, 33: True, 65: True, 96: True, 130: True, 300: True, 1301: True, 2049: True}

SHAPES = {"d128_gqa2_f16": (128, 8, 4, torch.float16), "d128_gqa4_bf16": (128, 8, 2, torch.bfloat16)}      # D, Hq, H, element type
POLICIES = ("roco", "h2o_head")
# (the seeds of tests/batch_kv4_cases.py: under MXFP6 rows too they leave the decisions of roco and h2o_head well defined on both
#  shapes — tests/test_batch_kv6_cpu.py checks it on the reference side)
SEEDS = {("d128_gqa2_f16", 0): 431, ("d128_gqa2_f16", 1): 432, ("d128_gqa4_bf16", 0): 531, ("d128_gqa4_bf16", 1): 532}


def inputs(shape, draw):
    """tests.batch_kv8_cases.inputs for the shapes and seeds above.  draw 0: short entries first, 1: short entries last.  Returns
    (entries, tokens): per entry its length T, score offset, score-row width W, whether it evicts, its T - 1 rows in position order
    (k0, v0 [H, T-1, D]), the physical row of every position (perm) and a warm score state over its W - 1 scored rows; per step the
    (q, k_new, v_new) of the whole table."""
    D, Hq, H, dtype = SHAPES[shape]
    g = torch.Generator().manual_seed(SEEDS[(shape, draw)])
    # bf16 outputs under the flat 1e-3 bar: V at 1/4 scale and within +-0.49, as tests/batch_kv8_cases.py explains (an entry of a few
    # slots averages nothing away, and a bf16 output in [0.5, 1) carries 1.95e-3 of rounding of its own)
    v_scale, v_max = (0.25, 0.49) if dtype is torch.bfloat16 else (1.0, float("inf"))
    lens = list(RAGGED_T) if draw == 0 else list(reversed(RAGGED_T))
    entries = []
    for T in lens:
        n, W = T - 1, T - OFFS[T]
        entries.append(dict(T=T, off=OFFS[T], W=W, evict=EVICTS[T],
                            k0=torch.randn(H, n, D, generator=g).to(dtype), v0=(torch.randn(H, n, D, generator=g) * v_scale).clamp(-v_max, v_max).to(dtype),
                            perm=torch.argsort(torch.rand(H, n, generator=g), dim=-1).int(), warm=torch.rand(H, W - 1, generator=g) * 1e-3))
    B = len(lens)
    tokens = [(torch.randn(B, Hq, 1, D, generator=g).to(dtype), torch.randn(B, H, 1, D, generator=g).to(dtype),
               (torch.randn(B, H, 1, D, generator=g) * v_scale).clamp(-v_max, v_max).to(dtype)) for _ in range(STEPS)]
    return entries, tokens


# ---- (c) lockstep: four sequences of different lengths and budgets, 32 steps, sequence 2 retired after step 15 --------------------------
LOCK = dict(prompts={0: 12, 1: 20, 2: 33, 3: 47}, budgets={0: 30, 1: 36, 2: 32, 3: 40}, scored={0: 20, 1: 30, 2: 28, 3: 10})
LOCK_STEPS, LOCK_RETIRE = 32, (2, 15)
LOCK_SHAPE = (4, 4, 128)      # Hq, H, D
LOCK_SEED = 1900


def lockstep_inputs(s):
    """Sequence `s` of LOCK: (entry for fill_entry — prompt + scored rows already in the cache —, its LOCK_STEPS tokens (q, k, v)).
    Every sequence draws from a generator of its own, so a run without one sequence sees the same rows and tokens for the others."""
    Hq, H, D = LOCK_SHAPE
    g = torch.Generator().manual_seed(LOCK_SEED + 17 * s)
    n, g0 = LOCK["prompts"][s] + LOCK["scored"][s], LOCK["scored"][s]
    entry = dict(W=LOCK["budgets"][s] + 1, k0=torch.randn(H, n, D, generator=g).half(), v0=torch.randn(H, n, D, generator=g).half(),
                 perm=torch.argsort(torch.rand(H, n, generator=g), dim=-1).int(), warm=torch.rand(H, g0, generator=g) * 1e-3)
    tokens = [[torch.randn(1, hh, 1, D, generator=g).half() for hh in (Hq, H, H)] for _ in range(LOCK_STEPS)]
    return entry, tokens


def lockstep_evicts(s, step):
    """Does sequence `s` evict at step `step` — as the decode loop decides, ITS length against ITS budget: it starts with its scored
    rows in the cache and holds budget + 1 rows from the step on at which it first exceeds the budget."""
    return LOCK["scored"][s] + step + 1 > LOCK["budgets"][s]
