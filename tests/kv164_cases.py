"""The decode-step cases of the 16-bit-key / MXFP4-value ("kv164") tests and their seeded inputs, shared by the CPU precondition
(tests/test_kv164_cpu.py: the oracle alone, on UNQUANTISED K — V cannot touch a decision) and the GPU tests (tests/test_hip_kv164.py).
The cases, the seed and the inputs are those of tests/kv6_cases.py (seed 5: every decision of the six scored cases is well defined on
unquantised keys), unchanged.

TWIN_EXTRA: cases of the 16-bit-twin test alone (no oracle, so no precondition): the GQA factors the kv6 cases cannot have — those of
tests/kv84_cases.py (GQA x 8 on the 8-wave, 4-wave and split paths, GQA x 2 on the 4-wave build)."""
import torch

from tests.kv6_cases import BF, D, F16, SCORED, SEED, STEPS, inputs, plan_kw, v_scale      # noqa: F401  (re-exported)
from tests.kv84_cases import TWIN_EXTRA, spread_rows      # noqa: F401  (re-exported)


def dequant_ref(k, v):
    """What a kv164 bank holds of rows k, v, as fp32: K as it is, V through the kv4 rule."""
    from tests import kv4_ref
    return k.float(), kv4_ref.dequant(*kv4_ref.quantize(v))


def edge_v(kind, shape, gen):
    """Appended V rows [..., 128] (fp16) that a wrong lane-quad maximum, exponent store or exponent byte index turns into a gross error.
    A block is shared by FOUR lanes of 8 elements each.  Block b of a row has magnitude 2^(4 b' - 10) (b' a permutation of 0..3 per row:
    widely different exponents), and within each block the maximum lies only in the 8-element piece `kind` (0..3) — the other three
    pieces are 64 x smaller; kind 'zero': as kind 0, with block 1 all zero."""
    piece = 0 if kind == "zero" else int(kind)
    v = torch.zeros(*shape, 128)
    flat = v.view(-1, 4, 4, 8)
    for i in range(flat.shape[0]):
        order = torch.randperm(4, generator=gen)
        for b in range(4):
            flat[i, b] = (torch.rand(4, 8, generator=gen) * 2 - 1) * 2.0 ** (4 * int(order[b]) - 16)
            flat[i, b, piece] = (torch.rand(8, generator=gen) * 0.5 + 0.5) * (torch.randint(0, 2, (8,), generator=gen) * 2 - 1) * 2.0 ** (4 * int(order[b]) - 10)
        if kind == "zero":
            flat[i, 1] = 0
    return v.half()
